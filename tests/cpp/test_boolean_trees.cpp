// tests/cpp/test_boolean_trees.cpp — TEST: the C++ host layer's nested boolean filters (BoolTree,
// And::tree / Or::tree, IRS_HIP_TREE_NODE) against the oracle's C API, composed per leaf: every
// by_term is the oracle's Or over that one entry with its boost product and index-global statistics
// (absent from the segment: nothing), a node's match and score are put together here by a recursive
// walk of the filter, apart from prepare().  And what the layer refuses.  Linked against
// libirs_hip.so on a GPU box, or against the CPU emulator build of the same sources.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "irs_hip.hpp"
#include "oracle.h"
#include "synth_index.h"

using namespace irs_hip_host;

#define REQUIRE(c)                                                          \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #c); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

namespace {

struct Segment {  // a synthetic segment and everything the two sides need of it
  irs_synth_index* idx = nullptr;
  const uint8_t *doc = nullptr, *norms = nullptr;
  uint64_t doc_len = 0, norm_count = 0;
  const irs_hip_term_meta* metas = nullptr;
  uint32_t num_terms = 0, num_docs = 0;
  std::unique_ptr<SegmentReader> reader;

  Segment(uint32_t docs, uint64_t first_doc, uint32_t max_rank) : num_docs{docs} {
    irs_synth_params p{};
    p.seed = 20260926;
    p.first_doc = first_doc;
    p.num_docs = docs;
    p.vocab_log2 = 20;
    p.max_rank = max_rank;
    p.layout = IRS_SYNTH_LAYOUT_SIMD4;
    p.mean_len = 100;
    p.stddev_len = 30;
    if (irs_synth_build(&p, &idx) != 0) throw std::runtime_error("irs_synth_build");
    doc = irs_synth_doc_bytes(idx, &doc_len);
    norms = irs_synth_norms(idx, &norm_count);
    static_assert(sizeof(irs_synth_term_meta) == sizeof(irs_hip_term_meta), "same layout");
    static_assert(sizeof(orc_term_meta) == sizeof(irs_hip_term_meta), "same layout");
    metas = reinterpret_cast<const irs_hip_term_meta*>(irs_synth_term_metas(idx, &num_terms));
    irs_hip_segment_desc d{};
    d.device = 0;
    d.layout = IRS_HIP_LAYOUT_SIMD4;
    d.doc_file = doc;
    d.doc_file_len = doc_len;
    d.num_docs = num_docs;
    d.has_freq = 1;
    d.norms = norms;
    d.norm_width = 1;
    d.norm_min_doc = 1;
    d.norm_count = norm_count;
    d.terms = metas;
    d.num_terms = num_terms;
    reader = std::make_unique<SegmentReader>(d);
  }
  ~Segment() {
    reader.reset();
    irs_synth_free(idx);
  }
  SegmentStats stats() const {
    return SegmentStats{irs_synth_docs_with_field(idx), irs_synth_total_term_freq(idx), metas,
                        num_terms};
  }
  orc_segment oracle_view() const {
    orc_segment s{};
    s.doc_file = doc;
    s.doc_file_len = doc_len;
    s.layout = ORC_LAYOUT_SIMD4;
    s.num_docs = num_docs;
    s.norms = norms;
    s.norm_width = 1;
    return s;
  }
};

bool close_rel(double a, double b) { return std::fabs(a - b) <= 1e-5 * std::fabs(b); }

template<typename E, typename F>
bool throws(F&& f) {
  try {
    f();
  } catch (const E&) {
    return true;
  } catch (...) {
    return false;
  }
  return false;
}

// One segment's side of the composition
struct Composer {
  const Segment& seg;
  const std::vector<SegmentStats>& index;
  orc_scorer osc;
  size_t n1;
  bool failed = false;

  // (matched, score) of a by_term with the boost product `boost`
  void leaf(uint32_t term, float boost, std::vector<uint8_t>& m, std::vector<double>& sc) {
    m.assign(n1, 0);
    sc.assign(n1, 0.0);
    if (term >= seg.num_terms || !seg.metas[term].docs_count) return;   // absent: matches nothing
    orc_term_meta meta;
    std::memcpy(&meta, &seg.metas[term], sizeof meta);
    uint64_t dwt = 0, dwf = 0, ttf = 0;
    for (const auto& s : index) {
      dwt += s.docs_count(term);
      dwf += s.docs_with_field;
      ttf += s.total_term_freq;
    }
    std::vector<float> f(n1);
    const orc_segment view = seg.oracle_view();
    if (orc_score_all(&view, &meta, 1, ORC_OP_OR, &osc, &boost, dwf, &dwt, ttf, f.data(), m.data()) < 0) failed = true;
    for (size_t d = 0; d < n1; ++d) sc[d] = m[d] ? double(f[d]) : 0.0;
  }

  void node(const BoolTree& t, float mult, std::vector<uint8_t>& m, std::vector<double>& sc) {
    using K = BoolTree::Kind;
    if (t.kind == K::kTerm) return leaf(t.term.term, mult * t.term.boost, m, sc);
    mult *= t.boost;
    std::vector<uint32_t> n_match(n1, 0);
    std::vector<uint8_t> barred(n1, 0);
    std::vector<double> sum(n1, 0.0);
    uint32_t n_pos = 0;
    for (const BoolTree& s : t.subs) {
      const BoolTree* f = &s;
      bool neg = false;
      while (f->kind == K::kNot) {
        f = &f->subs[0];
        neg = !neg;
      }
      std::vector<uint8_t> cm;
      std::vector<double> cs;
      node(*f, neg ? 1.f : mult, cm, cs);
      n_pos += neg ? 0u : 1u;
      for (size_t d = 0; d < n1; ++d) {
        if (!cm[d]) continue;
        if (neg) {
          barred[d] = 1;
        } else {
          ++n_match[d];
          sum[d] += cs[d];
        }
      }
    }
    const uint32_t need = t.kind == K::kAnd ? n_pos : std::max<uint32_t>(1, t.min_match_count);
    m.assign(n1, 0);
    sc.assign(n1, 0.0);
    for (size_t d = 0; d < n1; ++d)
      if (n_match[d] >= need && !barred[d]) {
        m[d] = 1;
        sc[d] = sum[d];
      }
  }
};

BoolTree L(uint32_t t, float boost = 1.f) { return BoolTree::leaf(t, boost); }

}  // namespace

int main() {
  constexpr uint32_t kMaxRank = 128, kTop = 50, kGone = kMaxRank + 500;
  Segment a(20000, 0, kMaxRank), b(9000, 20000, kMaxRank);
  const Segment* segs[2] = {&a, &b};
  const BM25 scorer;
  const std::vector<SegmentStats> index{a.stats(), b.stats()};

  // a AND (b OR (c AND d)); (a AND NOT b) OR c; +a +(b c d)~2 with boosts at every level and a
  // negated subtree; a min-match over mixed children with a term in two branches and a term no
  // segment holds; an ordinary Or written as a tree of one level
  std::vector<BoolTree> trees{
      And::tree({L(0), Or::tree({L(9), And::tree({L(2), L(5)})})}),
      Or::tree({And::tree({L(1), BoolTree::negated(L(3))}), L(30)}),
      And::tree({L(0, 0.5f), Or::tree({L(1, 2.f), L(4), L(6, 0.25f)}, 2, 4.f),
                 BoolTree::negated(And::tree({L(2), BoolTree::negated(BoolTree::negated(L(7)))}))}, 0.5f),
      Or::tree({And::tree({L(1), L(3, 0.25f)}, 4.f), L(7, 2.f), Or::tree({L(1), L(kGone)}), And::tree({L(0), L(kGone)})}, 2, 0.5f),
      Or::tree({L(2), L(9), L(30)})};
  std::vector<filter> filters(trees.begin(), trees.end());
  const auto prepared = prepare(filters, scorer, index);
  // the first: entries a, NODE(OR, 4), b, NODE(AND, 2), c, d
  REQUIRE(prepared[0].op == IRS_HIP_OP_AND && prepared[0].terms.size() == 6);
  REQUIRE(prepared[0].terms[0].term == 0 && prepared[0].terms[0].kind == IRS_HIP_SCORE_BM25);
  REQUIRE(prepared[0].terms[1].kind == (IRS_HIP_TREE_NODE | IRS_HIP_OP_OR) && prepared[0].terms[1].phrase_offset == 4);
  REQUIRE(prepared[0].terms[3].kind == (IRS_HIP_TREE_NODE | IRS_HIP_OP_AND) && prepared[0].terms[3].phrase_offset == 2);
  REQUIRE(prepared[0].terms[1].term == IRS_HIP_NO_TERM && prepared[0].terms[5].term == 5);
  REQUIRE(prepared[1].op == IRS_HIP_OP_OR && prepared[1].terms[2].kind == IRS_HIP_EXCLUDE && prepared[1].terms[2].term == 3);
  REQUIRE(prepared[2].terms[1].kind == (IRS_HIP_TREE_NODE | IRS_HIP_OP_MINMATCH) &&
          prepared[2].terms[1].phrase_offset == (3u | (2u << 16)));
  REQUIRE(prepared[2].terms[5].kind == (IRS_HIP_TREE_NODE | IRS_HIP_OP_AND | IRS_HIP_EXCLUDE));
  REQUIRE(prepared[2].terms[7].kind == IRS_HIP_SCORE_BM25);   // Not(Not(f)) is f
  REQUIRE(prepared[3].op == IRS_HIP_OP_MINMATCH && prepared[3].min_match == 2 && prepared[3].merge == IRS_HIP_MERGE_SUM);
  REQUIRE(prepared[4].op == IRS_HIP_OP_OR && prepared[4].terms.size() == 3);
  for (const auto& e : prepared[4].terms) REQUIRE(!(e.kind & IRS_HIP_TREE_NODE));
  {  // the boost product, from the top down
    TermStats st;
    uint64_t dwt = 0, dwf = 0, ttf = 0;
    for (const auto& s : index) {
      dwt += s.docs_count(6);
      dwf += s.docs_with_field;
      ttf += s.total_term_freq;
    }
    scorer.collect(st, dwf, dwt, ttf);
    REQUIRE(prepared[2].terms[4].term == 6 && prepared[2].terms[4].c0 == scorer.term_scorer(st, (0.5f * 4.f) * 0.25f).c0);
  }
  QueryBatch batch({a.reader.get(), b.reader.get()}, prepared, kTop);
  REQUIRE(batch.tree_units() == 8 && batch.clause_units() == 0 && batch.wide_units() == 0);
  const auto res = batch.run().results();
  const auto top = merge(res);

  const orc_scorer osc{ORC_SCORER_BM25, scorer.k(), scorer.b(), 0};
  for (size_t q = 0; q < trees.size(); ++q) {
    std::vector<double> all;   // every matching doc's score, both segments
    for (uint32_t s = 0; s < 2; ++s) {
      Composer c{*segs[s], index, osc, size_t(segs[s]->num_docs) + 1};
      std::vector<uint8_t> m;
      std::vector<double> score;
      c.node(trees[q], 1.f, m, score);
      REQUIRE(!c.failed);
      uint64_t total = 0;
      for (size_t d = 0; d < c.n1; ++d)
        if (m[d]) {
          ++total;
          all.push_back(score[d]);
        }
      REQUIRE(res.total(s, uint32_t(q)) == total);
      REQUIRE(total > 0 && res.count(s, uint32_t(q)) == std::min<uint64_t>(kTop, total));
      for (uint32_t i = 0; i < res.count(s, uint32_t(q)); ++i) {
        const irs_hip_hit h = res.of(s, uint32_t(q))[i];
        REQUIRE(h.doc < c.n1 && m[h.doc] && close_rel(h.score, score[h.doc]));
        REQUIRE(i == 0 || res.of(s, uint32_t(q))[i - 1].score >= h.score);
      }
    }
    std::sort(all.begin(), all.end(), [](double x, double y) { return x > y; });
    if (all.size() > kTop) all.resize(kTop);
    REQUIRE(top[q].size() == all.size());
    for (size_t i = 0; i < all.size(); ++i) REQUIRE(close_rel(top[q][i].score, all[i]));
  }

  // what the layer and the ABI refuse
  {
    // one level with Nots: a flat And, the excluded entries behind the included ones, no tree unit
    const auto flat = prepare({filter{And::tree({L(2), BoolTree::negated(L(9)), L(30)})}}, scorer, index);
    REQUIRE(flat[0].op == IRS_HIP_OP_AND && flat[0].terms.size() == 3);
    REQUIRE(flat[0].terms[0].term == 2 && flat[0].terms[1].term == 30 && flat[0].terms[2].kind == IRS_HIP_EXCLUDE);
    QueryBatch fb({a.reader.get()}, flat, kTop);
    REQUIRE(fb.tree_units() == 0);
    const BoolTree ab = And::tree({L(1), L(2)});
    REQUIRE(throws<not_supported>([&] { prepare({filter{Or::tree({ab, BoolTree::negated(L(3))})}}, scorer, index); }));
    REQUIRE(throws<not_supported>([&] { prepare({filter{Or::tree({ab, And::tree({BoolTree::negated(L(3))})})}}, scorer, index); }));
    REQUIRE(throws<not_supported>([&] { prepare({filter{BoolTree::negated(Or::tree({ab, L(3)}))}}, scorer, index); }));
    REQUIRE(throws<not_supported>([&] { prepare({filter{Or::tree({ab, Or::tree({L(3), L(4)}, 0)})}}, scorer, index); }));
    REQUIRE(throws<illegal_argument>([&] { prepare({filter{Or::tree({ab, And::tree({})})}}, scorer, index); }));
    std::vector<BoolTree> many{ab};
    for (uint32_t t = 0; t < 14; ++t) many.push_back(L(20 + t));
    REQUIRE(prepare({filter{Or::tree(many)}}, scorer, index)[0].terms.size() == 17);   // 16 leaves, one node
    many.push_back(L(40));
    REQUIRE(throws<not_supported>([&] { prepare({filter{Or::tree(many)}}, scorer, index); }));   // 17 leaves
    // MAX merge and a stray span written into the prepared query: refused by batch create
    auto one = prepare({filter{trees[0]}}, scorer, index);
    one[0].merge = IRS_HIP_MERGE_MAX;
    REQUIRE(throws<not_supported>([&] { QueryBatch({a.reader.get()}, one, kTop); }));
    one[0].merge = IRS_HIP_MERGE_SUM;
    one[0].terms[3].phrase_offset = 3;   // a span past its parent
    REQUIRE(throws<illegal_argument>([&] { QueryBatch({a.reader.get()}, one, kTop); }));
    one[0].terms[3].phrase_offset = 2;
    one[0].terms[2].kind = IRS_HIP_EXCLUDE;   // a Not under an Or node
    REQUIRE(throws<illegal_argument>([&] { QueryBatch({a.reader.get()}, one, kTop); }));
    // match sets of a batch with such a query
    QueryBatch mb({a.reader.get()}, prepare({filter{trees[0]}}, scorer, index), kTop);
    REQUIRE(throws<not_supported>([&] { mb.match_sets((uint64_t(a.num_docs) + 64) / 64); }));
  }
  std::printf("test_boolean_trees OK\n");
  return 0;
}
