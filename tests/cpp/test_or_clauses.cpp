// tests/cpp/test_or_clauses.cpp — TEST: the C++ host layer's Or with And children (Or::clauses, a
// disjunction of clauses, IRS_HIP_CLAUSE_AND) against the oracle's C API, composed per clause: a
// clause is the oracle's And over its entries (its Or for a clause of one), emptied here where the
// segment lacks an entry; a doc matches when enough clauses do, its score is their sum.  And what
// the layer refuses.  Linked against libirs_hip.so on a GPU box, or against the CPU emulator build
// of the same sources.
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

// The clauses of an Or as the layer orders them (subs, then clauses), each member (term, boost
// product from the top) — written out here, apart from prepare()
std::vector<std::vector<by_term>> clauses_of(const Or& o) {
  std::vector<std::vector<by_term>> out;
  for (const by_term& t : o.subs) out.push_back({by_term{t.term, o.boost * t.boost}});
  for (const And& c : o.clauses) {
    out.emplace_back();
    for (const by_term& t : c.subs) out.back().push_back(by_term{t.term, (o.boost * c.boost) * t.boost});
  }
  return out;
}

}  // namespace

int main() {
  constexpr uint32_t kMaxRank = 128, kTop = 50, kGone = kMaxRank + 500;
  Segment a(20000, 0, kMaxRank), b(9000, 20000, kMaxRank);
  const Segment* segs[2] = {&a, &b};
  const BM25 scorer;
  const std::vector<SegmentStats> index{a.stats(), b.stats()};

  // (a AND b) OR c; a min_match 2 form with boosts at all three levels, a term in two clauses and a
  // clause with a term no segment holds; one clause alone; an ordinary Or
  Or abc;
  abc.subs = {by_term{9}};
  abc.clauses = {And{{by_term{2}, by_term{5}}}};
  Or two;
  two.min_match_count = 2;
  two.boost = 0.5f;
  two.subs = {by_term{7, 2.f}, by_term{30}};
  And c1{{by_term{1}, by_term{3, 0.25f}}};
  c1.boost = 4.f;
  And c2{{by_term{1, 2.f}, by_term{4}, by_term{6}}};
  And c3{{by_term{0}, by_term{kGone}}};
  two.clauses = {c1, c2, c3};
  Or alone;
  alone.clauses = {And{{by_term{3}, by_term{8}, by_term{11}}}};
  std::vector<Or> ors{abc, two, alone, Or{{by_term{2}, by_term{9}, by_term{30}}}};
  std::vector<filter> filters(ors.begin(), ors.end());
  const auto prepared = prepare(filters, scorer, index);
  REQUIRE(prepared[0].op == IRS_HIP_OP_OR && prepared[0].terms.size() == 3);
  REQUIRE(prepared[0].terms[0].term == 9 && !(prepared[0].terms[0].kind & IRS_HIP_CLAUSE_AND));
  REQUIRE(prepared[0].terms[1].term == 2 && !(prepared[0].terms[1].kind & IRS_HIP_CLAUSE_AND));
  REQUIRE(prepared[0].terms[2].term == 5 && (prepared[0].terms[2].kind & IRS_HIP_CLAUSE_AND));
  REQUIRE(prepared[1].op == IRS_HIP_OP_MINMATCH && prepared[1].min_match == 2 && prepared[1].terms.size() == 9);
  REQUIRE(prepared[1].merge == IRS_HIP_MERGE_SUM);
  for (const auto& e : prepared[3].terms) REQUIRE(!(e.kind & IRS_HIP_CLAUSE_AND));
  QueryBatch batch({a.reader.get(), b.reader.get()}, prepared, kTop);
  REQUIRE(batch.clause_units() == 6 && batch.wide_units() == 0);
  const auto res = batch.run().results();
  const auto top = merge(res);

  const orc_segment views[2] = {a.oracle_view(), b.oracle_view()};
  const uint64_t dwf[2] = {a.stats().docs_with_field, b.stats().docs_with_field};
  const uint64_t ttf[2] = {a.stats().total_term_freq, b.stats().total_term_freq};
  const orc_scorer osc{ORC_SCORER_BM25, scorer.k(), scorer.b(), 0};
  for (size_t q = 0; q < 3; ++q) {
    const auto clauses = clauses_of(ors[q]);
    const uint32_t need = std::max<uint32_t>(1, ors[q].min_match_count);
    std::vector<double> all;   // every matching doc's score, both segments
    for (uint32_t s = 0; s < 2; ++s) {
      const size_t n1 = size_t(segs[s]->num_docs) + 1;
      std::vector<double> score(n1, 0.0);
      std::vector<uint32_t> count(n1, 0);
      for (const auto& cl : clauses) {
        const uint32_t n = uint32_t(cl.size());
        std::vector<orc_term_meta> metas(n);
        std::vector<uint64_t> dwt(n, 0);
        std::vector<float> boosts(n);
        bool present = true;
        for (uint32_t t = 0; t < n; ++t) {
          present = present && cl[t].term < segs[s]->num_terms && segs[s]->metas[cl[t].term].docs_count;
          if (cl[t].term < segs[s]->num_terms)
            std::memcpy(&metas[t], &segs[s]->metas[cl[t].term], sizeof(orc_term_meta));
          for (uint32_t o = 0; o < 2; ++o) dwt[t] += index[o].docs_count(cl[t].term);
          boosts[t] = cl[t].boost;
        }
        if (!present) continue;   // an absent entry: the clause is empty in this segment
        std::vector<float> sc(n1);
        std::vector<uint8_t> m(n1);
        REQUIRE(orc_score_all(&views[s], metas.data(), n, n > 1 ? ORC_OP_AND : ORC_OP_OR, &osc, boosts.data(),
                              dwf[0] + dwf[1], dwt.data(), ttf[0] + ttf[1], sc.data(), m.data()) >= 0);
        for (size_t d = 0; d < n1; ++d)
          if (m[d]) {
            ++count[d];
            score[d] += sc[d];
          }
      }
      uint64_t total = 0;
      for (size_t d = 0; d < n1; ++d)
        if (count[d] >= need) {
          ++total;
          all.push_back(score[d]);
        }
      REQUIRE(res.total(s, uint32_t(q)) == total);
      REQUIRE(total > 0 && res.count(s, uint32_t(q)) == std::min<uint64_t>(kTop, total));
      for (uint32_t i = 0; i < res.count(s, uint32_t(q)); ++i) {
        const irs_hip_hit h = res.of(s, uint32_t(q))[i];
        REQUIRE(h.doc < n1 && count[h.doc] >= need && close_rel(h.score, score[h.doc]));
        REQUIRE(i == 0 || res.of(s, uint32_t(q))[i - 1].score >= h.score);
      }
    }
    std::sort(all.begin(), all.end(), [](double x, double y) { return x > y; });
    if (all.size() > kTop) all.resize(kTop);
    REQUIRE(top[q].size() == all.size());
    for (size_t i = 0; i < all.size(); ++i) REQUIRE(close_rel(top[q][i].score, all[i]));
  }
  // one clause alone is the oracle's And of its entries, searched over both segments
  {
    const PreparedQuery& p = prepared[2];
    const uint32_t n = uint32_t(p.terms.size());
    std::vector<orc_term_meta> metas(2 * n);
    for (uint32_t s = 0; s < 2; ++s)
      for (uint32_t t = 0; t < n; ++t)
        std::memcpy(&metas[s * n + t], &segs[s]->metas[p.terms[t].term], sizeof(orc_term_meta));
    std::vector<orc_hit> want(kTop);
    uint64_t want_total = 0;
    const int64_t got_n = orc_search(views, 2, metas.data(), n, ORC_OP_AND, &osc, nullptr, dwf, ttf, kTop,
                                     want.data(), &want_total);
    REQUIRE(got_n >= 0);
    want.resize(size_t(got_n));
    REQUIRE(res.total(0, 2) + res.total(1, 2) == want_total && want_total > 0);
    REQUIRE(top[2].size() == want.size());
    std::sort(want.begin(), want.end(), [](const orc_hit& x, const orc_hit& y) { return x.score > y.score; });
    for (size_t i = 0; i < want.size(); ++i) REQUIRE(close_rel(top[2][i].score, want[i].score));
  }

  // what the layer and the ABI refuse
  {
    // clauses of one member each: a flat Or, no clause unit
    Or singles;
    singles.subs = {by_term{2}};
    singles.clauses = {And{{by_term{9}}}, And{{by_term{30}}}};
    const auto flat = prepare({filter{singles}}, scorer, index);
    for (const auto& e : flat[0].terms) REQUIRE(!(e.kind & IRS_HIP_CLAUSE_AND));
    QueryBatch fb({a.reader.get()}, flat, kTop);
    REQUIRE(fb.clause_units() == 0);
    Or bad = abc;
    bad.phrases.push_back(by_phrase{}.push_back(1).push_back(2));
    REQUIRE(throws<not_supported>([&] { prepare({filter{bad}}, scorer, index); }));
    bad = abc;
    bad.clauses[0].groups.push_back(Or{{by_term{1}, by_term{2}}});
    REQUIRE(throws<not_supported>([&] { prepare({filter{bad}}, scorer, index); }));
    bad = abc;
    bad.clauses[0].phrases.push_back(by_phrase{}.push_back(1).push_back(2));
    REQUIRE(throws<not_supported>([&] { prepare({filter{bad}}, scorer, index); }));
    bad = abc;
    bad.clauses[0].merge_type = IRS_HIP_MERGE_MAX;
    REQUIRE(throws<not_supported>([&] { prepare({filter{bad}}, scorer, index); }));
    bad = abc;
    bad.merge_type = IRS_HIP_MERGE_MIN;
    REQUIRE(throws<not_supported>([&] { prepare({filter{bad}}, scorer, index); }));
    bad = abc;
    bad.clauses.push_back(And{});
    REQUIRE(throws<illegal_argument>([&] { prepare({filter{bad}}, scorer, index); }));
    bad = abc;
    for (uint32_t t = 0; t < 14; ++t) bad.subs.push_back(by_term{20 + t});
    REQUIRE(throws<not_supported>([&] { prepare({filter{bad}}, scorer, index); }));   // 17 terms
    bad.subs.pop_back();
    REQUIRE(prepare({filter{bad}}, scorer, index)[0].terms.size() == 16);
    // Not children and doc sets around it
    Exclusion ex{abc, {by_term{4}}, std::nullopt};
    REQUIRE(throws<not_supported>([&] { prepare({filter{ex}}, scorer, index); }));
    Exclusion ds{abc, {}, by_doc_set{0}};
    REQUIRE(throws<not_supported>([&] { prepare({filter{ds}}, scorer, index); }));
    // MAX merge and an excluded entry written into the prepared query: refused by batch create
    auto one = prepare({filter{abc}}, scorer, index);
    one[0].merge = IRS_HIP_MERGE_MAX;
    REQUIRE(throws<not_supported>([&] { QueryBatch({a.reader.get()}, one, kTop); }));
    one[0].merge = IRS_HIP_MERGE_SUM;
    irs_hip_term_scorer e{};
    e.term = 3;
    e.kind = IRS_HIP_EXCLUDE;
    one[0].terms.push_back(e);
    REQUIRE(throws<not_supported>([&] { QueryBatch({a.reader.get()}, one, kTop); }));
    one[0].terms.pop_back();
    one[0].terms[0].kind |= IRS_HIP_CLAUSE_AND;   // the flag on the first entry
    REQUIRE(throws<illegal_argument>([&] { QueryBatch({a.reader.get()}, one, kTop); }));
    // match sets of a batch with such a query
    QueryBatch mb({a.reader.get()}, prepare({filter{abc}}, scorer, index), kTop);
    REQUIRE(throws<not_supported>([&] { mb.match_sets((uint64_t(a.num_docs) + 64) / 64); }));
  }
  std::printf("test_or_clauses OK\n");
  return 0;
}
