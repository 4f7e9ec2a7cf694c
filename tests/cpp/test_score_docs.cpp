// tests/cpp/test_score_docs.cpp — TEST: QueryBatch::score_docs of the C++ host layer
// (irs_hip_batch_score_docs: doc_iterator::seek + score for docs the caller names) against the
// oracle's C API — orc_score_all over ALL docs of a segment with index-global statistics — for flat
// Or / And / min-match queries over two segments, against the batch's own run for a nested tree, and
// what the layer refuses.  Linked against libirs_hip.so on a GPU box, or against the CPU emulator
// build of the same sources.
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

  Segment(uint32_t docs, uint64_t first_doc, uint32_t max_rank, bool positions = false) : num_docs{docs} {
    irs_synth_params p{};
    p.seed = 20260926;
    p.first_doc = first_doc;
    p.num_docs = docs;
    p.vocab_log2 = 20;
    p.max_rank = max_rank;
    p.layout = IRS_SYNTH_LAYOUT_SIMD4;
    p.mean_len = 100;
    p.stddev_len = 30;
    p.with_positions = positions ? 1 : 0;
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
    if (positions) {
      uint64_t pos_len = 0;
      d.pos_file = irs_synth_pos_bytes(idx, &pos_len);
      d.pos_file_len = pos_len;
    }
    reader = std::make_unique<SegmentReader>(d);
  }
  ~Segment() {
    reader.reset();
    irs_synth_free(idx);
  }
  SegmentStats stats() const {
    return SegmentStats{irs_synth_docs_with_field(idx), irs_synth_total_term_freq(idx), metas, num_terms};
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

struct Flat {   // one flat query as both sides see it
  filter flt;
  std::vector<uint32_t> terms;
  std::vector<float> boosts;
  int32_t op;
};

}  // namespace

int main() {
  constexpr uint32_t kMaxRank = 128, kTop = 50, kGone = kMaxRank + 500;
  Segment a(20000, 0, kMaxRank), b(9000, 20000, kMaxRank);
  const Segment* segs[2] = {&a, &b};
  const BM25 scorer;
  const std::vector<SegmentStats> index{a.stats(), b.stats()};
  const orc_scorer osc{ORC_SCORER_BM25, scorer.k(), scorer.b(), 0};

  And a3;
  a3.subs = {by_term{0, 1.f}, by_term{2, 0.5f}, by_term{30, 1.f}};
  And gone;
  gone.subs = {by_term{1, 1.f}, by_term{kGone, 1.f}};
  const std::vector<Flat> flat{
      {by_term{5, 2.f}, {5}, {2.f}, ORC_OP_OR},
      {Or{{by_term{1, 1.f}, by_term{40, 1.f}, by_term{90, 2.f}}}, {1, 40, 90}, {1.f, 1.f, 2.f}, ORC_OP_OR},
      {Or{{by_term{0, 1.f}, by_term{1, 1.f}, by_term{2, 1.f}, by_term{3, 1.f}}, 3}, {0, 1, 2, 3}, {1.f, 1.f, 1.f, 1.f},
       ORC_OP_MINMATCH | (3 << 8)},
      {a3, {0, 2, 30}, {1.f, 0.5f, 1.f}, ORC_OP_AND},
      {Or{{by_term{7, 1.f}, by_term{kGone, 1.f}}}, {7, kGone}, {1.f, 1.f}, ORC_OP_OR},   // an absent term: dropped
      {gone, {1, kGone}, {1.f, 1.f}, ORC_OP_AND}};                                       // ... empties the And
  std::vector<filter> filters;
  for (const Flat& f : flat) filters.push_back(f.flt);
  const BoolTree tree = And::tree({BoolTree::leaf(0), Or::tree({BoolTree::leaf(9), And::tree({BoolTree::leaf(2), BoolTree::leaf(5)})})});
  filters.push_back(filter{tree});
  const uint32_t nq = uint32_t(filters.size()), q_tree = nq - 1;
  QueryBatch batch({a.reader.get(), b.reader.get()}, prepare(filters, scorer, index), kTop);
  REQUIRE(batch.tree_units() == 2);

  // per unit: every 7th doc, 1 and the segment's last doc — 2858 / 1287 docs: many chunks, the last one partial
  std::vector<std::vector<uint32_t>> docs(size_t(2) * nq);
  for (uint32_t s = 0; s < 2; ++s)
    for (uint32_t q = 0; q < nq; ++q) {
      std::vector<uint32_t>& d = docs[size_t(s) * nq + q];
      for (uint32_t x = 1 + q; x <= segs[s]->num_docs; x += 7) d.push_back(x);
      if (d.back() != segs[s]->num_docs) d.push_back(segs[s]->num_docs);
    }
  docs[2].clear();   // an empty list
  const QueryBatch::ScoredDocs before = batch.score_docs(docs);   // (before any run)
  const auto res = batch.run().results();
  const QueryBatch::ScoredDocs got = batch.score_docs(docs);
  REQUIRE(before.offsets == got.offsets && before.scores == got.scores && before.matched == got.matched);
  REQUIRE(got.offsets.size() == size_t(2) * nq + 1 && got.offsets[0] == 0 && got.offsets[2] == got.offsets[3]);
  REQUIRE(got.scores.size() == got.offsets.back() && got.matched.size() == got.offsets.back());

  uint64_t n_matched = 0;
  for (uint32_t s = 0; s < 2; ++s) {
    const Segment& seg = *segs[s];
    const size_t n1 = size_t(seg.num_docs) + 1;
    const orc_segment view = seg.oracle_view();
    for (uint32_t q = 0; q < flat.size(); ++q) {
      const Flat& f = flat[q];
      std::vector<orc_term_meta> metas(f.terms.size());
      std::vector<uint64_t> dwt(f.terms.size(), 0);
      uint64_t dwf = 0, ttf = 0;
      for (const auto& st : index) {
        dwf += st.docs_with_field;
        ttf += st.total_term_freq;
      }
      for (size_t i = 0; i < f.terms.size(); ++i) {
        std::memset(&metas[i], 0, sizeof metas[i]);
        if (f.terms[i] < seg.num_terms) std::memcpy(&metas[i], &seg.metas[f.terms[i]], sizeof metas[i]);
        for (const auto& st : index) dwt[i] += st.docs_count(f.terms[i]);
      }
      std::vector<float> want(n1);
      std::vector<uint8_t> wm(n1);
      REQUIRE(orc_score_all(&view, metas.data(), uint32_t(metas.size()), f.op, &osc, f.boosts.data(), dwf, dwt.data(),
                            ttf, want.data(), wm.data()) >= 0);
      const size_t u = size_t(s) * nq + q;
      for (uint64_t i = got.offsets[u]; i < got.offsets[u + 1]; ++i) {
        const uint32_t d = docs[u][i - got.offsets[u]];
        REQUIRE((got.matched[i] != 0) == (wm[d] != 0));
        if (wm[d]) REQUIRE(close_rel(got.scores[i], want[d]));
        else REQUIRE(got.scores[i] == 0.f);
        n_matched += wm[d] != 0;
      }
      if (q == 5) for (uint64_t i = got.offsets[u]; i < got.offsets[u + 1]; ++i) REQUIRE(!got.matched[i]);
    }
    // the tree: its run's hits, asked for by doc, match with the run's scores
    std::vector<std::vector<uint32_t>> own(size_t(2) * nq);
    std::vector<irs_hip_hit> hits(res.of(s, q_tree), res.of(s, q_tree) + res.count(s, q_tree));
    REQUIRE(hits.size() == kTop);
    std::sort(hits.begin(), hits.end(), [](const irs_hip_hit& x, const irs_hip_hit& y) { return x.doc < y.doc; });
    for (const irs_hip_hit& h : hits) own[size_t(s) * nq + q_tree].push_back(h.doc);
    const QueryBatch::ScoredDocs t = batch.score_docs(own);
    REQUIRE(t.scores.size() == kTop);
    for (uint32_t i = 0; i < kTop; ++i) REQUIRE(t.matched[i] && std::fabs(t.scores[i] - hits[i].score) <= 2e-5 * hits[i].score);
  }
  REQUIRE(n_matched > 1000);

  // what the layer refuses
  REQUIRE(throws<illegal_argument>([&] { batch.score_docs({{1, 2}}); }));               // one list per unit
  std::vector<std::vector<uint32_t>> bad(size_t(2) * nq);
  bad[0] = {3, 3};
  REQUIRE(throws<illegal_argument>([&] { batch.score_docs(bad); }));                    // not strictly ascending
  bad[0] = {0};
  REQUIRE(throws<illegal_argument>([&] { batch.score_docs(bad); }));
  bad[0] = {a.num_docs + 1};
  REQUIRE(throws<illegal_argument>([&] { batch.score_docs(bad); }));
  bad[0] = {a.num_docs};
  bad[nq] = {b.num_docs + 1};                                                           // the second segment's own bound
  REQUIRE(throws<illegal_argument>([&] { batch.score_docs(bad); }));
  {
    Segment p(3000, 0, 48, true);
    by_phrase ph;
    ph.push_back(0).push_back(1);
    const std::vector<SegmentStats> pi{p.stats()};
    QueryBatch pb({p.reader.get()}, prepare({filter{ph}, filter{by_term{1, 1.f}}}, scorer, pi), 10);
    REQUIRE(throws<not_supported>([&] { pb.score_docs({{1, 2}, {1, 2}}); }));
    REQUIRE(throws<not_supported>([&] { pb.score_docs_to_device(nullptr, nullptr, 0, nullptr, nullptr); }));
    pb.run();
  }
  // the results of the batch are what they were
  const auto again = batch.run().results();
  for (uint32_t s = 0; s < 2; ++s)
    for (uint32_t q = 0; q < nq; ++q) {
      REQUIRE(again.count(s, q) == res.count(s, q) && again.total(s, q) == res.total(s, q));
      REQUIRE(std::memcmp(again.of(s, q), res.of(s, q), sizeof(irs_hip_hit) * res.count(s, q)) == 0);
    }
  std::printf("test_score_docs OK: %llu matched\n", (unsigned long long)n_matched);
  return 0;
}
