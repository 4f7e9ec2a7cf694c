// tests/cpp/test_nested.cpp — TEST: QueryBatch::nested_sets / nested_topk of the C++ host layer
// (irs_hip_batch_nested_sets / _topk: ByNestedFilter, nested_filter.cpp) on one segment, under
// kMatchNone, kMatchAny and a Match{min, max}: against the oracle's C API — orc_score_all over ALL docs
// for the child filter — and a plain loop over the parents.  Linked against libirs_hip.so on a GPU box,
// or against the CPU emulator build of the same sources.
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

int main() {
  constexpr uint32_t kDocs = 15000, kMaxRank = 64, kTop = 20, kStep = 6;
  irs_synth_params p{};
  p.seed = 20260926;
  p.num_docs = kDocs;
  p.vocab_log2 = 20;
  p.max_rank = kMaxRank;
  p.layout = IRS_SYNTH_LAYOUT_SIMD4;
  p.mean_len = 100;
  p.stddev_len = 30;
  irs_synth_index* idx = nullptr;
  REQUIRE(irs_synth_build(&p, &idx) == 0);
  uint64_t doc_len = 0, norm_count = 0;
  uint32_t num_terms = 0;
  const uint8_t* doc = irs_synth_doc_bytes(idx, &doc_len);
  const uint8_t* norms = irs_synth_norms(idx, &norm_count);
  static_assert(sizeof(irs_synth_term_meta) == sizeof(irs_hip_term_meta), "same layout");
  static_assert(sizeof(orc_term_meta) == sizeof(irs_hip_term_meta), "same layout");
  const auto* metas = reinterpret_cast<const irs_hip_term_meta*>(irs_synth_term_metas(idx, &num_terms));
  irs_hip_segment_desc d{};
  d.layout = IRS_HIP_LAYOUT_SIMD4;
  d.doc_file = doc;
  d.doc_file_len = doc_len;
  d.num_docs = kDocs;
  d.has_freq = 1;
  d.norms = norms;
  d.norm_width = 1;
  d.norm_min_doc = 1;
  d.norm_count = norm_count;
  d.terms = metas;
  d.num_terms = num_terms;
  {
    SegmentReader reader(d);
    const SegmentStats st{irs_synth_docs_with_field(idx), irs_synth_total_term_freq(idx), metas, num_terms};
    const std::vector<SegmentStats> index{st};
    const BM25 scorer;
    const std::vector<uint32_t> terms{30, 38};
    const std::vector<float> boosts{1.f, 2.f};
    QueryBatch batch({&reader}, prepare({filter{Or{{by_term{30, 1.f}, by_term{38, 2.f}}}}}, scorer, index), kTop);

    // the child filter over all docs, from the oracle
    orc_segment view{};
    view.doc_file = doc;
    view.doc_file_len = doc_len;
    view.layout = ORC_LAYOUT_SIMD4;
    view.num_docs = kDocs;
    view.norms = norms;
    view.norm_width = 1;
    const orc_scorer osc{ORC_SCORER_BM25, scorer.k(), scorer.b(), 0};
    std::vector<orc_term_meta> om(terms.size());
    std::vector<uint64_t> dwt(terms.size());
    for (size_t i = 0; i < terms.size(); ++i) {
      std::memcpy(&om[i], &metas[terms[i]], sizeof om[i]);
      dwt[i] = st.docs_count(terms[i]);
    }
    const size_t n1 = size_t(kDocs) + 1;
    std::vector<float> cs(n1);
    std::vector<uint8_t> cm(n1);
    REQUIRE(orc_score_all(&view, om.data(), uint32_t(om.size()), ORC_OP_OR, &osc, boosts.data(), st.docs_with_field,
                          dwt.data(), st.total_term_freq, cs.data(), cm.data()) >= 0);

    // every kStep-th doc a parent
    const uint64_t n_words = kDocs / 64 + 1;
    std::vector<uint64_t> parents(n_words, 0);
    for (uint32_t x = kStep; x <= kDocs; x += kStep) parents[x / 64] |= uint64_t(1) << (x % 64);
    DeviceBuffer d_parents(0, n_words * 8);
    REQUIRE(irs_hip_device_upload(0, d_parents.get(), parents.data(), n_words * 8) == IRS_HIP_OK);

    const Match forms[3] = {kMatchNone, kMatchAny, Match{2, 3}};
    uint64_t seen = 0;
    for (const Match& m : forms) {
      Nested opts;
      opts.match = m;
      opts.none_boost = 1.5f;
      const bool none = m.min == 0 && m.max == 0;
      // the restatement: a loop over the parents, a float64 sum of the oracle's child scores
      std::vector<uint8_t> hit(n1, 0);
      std::vector<double> score(n1, 0.0);
      uint64_t n_hit = 0;
      uint32_t prev = 0, c_max = 0;
      for (uint32_t x = kStep; x <= kDocs; x += kStep) {
        uint32_t c = 0;
        double sum = 0;
        for (uint32_t k = prev + 1; k < x; ++k)
          if (cm[k]) {
            ++c;
            sum += cs[k];
          }
        prev = x;
        if (c < m.min || c > m.max) continue;
        hit[x] = 1;
        score[x] = none ? 1.5 : sum;
        c_max = std::max(c_max, c);
        ++n_hit;
      }
      REQUIRE(n_hit > kTop);
      const double tol = 1e-5 + (c_max > 1 && !none ? (c_max - 1) * std::ldexp(1.0, -24) : 0.0);
      const QueryBatch::MatchSets sets = batch.nested_sets(d_parents.get(), n_words, opts);
      REQUIRE(sets.count(0, 0) == n_hit);
      for (uint32_t x = 0; x <= kDocs; ++x) REQUIRE(sets.contains(0, 0, x) == (hit[x] != 0));
      const QueryBatch::MatchSets only = batch.nested_sets(d_parents.get(), n_words, opts, false);
      REQUIRE(only.count(0, 0) == n_hit && only.words.empty());
      const QueryBatch::Results top = batch.nested_topk(d_parents.get(), n_words, opts);
      REQUIRE(top.total(0, 0) == n_hit && top.count(0, 0) == kTop);
      std::vector<double> all;
      for (uint32_t x = 0; x <= kDocs; ++x)
        if (hit[x]) all.push_back(score[x]);
      std::sort(all.begin(), all.end(), [](double a, double b) { return a > b; });
      const double thr = all[kTop - 1];
      const irs_hip_hit* h = top.of(0, 0);
      for (uint32_t i = 0; i < kTop; ++i) {
        REQUIRE(h[i].doc <= kDocs && hit[h[i].doc]);
        REQUIRE(std::fabs(h[i].score - score[h[i].doc]) <= tol * score[h[i].doc]);
        REQUIRE(score[h[i].doc] >= thr * (1 - 2 * tol));
        if (i) REQUIRE(h[i - 1].score > h[i].score || (h[i - 1].score == h[i].score && h[i - 1].doc < h[i].doc));
      }
      seen += n_hit;
    }
    // what the layer hands on: a rule with min > max
    bool refused = false;
    try {
      Nested bad;
      bad.match = Match{3, 2};
      batch.nested_sets(d_parents.get(), n_words, bad);
    } catch (const illegal_argument&) {
      refused = true;
    }
    REQUIRE(refused);
    batch.run();
    std::printf("test_nested OK: %llu hits\n", (unsigned long long)seen);
  }
  irs_synth_free(idx);
  return 0;
}
