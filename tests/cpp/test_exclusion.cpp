// tests/cpp/test_exclusion.cpp — TEST: the C++ host layer's Exclusion filter (irs::And of one
// included filter and Not(by_term) children) through prepare() and QueryBatch.  What it must
// give: the included filter's results on the same segment opened with every doc of the excluded
// terms deleted (irs_hip_segment_desc::doc_mask) — same totals, same docs, same scores.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "irs_hip.hpp"
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
  irs_synth_params p{};
  p.seed = 20261015;
  p.num_docs = 40000;
  p.vocab_log2 = 20;
  p.max_rank = 128;
  p.layout = IRS_SYNTH_LAYOUT_SIMD4;
  p.mean_len = 100;
  p.stddev_len = 30;
  p.with_positions = 1;
  irs_synth_index* idx = nullptr;
  REQUIRE(irs_synth_build(&p, &idx) == 0);
  int rc = 0;
  {
    uint64_t doc_len = 0, pos_len = 0, norm_count = 0;
    uint32_t num_terms = 0;
    irs_hip_segment_desc d{};
    d.layout = IRS_HIP_LAYOUT_SIMD4;
    d.doc_file = irs_synth_doc_bytes(idx, &doc_len);
    d.doc_file_len = doc_len;
    d.num_docs = p.num_docs;
    d.has_freq = 1;
    d.norms = irs_synth_norms(idx, &norm_count);
    d.norm_width = 1;
    d.norm_min_doc = 1;
    d.norm_count = norm_count;
    d.terms = reinterpret_cast<const irs_hip_term_meta*>(irs_synth_term_metas(idx, &num_terms));
    d.num_terms = num_terms;
    d.pos_file = irs_synth_pos_bytes(idx, &pos_len);
    d.pos_file_len = pos_len;
    SegmentReader seg(d);
    const std::vector<SegmentStats> index{
        SegmentStats{irs_synth_docs_with_field(idx), irs_synth_total_term_freq(idx), d.terms, num_terms}};

    const uint32_t ex1 = 9, ex2 = 40, ex3 = 2;
    std::vector<uint32_t> gone, docs;
    for (uint32_t t : {ex1, ex2, ex3}) {
      seg.postings(t, docs, nullptr, d.terms[t].docs_count);
      gone.insert(gone.end(), docs.begin(), docs.end());
    }
    std::sort(gone.begin(), gone.end());
    irs_hip_segment_desc dm = d;   // the same segment with the excluded terms' docs deleted
    dm.doc_mask = gone.data();
    dm.doc_mask_count = gone.size();
    SegmentReader masked(dm);

    Or o;
    for (uint32_t t : {1u, 5u, 12u, 33u, 70u}) o.subs.push_back(by_term{t, 1.f});
    Or mm = o;
    mm.min_match_count = 2;
    And a;
    a.subs = {by_term{0, 1.f}, by_term{3, 1.f}};
    by_phrase ph;
    ph.push_back(0).push_back(1);
    const std::vector<filter> excl{
        Exclusion{o, {by_term{ex1, 1.f}, by_term{ex2, 1.f}, by_term{ex3, 1.f}}},
        Exclusion{mm, {by_term{ex1, 1.f}, by_term{ex2, 1.f}, by_term{ex3, 1.f}}},
        Exclusion{a, {by_term{ex3, 1.f}, by_term{ex1, 1.f}, by_term{ex2, 1.f}, by_term{100000, 1.f}}},
        Exclusion{ph, {by_term{ex1, 1.f}, by_term{ex2, 1.f}, by_term{ex3, 1.f}}},
        Exclusion{by_term{ex1, 1.f}, {by_term{ex1, 1.f}}},   // empty
    };
    const std::vector<filter> plain{o, mm, a, ph, by_term{ex1, 1.f}};
    const auto prepared = prepare(excl, BM25{}, index);
    REQUIRE(prepared[0].terms.size() == 8 && prepared[0].terms[5].kind == IRS_HIP_EXCLUDE);
    const uint32_t k = 50;
    QueryBatch b1({&seg}, prepared, k);
    QueryBatch b2({&masked}, prepare(plain, BM25{}, index), k);
    const QueryBatch::Results r1 = b1.run().results(), r2 = b2.run().results();
    for (uint32_t q = 0; q + 1 < plain.size(); ++q) {
      REQUIRE(r1.total(0, q) == r2.total(0, q) && r1.total(0, q) > 0);
      REQUIRE(r1.count(0, q) == r2.count(0, q));
      const uint32_t n = r1.count(0, q);
      const float kth = r2.of(0, q)[n - 1].score;
      std::vector<uint32_t> d1, d2;   // the docs clear of the k-th score: the same on both sides
      for (uint32_t i = 0; i < n; ++i) {
        const irs_hip_hit x = r1.of(0, q)[i], y = r2.of(0, q)[i];
        REQUIRE(std::fabs(x.score - y.score) <= 1e-5f * std::fabs(y.score));
        REQUIRE(!std::binary_search(gone.begin(), gone.end(), x.doc));
        if (x.score > kth * (1.f + 1e-4f)) d1.push_back(x.doc);
        if (y.score > kth * (1.f + 1e-4f)) d2.push_back(y.doc);
      }
      std::sort(d1.begin(), d1.end());
      std::sort(d2.begin(), d2.end());
      REQUIRE(d1 == d2);
    }
    REQUIRE(r1.total(0, 4) == 0 && r1.count(0, 4) == 0 && r2.total(0, 4) == 0);
    std::printf("test_exclusion OK: totals %llu %llu %llu %llu\n", (unsigned long long)r1.total(0, 0),
                (unsigned long long)r1.total(0, 1), (unsigned long long)r1.total(0, 2),
                (unsigned long long)r1.total(0, 3));
  }
  irs_synth_free(idx);
  return rc;
}
