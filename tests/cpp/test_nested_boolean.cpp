// tests/cpp/test_nested_boolean.cpp — TEST: the C++ host layer's And of Or groups (And::groups,
// IRS_HIP_GROUP_ALT) through prepare() and QueryBatch: the normalisation (a one-term group is a
// term, a tree without a group of two is the flat And entry for entry), the refusals, the boost
// product term x Or x And (boolean_query_boost.hierarchy), the match sets a AND (b OR c) against
// the decoded postings, and Exclusion{And{...groups...}, ...} against the same And on the segment
// opened with the excluded terms' docs deleted.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iterator>
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

static bool same_entries(const PreparedQuery& x, const PreparedQuery& y) {
  if (x.op != y.op || x.merge != y.merge || x.min_match != y.min_match || x.terms.size() != y.terms.size())
    return false;
  for (size_t i = 0; i < x.terms.size(); ++i)
    if (std::memcmp(&x.terms[i], &y.terms[i], sizeof(irs_hip_term_scorer)) != 0) return false;
  return true;
}

int main() {
  irs_synth_params p{};
  p.seed = 20261016;
  p.num_docs = 40000;
  p.vocab_log2 = 20;
  p.max_rank = 128;
  p.layout = IRS_SYNTH_LAYOUT_SIMD4;
  p.mean_len = 100;
  p.stddev_len = 30;
  irs_synth_index* idx = nullptr;
  REQUIRE(irs_synth_build(&p, &idx) == 0);
  int rc = 0;
  {
    uint64_t doc_len = 0, norm_count = 0;
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
    SegmentReader seg(d);
    const std::vector<SegmentStats> index{
        SegmentStats{irs_synth_docs_with_field(idx), irs_synth_total_term_freq(idx), d.terms, num_terms}};
    const uint64_t dwf = irs_synth_docs_with_field(idx), ttf = irs_synth_total_term_freq(idx);

    // normalisation: one-term groups are terms, the query is the flat And entry for entry
    And flat;
    flat.subs = {by_term{1, 1.f}, by_term{2, 1.f}, by_term{3, 1.5f}};
    And one;
    one.subs = {by_term{1, 1.f}};
    one.groups = {Or{{by_term{2, 1.f}}}, Or{{by_term{3, 1.5f}}}};
    {
      const auto pq = prepare({filter{flat}, filter{one}}, BM25{}, index);
      REQUIRE(same_entries(pq[0], pq[1]));
      for (const auto& e : pq[1].terms) REQUIRE(!(e.kind & IRS_HIP_GROUP_ALT));
    }
    // the boost product (term x Or x And), the flags of the members after a group's first
    And h;
    h.subs = {by_term{4, 0.5f}};
    h.groups = {Or{{by_term{1, 3.f}, by_term{2, 1.f}}, 1, IRS_HIP_MERGE_SUM, 2.f}};
    h.boost = 1.5f;
    {
      const auto pq = prepare({filter{h}}, BM25{}, index);
      REQUIRE(pq[0].op == IRS_HIP_OP_AND && pq[0].terms.size() == 3);
      const uint32_t terms[3] = {4, 1, 2};
      const float boosts[3] = {1.5f * 0.5f, (1.5f * 2.f) * 3.f, (1.5f * 2.f) * 1.f};
      for (int i = 0; i < 3; ++i) {
        TermStats st;
        BM25{}.collect(st, dwf, d.terms[terms[i]].docs_count, ttf);
        const irs_hip_term_scorer want = BM25{}.term_scorer(st, boosts[i]);
        REQUIRE(pq[0].terms[i].term == terms[i]);
        REQUIRE(pq[0].terms[i].c0 == want.c0);
        REQUIRE((pq[0].terms[i].kind & ~IRS_HIP_GROUP_ALT) == want.kind);
        REQUIRE(bool(pq[0].terms[i].kind & IRS_HIP_GROUP_ALT) == (i == 2));
      }
      // a flat Or's boost multiplies too
      const auto po = prepare({filter{Or{{by_term{1, 1.f}, by_term{2, 2.f}}, 1, IRS_HIP_MERGE_SUM, 3.f}},
                               filter{Or{{by_term{1, 3.f}, by_term{2, 6.f}}}}}, BM25{}, index);
      REQUIRE(same_entries(po[0], po[1]));
    }
    // refusals
    {
      auto refused_ns = [&](const And& a) {
        try {
          prepare({filter{a}}, BM25{}, index);
        } catch (const not_supported&) {
          return true;
        }
        return false;
      };
      And mm = one;
      mm.groups = {Or{{by_term{2, 1.f}, by_term{3, 1.f}}, 2}};
      REQUIRE(refused_ns(mm));
      And mx = one;
      mx.groups = {Or{{by_term{2, 1.f}, by_term{3, 1.f}}, 1, IRS_HIP_MERGE_MAX}};
      REQUIRE(refused_ns(mx));
      And many = one;
      many.groups = {Or{}};
      for (uint32_t t = 0; t < 16; ++t) many.groups[0].subs.push_back(by_term{t, 1.f});
      REQUIRE(refused_ns(many));
      And empty = one;
      empty.groups = {Or{}};
      bool threw = false;
      try {
        prepare({filter{empty}}, BM25{}, index);
      } catch (const illegal_argument&) {
        threw = true;
      }
      REQUIRE(threw);
    }
    // runs: a AND (b OR c) matches docs(a) n (docs(b) u docs(c)); with exclusions, the same And on
    // the segment with the excluded terms' docs deleted
    const uint32_t ta = 3, tb = 7, tc = 20, ex1 = 11, ex2 = 0;
    auto docs_of = [&](uint32_t t) {
      std::vector<uint32_t> v;
      seg.postings(t, v, nullptr, d.terms[t].docs_count);
      return v;
    };
    std::vector<uint32_t> bc, want;
    {
      const auto b = docs_of(tb), c = docs_of(tc), a = docs_of(ta);
      std::set_union(b.begin(), b.end(), c.begin(), c.end(), std::back_inserter(bc));
      std::set_intersection(a.begin(), a.end(), bc.begin(), bc.end(), std::back_inserter(want));
    }
    std::vector<uint32_t> gone;
    for (uint32_t t : {ex1, ex2}) {
      const auto v = docs_of(t);
      gone.insert(gone.end(), v.begin(), v.end());
    }
    std::sort(gone.begin(), gone.end());
    gone.erase(std::unique(gone.begin(), gone.end()), gone.end());
    irs_hip_segment_desc dm = d;
    dm.doc_mask = gone.data();
    dm.doc_mask_count = gone.size();
    SegmentReader masked(dm);

    And g;
    g.subs = {by_term{ta, 1.f}};
    g.groups = {Or{{by_term{tb, 1.f}, by_term{tc, 1.f}}}};
    const uint32_t k = 4096;
    const std::vector<filter> fx{g, Exclusion{g, {by_term{ex1, 1.f}, by_term{ex2, 1.f}}}};
    QueryBatch b1({&seg}, prepare(fx, BM25{}, index), k);
    QueryBatch b2({&masked}, prepare({filter{g}}, BM25{}, index), k);
    const QueryBatch::Results r1 = b1.run().results(), r2 = b2.run().results();
    REQUIRE(r1.total(0, 0) == want.size() && want.size() > 0);
    REQUIRE(r1.count(0, 0) == std::min<uint64_t>(k, want.size()));
    {
      std::vector<uint32_t> got;
      for (uint32_t i = 0; i < r1.count(0, 0); ++i) got.push_back(r1.of(0, 0)[i].doc);
      std::sort(got.begin(), got.end());
      REQUIRE(std::unique(got.begin(), got.end()) == got.end());
      REQUIRE(std::includes(want.begin(), want.end(), got.begin(), got.end()));
      if (want.size() <= k) REQUIRE(got == want);
    }
    REQUIRE(r1.total(0, 1) == r2.total(0, 0) && r1.count(0, 1) == r2.count(0, 0) && r1.total(0, 1) > 0);
    for (uint32_t i = 0; i < r1.count(0, 1); ++i) {
      const irs_hip_hit x = r1.of(0, 1)[i], y = r2.of(0, 0)[i];
      REQUIRE(x.doc == y.doc && std::fabs(x.score - y.score) <= 1e-5f * std::fabs(y.score));
      REQUIRE(!std::binary_search(gone.begin(), gone.end(), x.doc));
    }
    std::printf("test_nested_boolean OK: totals %llu %llu\n", (unsigned long long)r1.total(0, 0),
                (unsigned long long)r1.total(0, 1));
  }
  irs_synth_free(idx);
  return rc;
}
