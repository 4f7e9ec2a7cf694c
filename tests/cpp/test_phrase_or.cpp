// tests/cpp/test_phrase_or.cpp — TEST: the C++ host layer's Or of ONE by_phrase and by_terms (a
// phrase or optional terms, IRS_HIP_PHRASE_OPTIONAL) through prepare() and QueryBatch: the entries
// prepare() builds (the phrase's one blob from its own words, every by_term its own statistics, the
// Or's boost in both), its refusals, and a query against the docs worked out from the plain
// phrase's results and the term's postings: the union, scores = the phrase's + the term's own
// where both hold the doc.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
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
  p.seed = 20261018;
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

    const uint32_t a = 10, c = 12, rare = 120;
    by_phrase ac;
    ac.push_back(a).push_back(c);
    Or q1, q2;
    q1.phrases = {ac};
    q1.subs = {by_term{rare, 1.f}};
    q2.phrases = {ac};
    q2.subs = {by_term{rare, 0.5f}};
    q2.boost = 2.f;
    const auto pv = prepare(std::vector<filter>{q1, q2, ac}, BM25{}, index);
    REQUIRE(pv[1].op == IRS_HIP_OP_PHRASE && pv[1].terms.size() == 3);
    REQUIRE(pv[1].terms[0].kind == IRS_HIP_SCORE_BM25 && pv[1].terms[1].kind == IRS_HIP_SCORE_BM25 &&
            pv[1].terms[2].kind == (IRS_HIP_SCORE_BM25 | IRS_HIP_PHRASE_OPTIONAL));
    REQUIRE(pv[1].terms[0].term == a && pv[1].terms[1].term == c && pv[1].terms[2].term == rare);
    REQUIRE(pv[1].terms[1].phrase_offset == 1 && pv[1].terms[2].phrase_offset == 0);
    {
      const uint64_t dwf = irs_synth_docs_with_field(idx), ttf = irs_synth_total_term_freq(idx);
      TermStats st, rt;
      for (uint32_t t : {a, c}) BM25{}.collect(st, dwf, d.terms[t].docs_count, ttf);
      BM25{}.collect(rt, dwf, d.terms[rare].docs_count, ttf);
      REQUIRE(pv[1].terms[0].c0 == BM25{}.term_scorer(st, 2.f).c0 && pv[1].terms[1].c0 == pv[1].terms[0].c0);
      REQUIRE(pv[1].terms[2].c0 == BM25{}.term_scorer(rt, 2.f * 0.5f).c0);
      REQUIRE(pv[0].terms[0].c0 == BM25{}.term_scorer(st, 1.f).c0);
    }
    // refused: two phrases, a variadic phrase, min_match_count > 1, a non-SUM merge, 9 entries
    auto refused = [&](const Or& bad) {
      try {
        prepare(std::vector<filter>{bad}, BM25{}, index);
      } catch (const not_supported&) { return true; }
      return false;
    };
    {
      Or two = q1, var = q1, mm = q1, mx = q1, big = q1;
      two.phrases.push_back(ac);
      by_phrase v;
      v.push_back(std::vector<uint32_t>{a, 91}).push_back(c);
      var.phrases = {v};
      mm.min_match_count = 2;
      mx.merge_type = IRS_HIP_MERGE_MAX;
      for (uint32_t t = 10; t < 17; ++t) big.subs.push_back(by_term{t, 1.f});
      REQUIRE(refused(two) && refused(var) && refused(mm) && refused(mx) && refused(big));
      REQUIRE(!refused(q1));
    }

    const uint32_t k = IRS_HIP_MAX_K;
    QueryBatch bq({&seg}, pv, k);
    QueryBatch bp({&seg}, prepare(std::vector<filter>{ac}, BM25{}, index), k);
    QueryBatch bt({&seg}, prepare(std::vector<filter>{by_term{rare, 1.f}}, BM25{}, index), k);
    const QueryBatch::Results rq = bq.run().results(), rp = bp.run().results(), rt = bt.run().results();
    REQUIRE(rp.total(0, 0) > 0 && rt.total(0, 0) > 0 && rp.total(0, 0) + rt.total(0, 0) < k);
    // the plain phrase next to units with optional terms: bit for bit what it gives alone
    REQUIRE(rq.count(0, 2) == rp.count(0, 0) && rq.total(0, 2) == rp.total(0, 0));
    for (uint32_t i = 0; i < rp.count(0, 0); ++i) {
      const irs_hip_hit x = rq.of(0, 2)[i], y = rp.of(0, 0)[i];
      REQUIRE(x.doc == y.doc && std::memcmp(&x.score, &y.score, 4) == 0);
    }
    // the docs: the phrase's and the term's; the scores: the phrase's (its own batch) + the term's
    // (its own batch) where each holds the doc, float32
    std::vector<uint32_t> want, got;
    for (uint32_t i = 0; i < rp.count(0, 0); ++i) want.push_back(rp.of(0, 0)[i].doc);
    for (uint32_t i = 0; i < rt.count(0, 0); ++i) want.push_back(rt.of(0, 0)[i].doc);
    std::sort(want.begin(), want.end());
    const size_t listed = want.size();
    want.erase(std::unique(want.begin(), want.end()), want.end());
    const size_t both = listed - want.size();
    for (uint32_t i = 0; i < rq.count(0, 0); ++i) got.push_back(rq.of(0, 0)[i].doc);
    std::sort(got.begin(), got.end());
    REQUIRE(got == want && rq.total(0, 0) == want.size() && rq.total(0, 1) == want.size());
    for (uint32_t i = 0; i < rq.count(0, 0); ++i) {
      const irs_hip_hit x = rq.of(0, 0)[i];
      float sum = 0.f;
      for (uint32_t j = 0; j < rp.count(0, 0); ++j) if (rp.of(0, 0)[j].doc == x.doc) sum += rp.of(0, 0)[j].score;
      for (uint32_t j = 0; j < rt.count(0, 0); ++j) if (rt.of(0, 0)[j].doc == x.doc) sum += rt.of(0, 0)[j].score;
      REQUIRE(sum > 0.f && std::fabs(x.score - sum) <= 1e-5f * sum);
      if (i) REQUIRE(rq.of(0, 0)[i - 1].score > x.score || (rq.of(0, 0)[i - 1].score == x.score && rq.of(0, 0)[i - 1].doc < x.doc));
    }
    REQUIRE(both > 0);
    std::printf("test_phrase_or OK: %llu docs, %llu through both children\n", (unsigned long long)want.size(),
                (unsigned long long)both);
  }
  irs_synth_free(idx);
  return rc;
}
