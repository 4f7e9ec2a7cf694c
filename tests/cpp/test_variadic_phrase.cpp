// tests/cpp/test_variadic_phrase.cpp — TEST: the C++ host layer's variadic by_phrase (a part that
// stands for a set of terms, by_phrase::push_back(std::vector<uint32_t>)) through prepare() and
// QueryBatch: the entries and the one stats blob prepare() builds, its refusals, and results — the
// docs of (a|b) c are those of "a c" and of "b c", one-member parts give the plain phrase's
// results bit for bit, Not under an And removes the excluded term's docs.
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
  p.seed = 20261016;
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

    // prepare(): entries part after part, the members after a part's first flagged; ONE blob
    // with the idf of every slot (one segment: slot i of a part = its i-th present member)
    const uint32_t a = 90, b = 91, c = 95, e = 100;
    by_phrase v;
    v.push_back(std::vector<uint32_t>{a, b}).push_back(c);
    const auto pv = prepare(std::vector<filter>{v}, BM25{}, index);
    REQUIRE(pv[0].op == IRS_HIP_OP_PHRASE && pv[0].terms.size() == 3);
    REQUIRE(pv[0].terms[0].kind == IRS_HIP_SCORE_BM25 &&
            pv[0].terms[1].kind == (IRS_HIP_SCORE_BM25 | IRS_HIP_PHRASE_ALT) &&
            pv[0].terms[2].kind == IRS_HIP_SCORE_BM25);
    REQUIRE(pv[0].terms[1].phrase_offset == 0 && pv[0].terms[2].phrase_offset == 1);
    {
      TermStats st;
      const uint64_t dwf = irs_synth_docs_with_field(idx), ttf = irs_synth_total_term_freq(idx);
      for (uint32_t t : {a, b, c}) BM25{}.collect(st, dwf, d.terms[t].docs_count, ttf);
      REQUIRE(pv[0].terms[0].c0 == BM25{}.term_scorer(st, 1.f).c0);
    }
    // refused: one part, 17 members, a term twice in a part
    bool threw = false;
    try {
      by_phrase one;
      one.push_back(std::vector<uint32_t>{a, b});
      prepare(std::vector<filter>{one}, BM25{}, index);
    } catch (const illegal_argument&) { threw = true; }
    REQUIRE(threw);
    threw = false;
    try {
      by_phrase big;
      big.push_back(std::vector<uint32_t>{0, 1, 2, 3, 4, 5, 6, 7, 8}).push_back(std::vector<uint32_t>{9, 10, 11, 12, 13, 14, 15, 16});
      prepare(std::vector<filter>{big}, BM25{}, index);
    } catch (const not_supported&) { threw = true; }
    REQUIRE(threw);
    threw = false;
    try {
      by_phrase twice;
      twice.push_back(std::vector<uint32_t>{a, a}).push_back(c);
      prepare(std::vector<filter>{twice}, BM25{}, index);
    } catch (const illegal_argument&) { threw = true; }
    REQUIRE(threw);

    // (a|b) c matches the docs of "a c" and those of "b c"; one-member parts on the variadic kernel
    // give what the plain phrases give, bit for bit
    by_phrase ac, bc, ac1, ce;
    ac.push_back(a).push_back(c);
    bc.push_back(b).push_back(c);
    ac1.push_back(std::vector<uint32_t>{a}).push_back(std::vector<uint32_t>{c});
    ce.push_back(c).push_back(std::vector<uint32_t>{e, a, b}, 1);
    const uint32_t k = IRS_HIP_MAX_K;
    QueryBatch bv({&seg}, prepare(std::vector<filter>{v, ac1, ce, Exclusion{v, {by_term{a, 1.f}}}}, BM25{}, index), k);
    QueryBatch bp({&seg}, prepare(std::vector<filter>{ac, bc}, BM25{}, index), k);
    const QueryBatch::Results rv = bv.run().results(), rp = bp.run().results();
    REQUIRE(rp.total(0, 0) > 0 && rp.total(0, 1) > 0 && rv.total(0, 0) < k);
    std::vector<uint32_t> want, got, ex;
    for (uint32_t q = 0; q < 2; ++q)
      for (uint32_t i = 0; i < rp.count(0, q); ++i) want.push_back(rp.of(0, q)[i].doc);
    std::sort(want.begin(), want.end());
    want.erase(std::unique(want.begin(), want.end()), want.end());
    for (uint32_t i = 0; i < rv.count(0, 0); ++i) got.push_back(rv.of(0, 0)[i].doc);
    std::sort(got.begin(), got.end());
    REQUIRE(got == want && rv.total(0, 0) == want.size());
    REQUIRE(rv.count(0, 1) == rp.count(0, 0) && rv.total(0, 1) == rp.total(0, 0));
    for (uint32_t i = 0; i < rv.count(0, 1); ++i) {
      const irs_hip_hit x = rv.of(0, 1)[i], y = rp.of(0, 0)[i];
      REQUIRE(x.doc == y.doc && std::memcmp(&x.score, &y.score, 4) == 0);
    }
    // Not(a): the docs of "b c" without a
    seg.postings(a, ex, nullptr, d.terms[a].docs_count);
    for (uint32_t i = 0; i < rv.count(0, 3); ++i)
      REQUIRE(!std::binary_search(ex.begin(), ex.end(), rv.of(0, 3)[i].doc));
    REQUIRE(rv.total(0, 3) > 0 && rv.total(0, 3) <= rp.total(0, 1));
    std::printf("test_variadic_phrase OK: totals %llu %llu %llu %llu\n", (unsigned long long)rv.total(0, 0),
                (unsigned long long)rv.total(0, 1), (unsigned long long)rv.total(0, 2),
                (unsigned long long)rv.total(0, 3));
  }
  irs_synth_free(idx);
  return rc;
}
