// tests/cpp/test_phrases_and.cpp — TEST: the C++ host layer's And of SEVERAL by_phrases (and
// by_terms) — IRS_HIP_PHRASE_NEXT — through prepare() and QueryBatch: the opt-in
// (And::phrase_conjunction; without it two phrases are not_supported as they always were), the
// entries prepare() builds (each phrase its own blob from its own words, the first word of the
// second phrase flagged, every by_term its own statistics, the And's boost in all), and a run
// against the parts' own batches: the docs both phrases (and the term) hold, scores = the sum of
// the parts' scores.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
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

    const uint32_t a = 2, c = 3, e = 4, often = 12;
    by_phrase ac, ce;
    ac.push_back(a).push_back(c);
    ce.push_back(c).push_back(e, 1);      // c . e: offsets 0, 2
    ce.boost = 0.5f;
    And two, with_term;
    two.phrases = {ac, ce};
    two.boost = 2.f;
    with_term.phrases = {ac, ce};
    with_term.subs = {by_term{often, 1.f}};
    // the opt-in: unset, what it always was
    auto refused = [&](const And& bad) {
      try {
        prepare(std::vector<filter>{bad}, BM25{}, index);
      } catch (const not_supported&) { return true; }
      return false;
    };
    REQUIRE(refused(two) && refused(with_term));
    two.phrase_conjunction = with_term.phrase_conjunction = true;
    REQUIRE(!refused(two) && !refused(with_term));
    {
      And five = two, nine = with_term, var = two, grp = two, mx = two;
      five.phrases = {ac, ac, ac, ac, ac};
      nine.phrases = {ac, ce, ac, ce};
      by_phrase v;
      v.push_back(std::vector<uint32_t>{a, 91}).push_back(c);
      var.phrases = {ac, v};
      grp.groups.push_back(Or{{by_term{1, 1.f}, by_term{2, 1.f}}});
      mx.merge_type = IRS_HIP_MERGE_MAX;
      REQUIRE(refused(five) && refused(nine) && refused(var) && refused(grp) && refused(mx));
      And one_word = two;
      by_phrase w;
      w.push_back(a);
      one_word.phrases = {ac, w};
      bool threw = false;
      try {
        prepare(std::vector<filter>{one_word}, BM25{}, index);
      } catch (const illegal_argument&) { threw = true; }
      REQUIRE(threw);
    }
    const auto pv = prepare(std::vector<filter>{two, with_term}, BM25{}, index);
    REQUIRE(pv[0].op == IRS_HIP_OP_PHRASE && pv[0].terms.size() == 4 && pv[1].terms.size() == 5);
    const int32_t B = IRS_HIP_SCORE_BM25;
    REQUIRE(pv[1].terms[0].kind == B && pv[1].terms[1].kind == B && pv[1].terms[2].kind == (B | IRS_HIP_PHRASE_NEXT) &&
            pv[1].terms[3].kind == B && pv[1].terms[4].kind == (B | IRS_HIP_PHRASE_REQUIRED));
    REQUIRE(pv[0].terms[2].kind == (B | IRS_HIP_PHRASE_NEXT) && pv[0].terms[3].kind == B);
    REQUIRE(pv[1].terms[0].term == a && pv[1].terms[1].term == c && pv[1].terms[2].term == c &&
            pv[1].terms[3].term == e && pv[1].terms[4].term == often);
    REQUIRE(pv[1].terms[0].phrase_offset == 0 && pv[1].terms[1].phrase_offset == 1 &&
            pv[1].terms[2].phrase_offset == 0 && pv[1].terms[3].phrase_offset == 2 && pv[1].terms[4].phrase_offset == 0);
    {
      const uint64_t dwf = irs_synth_docs_with_field(idx), ttf = irs_synth_total_term_freq(idx);
      TermStats s1, s2;
      for (uint32_t t : {a, c}) BM25{}.collect(s1, dwf, d.terms[t].docs_count, ttf);
      for (uint32_t t : {c, e}) BM25{}.collect(s2, dwf, d.terms[t].docs_count, ttf);
      REQUIRE(pv[0].terms[0].c0 == BM25{}.term_scorer(s1, 2.f).c0 && pv[0].terms[1].c0 == pv[0].terms[0].c0);
      REQUIRE(pv[0].terms[2].c0 == BM25{}.term_scorer(s2, 2.f * 0.5f).c0 && pv[0].terms[3].c0 == pv[0].terms[2].c0);
      REQUIRE(pv[0].terms[2].c0 != pv[0].terms[0].c0);
    }

    const uint32_t k = IRS_HIP_MAX_K;
    // without boosts: scores that add up from the parts' own batches
    And two1 = two, term1 = with_term;
    by_phrase ce1 = ce;
    ce1.boost = 1.f;
    two1.boost = 1.f;
    two1.phrases = {ac, ce1};
    term1.phrases = {ac, ce1};
    QueryBatch bq({&seg}, prepare(std::vector<filter>{two1, term1, ac}, BM25{}, index), k);
    REQUIRE(bq.phrase_conj_units() == 2);
    QueryBatch bp({&seg}, prepare(std::vector<filter>{ac, ce1}, BM25{}, index), k);
    REQUIRE(bp.phrase_conj_units() == 0);
    const QueryBatch::Results rq = bq.run().results(), rp = bp.run().results();
    REQUIRE(rp.total(0, 0) > 0 && rp.total(0, 0) < k && rp.total(0, 1) > 0 && rp.total(0, 1) < k);
    // the plain phrase next to the units of two phrases: bit for bit what it gives in a batch without them
    REQUIRE(rq.count(0, 2) == rp.count(0, 0) && rq.total(0, 2) == rp.total(0, 0));
    for (uint32_t i = 0; i < rp.count(0, 0); ++i) {
      const irs_hip_hit x = rq.of(0, 2)[i], y = rp.of(0, 0)[i];
      REQUIRE(x.doc == y.doc && std::memcmp(&x.score, &y.score, 4) == 0);
    }
    std::map<uint32_t, float> s_ac, s_ce;
    for (uint32_t i = 0; i < rp.count(0, 0); ++i) s_ac[rp.of(0, 0)[i].doc] = rp.of(0, 0)[i].score;
    for (uint32_t i = 0; i < rp.count(0, 1); ++i) s_ce[rp.of(0, 1)[i].doc] = rp.of(0, 1)[i].score;
    std::vector<uint32_t> term_docs, term_freqs;
    seg.postings(often, term_docs, &term_freqs, d.terms[often].docs_count);
    // query 0: the docs of both phrases, score = the sum of the two
    std::vector<uint32_t> want0, want1, got;
    for (const auto& kv : s_ac)
      if (s_ce.count(kv.first)) {
        want0.push_back(kv.first);
        if (std::binary_search(term_docs.begin(), term_docs.end(), kv.first)) want1.push_back(kv.first);
      }
    for (uint32_t i = 0; i < rq.count(0, 0); ++i) got.push_back(rq.of(0, 0)[i].doc);
    std::sort(got.begin(), got.end());
    REQUIRE(got == want0 && rq.total(0, 0) == want0.size() && !want0.empty());
    for (uint32_t i = 0; i < rq.count(0, 0); ++i) {
      const irs_hip_hit x = rq.of(0, 0)[i];
      const float sum = s_ac[x.doc] + s_ce[x.doc];
      REQUIRE(std::fabs(x.score - sum) <= 1e-5f * sum);
      if (i) REQUIRE(rq.of(0, 0)[i - 1].score > x.score || (rq.of(0, 0)[i - 1].score == x.score && rq.of(0, 0)[i - 1].doc < x.doc));
    }
    // query 1: ... that the required term holds too, each scoring above the two phrases alone
    got.clear();
    for (uint32_t i = 0; i < rq.count(0, 1); ++i) got.push_back(rq.of(0, 1)[i].doc);
    std::sort(got.begin(), got.end());
    REQUIRE(got == want1 && rq.total(0, 1) == want1.size() && !want1.empty() && want1.size() < want0.size());
    for (uint32_t i = 0; i < rq.count(0, 1); ++i) {
      const irs_hip_hit x = rq.of(0, 1)[i];
      REQUIRE(x.score > s_ac[x.doc] + s_ce[x.doc]);
    }
    std::printf("test_phrases_and OK: totals %llu %llu of %llu and %llu\n", (unsigned long long)want0.size(),
                (unsigned long long)want1.size(), (unsigned long long)rp.total(0, 0), (unsigned long long)rp.total(0, 1));
  }
  irs_synth_free(idx);
  return rc;
}
