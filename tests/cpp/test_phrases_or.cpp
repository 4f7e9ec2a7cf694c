// tests/cpp/test_phrases_or.cpp — TEST: the C++ host layer's Or of SEVERAL by_phrases —
// IRS_HIP_PHRASE_OR — through prepare() and QueryBatch: the opt-in (Or::phrase_disjunction; without
// it two phrases are not_supported as they always were), the entries prepare() builds (each phrase
// its own blob from its own words, the first word of the second phrase flagged, the Or's boost in
// all), and a run against the phrases' own batches: the docs either phrase holds, each once, scores
// = the sum of the scores of the phrases that match.
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

    const uint32_t a = 2, c = 3, e = 4;
    by_phrase ac, ce;
    ac.push_back(a).push_back(c);
    ce.push_back(c).push_back(e, 1);      // c . e: offsets 0, 2
    ce.boost = 0.5f;
    Or two;
    two.phrases = {ac, ce};
    two.boost = 2.f;
    // the opt-in: unset, what it always was
    auto refused = [&](const Or& bad) {
      try {
        prepare(std::vector<filter>{bad}, BM25{}, index);
      } catch (const not_supported&) { return true; }
      return false;
    };
    REQUIRE(refused(two));
    two.phrase_disjunction = true;
    REQUIRE(!refused(two));
    {
      Or five = two, nine = two, var = two, term = two, mm = two, mx = two;
      five.phrases = {ac, ac, ac, ac, ac};
      by_phrase ace;
      ace.push_back(a).push_back(c).push_back(e);
      nine.phrases = {ace, ace, ace};
      by_phrase v;
      v.push_back(std::vector<uint32_t>{a, 91}).push_back(c);
      var.phrases = {ac, v};
      term.subs = {by_term{12, 1.f}};
      mm.min_match_count = 2;
      mx.merge_type = IRS_HIP_MERGE_MAX;
      REQUIRE(refused(five) && refused(nine) && refused(var) && refused(term) && refused(mm) && refused(mx));
      Or one_word = two;
      by_phrase w;
      w.push_back(a);
      one_word.phrases = {ac, w};
      bool threw = false;
      try {
        prepare(std::vector<filter>{one_word}, BM25{}, index);
      } catch (const illegal_argument&) { threw = true; }
      REQUIRE(threw);
    }
    const auto pv = prepare(std::vector<filter>{two}, BM25{}, index);
    REQUIRE(pv[0].op == IRS_HIP_OP_PHRASE && pv[0].terms.size() == 4);
    const int32_t B = IRS_HIP_SCORE_BM25;
    REQUIRE(pv[0].terms[0].kind == B && pv[0].terms[1].kind == B && pv[0].terms[2].kind == (B | IRS_HIP_PHRASE_OR) &&
            pv[0].terms[3].kind == B);
    REQUIRE(pv[0].terms[0].term == a && pv[0].terms[1].term == c && pv[0].terms[2].term == c && pv[0].terms[3].term == e);
    REQUIRE(pv[0].terms[0].phrase_offset == 0 && pv[0].terms[1].phrase_offset == 1 &&
            pv[0].terms[2].phrase_offset == 0 && pv[0].terms[3].phrase_offset == 2);
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
    // without boosts: scores that add up from the phrases' own batches
    Or two1 = two, rev1 = two;
    by_phrase ce1 = ce;
    ce1.boost = 1.f;
    two1.boost = rev1.boost = 1.f;
    two1.phrases = {ac, ce1};
    rev1.phrases = {ce1, ac};
    QueryBatch bq({&seg}, prepare(std::vector<filter>{two1, rev1, ac}, BM25{}, index), k);
    REQUIRE(bq.phrase_disj_units() == 2);
    QueryBatch bp({&seg}, prepare(std::vector<filter>{ac, ce1}, BM25{}, index), k);
    REQUIRE(bp.phrase_disj_units() == 0);
    const QueryBatch::Results rq = bq.run().results(), rp = bp.run().results();
    REQUIRE(rp.total(0, 0) > 0 && rp.total(0, 1) > 0 && rp.total(0, 0) + rp.total(0, 1) < k);
    // the plain phrase next to the units of two phrases: bit for bit what it gives in a batch without them
    REQUIRE(rq.count(0, 2) == rp.count(0, 0) && rq.total(0, 2) == rp.total(0, 0));
    for (uint32_t i = 0; i < rp.count(0, 0); ++i) {
      const irs_hip_hit x = rq.of(0, 2)[i], y = rp.of(0, 0)[i];
      REQUIRE(x.doc == y.doc && std::memcmp(&x.score, &y.score, 4) == 0);
    }
    std::map<uint32_t, float> s_ac, s_ce;
    for (uint32_t i = 0; i < rp.count(0, 0); ++i) s_ac[rp.of(0, 0)[i].doc] = rp.of(0, 0)[i].score;
    for (uint32_t i = 0; i < rp.count(0, 1); ++i) s_ce[rp.of(0, 1)[i].doc] = rp.of(0, 1)[i].score;
    // the docs of either phrase, each once; a doc of both scores the sum of the two
    std::vector<uint32_t> want;
    size_t both = 0;
    for (const auto& kv : s_ac) {
      want.push_back(kv.first);
      both += s_ce.count(kv.first);
    }
    for (const auto& kv : s_ce)
      if (!s_ac.count(kv.first)) want.push_back(kv.first);
    std::sort(want.begin(), want.end());
    REQUIRE(both > 0 && both < s_ac.size() && both < s_ce.size());
    for (uint32_t q = 0; q < 2; ++q) {   // both orders: ownership from either side
      std::vector<uint32_t> got;
      for (uint32_t i = 0; i < rq.count(0, q); ++i) got.push_back(rq.of(0, q)[i].doc);
      std::sort(got.begin(), got.end());
      REQUIRE(got == want && rq.total(0, q) == want.size());
      for (uint32_t i = 0; i < rq.count(0, q); ++i) {
        const irs_hip_hit x = rq.of(0, q)[i];
        const bool in_ac = s_ac.count(x.doc) != 0, in_ce = s_ce.count(x.doc) != 0;
        const float sum = in_ac && in_ce ? (q == 0 ? s_ac[x.doc] + s_ce[x.doc] : s_ce[x.doc] + s_ac[x.doc])
                          : in_ac ? s_ac[x.doc] : s_ce[x.doc];
        REQUIRE(std::fabs(x.score - sum) <= 1e-5f * sum);
        if (!(in_ac && in_ce)) REQUIRE(std::memcmp(&x.score, &sum, 4) == 0);   // one phrase: its value as it is
        if (i) REQUIRE(rq.of(0, q)[i - 1].score > x.score || (rq.of(0, q)[i - 1].score == x.score && rq.of(0, q)[i - 1].doc < x.doc));
      }
    }
    std::printf("test_phrases_or OK: %llu docs, %llu of both phrases, of %llu and %llu\n", (unsigned long long)want.size(),
                (unsigned long long)both, (unsigned long long)rp.total(0, 0), (unsigned long long)rp.total(0, 1));
  }
  irs_synth_free(idx);
  return rc;
}
