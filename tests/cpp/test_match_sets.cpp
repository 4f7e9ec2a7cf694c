// tests/cpp/test_match_sets.cpp — TEST: unscored execution through the C++ host layer:
// execute_unscored(reader, filter) for by_term / Or / And (flat and grouped) / Exclusion / by_phrase
// and QueryBatch::match_sets, every set bit for bit against the oracle's C API (orc_score_all's
// `matched`, orc_score_all_phrase's frequencies; an exclusion = the excluded terms' docs added to
// the oracle segment's doc mask; a grouped And = the AND of the oracle's Ors), the counts against
// the populations and against the total_hits of the scored run of the same batch.
#include <algorithm>
#include <cstdio>
#include <cstring>
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
  irs_synth_params p{};
  p.seed = 20261016;
  p.num_docs = 30000;
  p.vocab_log2 = 20;
  p.max_rank = 96;
  p.layout = IRS_SYNTH_LAYOUT_SIMD4;
  p.mean_len = 100;
  p.stddev_len = 30;
  p.with_positions = 1;
  irs_synth_index* idx = nullptr;
  REQUIRE(irs_synth_build(&p, &idx) == 0);
  {
    uint64_t doc_len = 0, norm_count = 0, pos_len = 0;
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
    // deleted docs: a run and a stride
    std::vector<uint32_t> gone;
    for (uint32_t x = 300; x < 500; ++x) gone.push_back(x);
    for (uint32_t x = 1; x <= p.num_docs; x += 17) gone.push_back(x);
    std::sort(gone.begin(), gone.end());
    gone.erase(std::unique(gone.begin(), gone.end()), gone.end());
    d.doc_mask = gone.data();
    d.doc_mask_count = gone.size();
    SegmentReader seg(d);
    const uint64_t dwf = irs_synth_docs_with_field(idx), ttf = irs_synth_total_term_freq(idx);
    const SegmentStats stats{dwf, ttf, d.terms, num_terms};
    const uint32_t n1 = p.num_docs + 1;
    const orc_scorer osc{ORC_SCORER_BM25, 1.2f, 0.75f, 0};

    auto view_with = [&](const std::vector<uint32_t>& mask) {
      orc_segment v{};
      v.doc_file = static_cast<const uint8_t*>(d.doc_file);
      v.doc_file_len = doc_len;
      v.layout = ORC_LAYOUT_SIMD4;
      v.num_docs = p.num_docs;
      v.norms = static_cast<const uint8_t*>(d.norms);
      v.norm_width = 1;
      v.pos_file = static_cast<const uint8_t*>(d.pos_file);
      v.pos_file_len = pos_len;
      v.doc_mask = mask.data();
      v.doc_mask_count = mask.size();
      return v;
    };
    auto meta_of = [&](uint32_t t) {
      orc_term_meta m{};
      if (t < num_terms) std::memcpy(&m, &d.terms[t], sizeof m);
      return m;
    };
    // the segment's mask plus every doc of the excluded terms
    auto mask_with = [&](const std::vector<uint32_t>& excluded) {
      std::vector<uint32_t> m = gone;
      for (uint32_t t : excluded) {
        if (t >= num_terms) continue;
        std::vector<uint32_t> docs;
        seg.postings(t, docs, nullptr, d.terms[t].docs_count);
        m.insert(m.end(), docs.begin(), docs.end());
      }
      return m;
    };
    auto oracle_bool = [&](const std::vector<uint32_t>& terms, int32_t op, const std::vector<uint32_t>& mask,
                           std::vector<uint8_t>& matched) {
      const orc_segment v = view_with(mask);
      std::vector<orc_term_meta> metas;
      std::vector<uint64_t> dwt;
      for (uint32_t t : terms) {
        metas.push_back(meta_of(t));
        dwt.push_back(t < num_terms ? d.terms[t].docs_count : 0);
      }
      std::vector<float> scores(n1);
      matched.assign(n1, 0);
      return orc_score_all(&v, metas.data(), uint32_t(terms.size()), op, &osc, nullptr, dwf, dwt.data(), ttf,
                           scores.data(), matched.data()) >= 0;
    };
    auto same = [&](const DocSet& got, const std::vector<uint8_t>& want) {
      uint64_t n = 0;
      for (uint32_t doc = 0; doc < n1; ++doc) {
        if (got.contains(doc) != (want[doc] != 0)) {
          std::fprintf(stderr, "doc %u: got %d want %d\n", doc, int(got.contains(doc)), int(want[doc]));
          return false;
        }
        n += want[doc] != 0;
      }
      for (uint32_t doc = n1; doc < 64 * got.words.size(); ++doc)
        if (got.contains(doc)) return false;
      return got.count() == n && got.postings == n;
    };
    std::vector<uint8_t> want, other;

    // by_term
    REQUIRE(oracle_bool({5}, ORC_OP_OR, gone, want));
    REQUIRE(same(execute_unscored(seg, stats, p.num_docs, by_term{5, 1.f}), want));
    // Or, min-match
    const Or o3{{by_term{1, 1.f}, by_term{40, 1.f}, by_term{90, 2.f}}};
    REQUIRE(oracle_bool({1, 40, 90}, ORC_OP_OR, gone, want));
    REQUIRE(same(execute_unscored(seg, stats, p.num_docs, o3), want));
    Or mm{{by_term{0, 1.f}, by_term{1, 1.f}, by_term{2, 1.f}, by_term{3, 1.f}}, 3};
    REQUIRE(oracle_bool({0, 1, 2, 3}, ORC_OP_MINMATCH | (3 << 8), gone, want));
    REQUIRE(same(execute_unscored(seg, stats, p.num_docs, mm), want));
    // And, flat and grouped: a AND (b OR c)
    And a3;
    a3.subs = {by_term{0, 1.f}, by_term{2, 1.f}, by_term{30, 1.f}};
    REQUIRE(oracle_bool({0, 2, 30}, ORC_OP_AND, gone, want));
    REQUIRE(same(execute_unscored(seg, stats, p.num_docs, a3), want));
    And g;
    g.subs = {by_term{3, 1.f}};
    g.groups = {Or{{by_term{7, 1.f}, by_term{20, 1.f}}}};
    REQUIRE(oracle_bool({3}, ORC_OP_OR, gone, want));
    REQUIRE(oracle_bool({7, 20}, ORC_OP_OR, gone, other));
    for (uint32_t i = 0; i < n1; ++i) want[i] = want[i] && other[i];
    REQUIRE(same(execute_unscored(seg, stats, p.num_docs, g), want));
    // Exclusion: the included filter on the segment with the excluded terms' docs masked too
    const std::vector<uint32_t> ex{11, 0, 5000};
    const Exclusion xg{g, {by_term{11, 1.f}, by_term{0, 1.f}, by_term{5000, 1.f}}};
    REQUIRE(oracle_bool({3}, ORC_OP_OR, mask_with(ex), want));
    REQUIRE(oracle_bool({7, 20}, ORC_OP_OR, mask_with(ex), other));
    for (uint32_t i = 0; i < n1; ++i) want[i] = want[i] && other[i];
    REQUIRE(same(execute_unscored(seg, stats, p.num_docs, xg), want));
    const Exclusion xo{o3, {by_term{2, 1.f}}};
    REQUIRE(oracle_bool({1, 40, 90}, ORC_OP_OR, mask_with({2}), want));
    REQUIRE(same(execute_unscored(seg, stats, p.num_docs, xo), want));
    // by_phrase, with and without an exclusion; an absent term
    auto oracle_phrase = [&](const std::vector<uint32_t>& terms, const std::vector<uint32_t>& offs,
                             const std::vector<uint32_t>& mask, std::vector<uint8_t>& matched) {
      const orc_segment v = view_with(mask);
      std::vector<orc_term_meta> metas;
      std::vector<uint64_t> dwt;
      for (uint32_t t : terms) {
        metas.push_back(meta_of(t));
        dwt.push_back(d.terms[t].docs_count);
      }
      std::vector<float> scores(n1);
      std::vector<uint32_t> pf(n1);
      if (orc_score_all_phrase(&v, metas.data(), uint32_t(terms.size()), offs.data(), &osc, 1.f, dwf,
                               dwt.data(), ttf, scores.data(), pf.data()) < 0)
        return false;
      matched.assign(n1, 0);
      for (uint32_t i = 0; i < n1; ++i) matched[i] = pf[i] > 0;
      return true;
    };
    by_phrase ph;
    ph.push_back(0).push_back(1);
    REQUIRE(oracle_phrase({0, 1}, {0, 1}, gone, want));
    REQUIRE(same(execute_unscored(seg, stats, p.num_docs, ph), want));
    by_phrase ph3;
    ph3.push_back(2).push_back(0).push_back(1, 1);
    REQUIRE(oracle_phrase({2, 0, 1}, {0, 1, 3}, gone, want));
    REQUIRE(same(execute_unscored(seg, stats, p.num_docs, ph3), want));
    REQUIRE(oracle_phrase({0, 1}, {0, 1}, mask_with({2}), want));
    REQUIRE(same(execute_unscored(seg, stats, p.num_docs, Exclusion{ph, {by_term{2, 1.f}}}), want));
    by_phrase absent;
    absent.push_back(0).push_back(5000);
    REQUIRE(execute_unscored(seg, stats, p.num_docs, absent).count() == 0);

    // QueryBatch::match_sets over a mixed list (boolean and phrase parts stitched back in the
    // caller's order), before and after run(); counts == total_hits; counts alone; the errors
    const std::vector<filter> all{by_term{5, 1.f}, ph, o3, a3, ph3, g, xg, mm};
    const uint64_t n_words = (uint64_t(p.num_docs) + 1 + 63) / 64;
    QueryBatch batch({&seg}, prepare(all, BM25{}, {stats}), 100);
    const QueryBatch::MatchSets m0 = batch.match_sets(n_words);
    const QueryBatch::Results r = batch.run().results();
    const QueryBatch::MatchSets m1 = batch.match_sets(n_words), mc = batch.match_sets(n_words, false);
    REQUIRE(m0.words == m1.words && m0.counts == m1.counts && mc.counts == m0.counts && mc.words.empty());
    for (uint32_t q = 0; q < all.size(); ++q) {
      REQUIRE(m0.count(0, q) == r.total(0, q));
      const DocSet one = execute_unscored(seg, stats, p.num_docs, all[q]);
      REQUIRE(std::equal(one.words.begin(), one.words.end(), m0.of(0, q)) && one.postings == m0.count(0, q));
      for (uint32_t i = 0; i < r.count(0, q); ++i) REQUIRE(m0.contains(0, q, r.of(0, q)[i].doc));
      for (uint32_t x : gone) REQUIRE(!m0.contains(0, q, x));
    }
    bool threw = false;
    try {
      batch.match_sets(p.num_docs / 64);   // too few words for the segment
    } catch (const illegal_argument&) {
      threw = true;
    }
    REQUIRE(threw);
    threw = false;
    try {
      batch.match_sets_to_device(nullptr, n_words, nullptr);   // a mixed batch has two device batches
    } catch (const not_supported&) {
      threw = true;
    }
    REQUIRE(threw);
    std::printf("test_match_sets OK: counts %llu %llu %llu\n", (unsigned long long)m0.count(0, 0),
                (unsigned long long)m0.count(0, 1), (unsigned long long)m0.count(0, 6));
  }
  irs_synth_free(idx);
  return 0;
}
