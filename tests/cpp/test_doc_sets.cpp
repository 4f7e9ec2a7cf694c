// tests/cpp/test_doc_sets.cpp — TEST: the C++ host layer's by_doc_set (the unscored child of an
// And, next to its Nots) through prepare() and QueryBatch::set_doc_sets, host and DeviceBuffer
// forms.  What it must give: the included filter's results on the same segment with every doc
// outside the set (and every doc of the excluded terms) deleted — checked against the oracle's C
// API (orc_score_all on the complement-masked segment) for the boolean queries, and against the
// library's own run on that masked segment for the phrase.
#include <algorithm>
#include <cmath>
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
  p.seed = 20261017;
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
    std::vector<uint32_t> gone;
    for (uint32_t x = 200; x < 260; ++x) gone.push_back(x);
    d.doc_mask = gone.data();
    d.doc_mask_count = gone.size();
    SegmentReader seg(d);
    const uint64_t dwf = irs_synth_docs_with_field(idx), ttf = irs_synth_total_term_freq(idx);
    const std::vector<SegmentStats> index{SegmentStats{dwf, ttf, d.terms, num_terms}};

    // two rows: every third doc; a contiguous range (a stride larger than the segment needs)
    const uint64_t n_words = p.num_docs / 64 + 1 + 5, n_rows = 2;
    std::vector<uint64_t> sets(n_rows * n_words, 0);
    auto allowed = [&](uint32_t row, uint32_t doc) {
      return row == 0 ? doc % 3 == 1 : (doc >= 9000 && doc < 21000);
    };
    for (uint32_t row = 0; row < n_rows; ++row)
      for (uint32_t doc = 1; doc <= p.num_docs; ++doc)
        if (allowed(row, doc)) sets[row * n_words + doc / 64] |= uint64_t(1) << (doc % 64);
    const uint32_t ex = 9;
    std::vector<uint32_t> ex_docs;
    seg.postings(ex, ex_docs, nullptr, d.terms[ex].docs_count);
    // the complement-masked segment of (row, with the excluded term or without)
    auto mask_of = [&](uint32_t row, bool excluded) {
      std::vector<uint32_t> m = gone;
      for (uint32_t doc = 1; doc <= p.num_docs; ++doc)
        if (!allowed(row, doc)) m.push_back(doc);
      if (excluded) m.insert(m.end(), ex_docs.begin(), ex_docs.end());
      std::sort(m.begin(), m.end());
      m.erase(std::unique(m.begin(), m.end()), m.end());
      return m;
    };

    Or o;
    for (uint32_t t : {1u, 5u, 12u, 33u, 70u}) o.subs.push_back(by_term{t, 1.f});
    Or mm = o;
    mm.min_match_count = 2;
    And a;
    a.subs = {by_term{0, 1.f}, by_term{3, 1.f}};
    by_phrase ph;
    ph.push_back(0).push_back(1);
    const std::vector<filter> filters{
        Exclusion{o, {by_term{ex, 1.f}}, by_doc_set{0}},
        Exclusion{mm, {}, by_doc_set{1}},
        Exclusion{a, {by_term{ex, 1.f}}, by_doc_set{1}},
        Exclusion{ph, {by_term{ex, 1.f}}, by_doc_set{0}},
        o,   // unrestricted, in the same batch
    };
    const auto prepared = prepare(filters, BM25{}, index);
    REQUIRE(prepared[0].doc_set == 0 && prepared[1].doc_set == 1 && prepared[4].doc_set == IRS_HIP_NO_DOC_SET);
    REQUIRE(prepared[0].terms.size() == 6 && prepared[0].terms[5].kind == IRS_HIP_EXCLUDE);
    const uint32_t k = 50;

    // a batch with a by_doc_set and no sets: refused; rows too short: illegal_argument
    {
      QueryBatch b({&seg}, prepared, k);
      bool threw = false;
      try { b.run(); } catch (const illegal_argument&) { threw = true; }
      REQUIRE(threw);
      threw = false;
      try { b.set_doc_sets(sets.data(), n_rows, p.num_docs / 64); } catch (const illegal_argument&) { threw = true; }
      REQUIRE(threw);
      threw = false;
      try { b.set_doc_sets(sets.data(), 1, n_words); } catch (const illegal_argument&) { threw = true; }   // row 1 >= n_rows
      REQUIRE(threw);
    }

    QueryBatch bh({&seg}, prepared, k);
    bh.set_doc_sets(sets.data(), n_rows, n_words);
    const QueryBatch::Results rh = bh.run().results();
    DeviceBuffer dsets(0, sets.size() * 8);
    check(irs_hip_device_upload(0, dsets.get(), sets.data(), sets.size() * 8), "upload");
    QueryBatch bd({&seg}, prepared, k);
    bd.set_doc_sets(dsets, n_rows, n_words);
    const QueryBatch::Results rd = bd.run().results();
    REQUIRE(rh.total_hits == rd.total_hits && rh.counts == rd.counts);
    REQUIRE(std::memcmp(rh.hits.data(), rd.hits.data(), rh.hits.size() * sizeof(irs_hip_hit)) == 0);
    {
      DeviceBuffer small(0, 64);
      bool threw = false;
      try { bd.set_doc_sets(small, n_rows, n_words); } catch (const illegal_argument&) { threw = true; }
      REQUIRE(threw);
    }
    const QueryBatch::DocSetStats st = bh.doc_set_stats();
    REQUIRE(st.tiles > 0 && st.tiles_skipped < st.tiles && st.leads == 0);
    // the range row leaves whole tiles empty at the smallest tile
    // (tile 4096: docs 9000..20999 lie in tiles 2..5 of 8)

    // the boolean queries against the oracle on the complement-masked segment
    const orc_scorer osc{ORC_SCORER_BM25, 1.2f, 0.75f, 0};
    struct Case { uint32_t q; std::vector<uint32_t> terms; int32_t op; uint32_t row; bool excluded; };
    const std::vector<Case> cases{{0, {1, 5, 12, 33, 70}, ORC_OP_OR, 0, true},
                                  {1, {1, 5, 12, 33, 70}, ORC_OP_MINMATCH | (2 << 8), 1, false},
                                  {2, {0, 3}, ORC_OP_AND, 1, true}};
    for (const Case& c : cases) {
      const std::vector<uint32_t> mask = mask_of(c.row, c.excluded);
      orc_segment v{};
      v.doc_file = static_cast<const uint8_t*>(d.doc_file);
      v.doc_file_len = doc_len;
      v.layout = ORC_LAYOUT_SIMD4;
      v.num_docs = p.num_docs;
      v.norms = static_cast<const uint8_t*>(d.norms);
      v.norm_width = 1;
      v.doc_mask = mask.data();
      v.doc_mask_count = mask.size();
      std::vector<orc_term_meta> metas(c.terms.size());
      std::vector<uint64_t> dwt;
      for (size_t i = 0; i < c.terms.size(); ++i) {
        std::memcpy(&metas[i], &d.terms[c.terms[i]], sizeof(orc_term_meta));
        dwt.push_back(d.terms[c.terms[i]].docs_count);
      }
      std::vector<float> scores(p.num_docs + 1);
      std::vector<uint8_t> matched(p.num_docs + 1, 0);
      REQUIRE(orc_score_all(&v, metas.data(), uint32_t(c.terms.size()), c.op, &osc, nullptr, dwf, dwt.data(), ttf,
                            scores.data(), matched.data()) >= 0);
      uint64_t n_match = 0;
      std::vector<float> best;
      for (uint32_t doc = 1; doc <= p.num_docs; ++doc)
        if (matched[doc]) {
          ++n_match;
          best.push_back(scores[doc]);
        }
      std::sort(best.rbegin(), best.rend());
      REQUIRE(n_match > 0 && rh.total(0, c.q) == n_match);
      const uint32_t n = rh.count(0, c.q);
      REQUIRE(n == std::min<uint64_t>(k, n_match));
      for (uint32_t i = 0; i < n; ++i) {
        const irs_hip_hit x = rh.of(0, c.q)[i];
        REQUIRE(matched[x.doc] && allowed(c.row, x.doc));
        REQUIRE(std::fabs(x.score - scores[x.doc]) <= 1e-5f * std::fabs(scores[x.doc]));
        REQUIRE(std::fabs(x.score - best[i]) <= 2e-5f * std::fabs(best[i]));   // rank i of the oracle's order
      }
    }
    // the phrase against the library's own run on the masked segment; the unrestricted query
    // against its run alone
    {
      const std::vector<uint32_t> mask = mask_of(0, true);
      irs_hip_segment_desc dm = d;
      dm.doc_mask = mask.data();
      dm.doc_mask_count = mask.size();
      SegmentReader masked(dm);
      QueryBatch bp({&masked}, prepare(std::vector<filter>{ph}, BM25{}, index), k);
      const QueryBatch::Results rp = bp.run().results();
      REQUIRE(rp.total(0, 0) == rh.total(0, 3) && rp.total(0, 0) > 0 && rp.count(0, 0) == rh.count(0, 3));
      REQUIRE(std::memcmp(rp.of(0, 0), rh.of(0, 3), rp.count(0, 0) * sizeof(irs_hip_hit)) == 0);
      QueryBatch bu({&seg}, prepare(std::vector<filter>{o}, BM25{}, index), k);
      const QueryBatch::Results ru = bu.run().results();
      REQUIRE(ru.total(0, 0) == rh.total(0, 4) && ru.count(0, 0) == rh.count(0, 4));
      for (uint32_t i = 0; i < ru.count(0, 0); ++i)
        REQUIRE(std::fabs(ru.of(0, 0)[i].score - rh.of(0, 4)[i].score) <= 1e-5f * ru.of(0, 0)[i].score);
    }
    // lead pieces, counted: the And and the phrase under the range row / every third doc
    {
      QueryBatch bc({&seg}, prepared, k);
      bc.set_doc_sets(sets.data(), n_rows, n_words).count_work(true);
      const QueryBatch::Results rc = bc.run().results();
      REQUIRE(rc.total_hits == rh.total_hits);
      const QueryBatch::DocSetStats sc = bc.doc_set_stats();
      REQUIRE(sc.leads > 0 && sc.leads_skipped > 0 && sc.leads_skipped < sc.leads && sc.tiles == st.tiles);
    }
    // cleared: the batch no longer holds what its by_doc_set queries name — run() refuses
    bh.set_doc_sets(static_cast<const uint64_t*>(nullptr), 0, 0);
    {
      bool threw = false;
      try { bh.run(); } catch (const illegal_argument&) { threw = true; }
      REQUIRE(threw);
    }
    // ... and a batch without by_doc_set queries is what it was: sets given and cleared again
    {
      const auto plain = prepare(std::vector<filter>{o, mm}, BM25{}, index);
      QueryBatch bu({&seg}, plain, k);
      const QueryBatch::Results r0 = bu.run().results();
      bu.set_doc_sets(sets.data(), n_rows, n_words);   // (no query names a row: nothing is restricted)
      const QueryBatch::Results r1 = bu.run().results();
      bu.set_doc_sets(static_cast<const uint64_t*>(nullptr), 0, 0);
      const QueryBatch::Results r2 = bu.run().results();
      REQUIRE(r0.total_hits == r1.total_hits && r0.total_hits == r2.total_hits);
      REQUIRE(std::memcmp(r0.hits.data(), r2.hits.data(), r0.hits.size() * sizeof(irs_hip_hit)) == 0);
    }
    std::printf("test_doc_sets OK: totals %llu %llu %llu %llu, tiles %llu skipped %llu\n",
                (unsigned long long)rh.total(0, 0), (unsigned long long)rh.total(0, 1),
                (unsigned long long)rh.total(0, 2), (unsigned long long)rh.total(0, 3),
                (unsigned long long)st.tiles, (unsigned long long)st.tiles_skipped);
  }
  irs_synth_free(idx);
  return 0;
}
