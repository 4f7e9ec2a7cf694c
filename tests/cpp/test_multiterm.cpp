// tests/cpp/test_multiterm.cpp — TEST: the C++ host layer's scored multi-term filter
// (by_scored_terms: irs::by_terms with scorers, IRS_HIP_OP_MULTITERM) and the scored expansion
// helper beyond 16 scored states, against the oracle's C API; what the layer refuses.  Linked
// against libirs_hip.so on a GPU box, or against the CPU emulator build of the same sources.
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

  Segment(uint32_t docs, uint64_t first_doc, uint32_t max_rank) : num_docs{docs} {
    irs_synth_params p{};
    p.seed = 20260926;
    p.first_doc = first_doc;
    p.num_docs = docs;
    p.vocab_log2 = 20;
    p.max_rank = max_rank;
    p.layout = IRS_SYNTH_LAYOUT_SIMD4;
    p.mean_len = 100;
    p.stddev_len = 30;
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
    reader = std::make_unique<SegmentReader>(d);
  }
  ~Segment() {
    reader.reset();
    irs_synth_free(idx);
  }
  SegmentStats stats() const {
    return SegmentStats{irs_synth_docs_with_field(idx), irs_synth_total_term_freq(idx), metas,
                        num_terms};
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

bool close_rel(float a, float b) { return std::fabs(a - b) <= 1e-5f * std::fabs(b); }

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

}  // namespace

int main() {
  constexpr uint32_t kMaxRank = 128, kTop = 50;
  Segment a(20000, 0, kMaxRank), b(9000, 20000, kMaxRank);
  const Segment* segs[2] = {&a, &b};
  const BM25 scorer;
  const std::vector<SegmentStats> index{a.stats(), b.stats()};

  // a 40-term filter with boosts and min_match 3, one of 17 terms matching any, and an ordinary Or
  by_scored_terms forty;
  forty.min_match = 3;
  forty.boost = 1.5f;
  for (uint32_t t = 0; t < 40; ++t) forty.terms.push_back(by_term{5 + 3 * t, 0.25f * float(1 + t % 8)});
  forty.terms[7].term = kMaxRank + 500;   // no such term: counts for nothing
  by_scored_terms seventeen;
  for (uint32_t t = 0; t < 17; ++t) seventeen.terms.push_back(by_term{60 + t});
  std::vector<filter> filters{forty, seventeen, Or{{by_term{2}, by_term{9}, by_term{30}}}};
  const auto prepared = prepare(filters, scorer, index);
  REQUIRE(prepared[0].op == IRS_HIP_OP_MULTITERM && prepared[0].min_match == 3 && prepared[0].terms.size() == 40);
  REQUIRE(prepared[1].op == IRS_HIP_OP_MULTITERM && prepared[1].min_match == 1);
  QueryBatch batch({a.reader.get(), b.reader.get()}, prepared, kTop);
  REQUIRE(batch.wide_units() == 4);
  const auto res = batch.run().results();
  const auto top = merge(res);

  const orc_segment views[2] = {a.oracle_view(), b.oracle_view()};
  const uint64_t dwf[2] = {a.stats().docs_with_field, b.stats().docs_with_field};
  const uint64_t ttf[2] = {a.stats().total_term_freq, b.stats().total_term_freq};
  const orc_scorer osc{ORC_SCORER_BM25, scorer.k(), scorer.b(), 0};
  for (size_t q = 0; q < filters.size(); ++q) {
    const PreparedQuery& p = prepared[q];
    const uint32_t n = uint32_t(p.terms.size());
    std::vector<orc_term_meta> metas(2 * n);
    std::vector<float> boosts(n, 1.f);
    for (uint32_t s = 0; s < 2; ++s)
      for (uint32_t t = 0; t < n; ++t)
        if (p.terms[t].term < segs[s]->num_terms)
          std::memcpy(&metas[s * n + t], &segs[s]->metas[p.terms[t].term], sizeof(orc_term_meta));
    if (q == 0)
      for (uint32_t t = 0; t < n; ++t) boosts[t] = forty.boost * forty.terms[t].boost;
    const int32_t op = p.min_match > 1 ? (ORC_OP_MINMATCH | int32_t(p.min_match << 8)) : ORC_OP_OR;
    std::vector<orc_hit> want(kTop);
    uint64_t want_total = 0;
    const int64_t got_n = orc_search(views, 2, metas.data(), n, op, &osc, boosts.data(), dwf, ttf, kTop,
                                     want.data(), &want_total);
    REQUIRE(got_n >= 0);
    want.resize(size_t(got_n));
    REQUIRE(res.total(0, uint32_t(q)) + res.total(1, uint32_t(q)) == want_total);
    REQUIRE(want_total > kTop);
    REQUIRE(top[q].size() == want.size());
    std::sort(want.begin(), want.end(), [](const orc_hit& x, const orc_hit& y) { return x.score > y.score; });
    for (size_t i = 0; i < want.size(); ++i) REQUIRE(close_rel(top[q][i].score, want[i].score));
  }

  // the scored expansion helper: 30 scored states go out as one multi-term query, 16 as an Or
  {
    uint32_t checked = 0;
    std::vector<std::vector<uint32_t>> visits(2);
    for (uint32_t t = 20; t < 120; ++t) {
      visits[0].push_back(t);
      if (t % 3) visits[1].push_back(t);
    }
    const PreparedExpansion wide = prepare_expansion(visits, 30, scorer, index);
    const PreparedExpansion narrow = prepare_expansion(visits, 16, scorer, index);
    REQUIRE(wide.scored.op == IRS_HIP_OP_MULTITERM && wide.scored.min_match == 1);
    REQUIRE(wide.scored.terms.size() > 16 && wide.scored.terms.size() <= 30);
    REQUIRE(narrow.scored.op == IRS_HIP_OP_OR && narrow.scored.terms.size() <= 16);
    REQUIRE(throws<not_supported>([&] { prepare_expansion(visits, 65, scorer, index); }));
    const auto r = execute_expansions({a.reader.get(), b.reader.get()}, {a.num_docs, b.num_docs},
                                      {wide, narrow}, kTop);
    // every visited term's docs match; the scored part of a segment is the oracle's disjunction of
    // the terms scored there, with the statistics of the segments where they are scored
    for (uint32_t s = 0; s < 2; ++s) {
      const auto& sc = wide.scored_in[s];
      if (sc.empty()) {   // (the longest lists are the larger segment's: nothing scores here)
        for (uint32_t i = 0; i < r.count(s, 0); ++i) REQUIRE(r.of(s, 0)[i].score == 0.f);
        continue;
      }
      std::vector<orc_term_meta> metas(sc.size());
      std::vector<uint64_t> dwt(sc.size(), 0);
      for (size_t j = 0; j < sc.size(); ++j) {
        std::memcpy(&metas[j], &segs[s]->metas[sc[j]], sizeof(orc_term_meta));
        for (uint32_t o = 0; o < 2; ++o)
          if (std::binary_search(wide.scored_in[o].begin(), wide.scored_in[o].end(), sc[j]))
            dwt[j] += segs[o]->metas[sc[j]].docs_count;
      }
      std::vector<float> scores(size_t(segs[s]->num_docs) + 1);
      std::vector<uint8_t> matched(scores.size());
      REQUIRE(orc_score_all(&views[s], metas.data(), uint32_t(sc.size()), ORC_OP_OR, &osc, nullptr,
                            dwf[0] + dwf[1], dwt.data(), ttf[0] + ttf[1], scores.data(), matched.data()) >= 0);
      REQUIRE(r.count(s, 0) == kTop && r.total(s, 0) >= r.count(s, 0));
      ++checked;
      for (uint32_t i = 0; i < r.count(s, 0); ++i) {
        const irs_hip_hit h = r.of(s, 0)[i];
        REQUIRE(h.doc <= segs[s]->num_docs && matched[h.doc] && close_rel(h.score, scores[h.doc]));
        REQUIRE(i == 0 || r.of(s, 0)[i - 1].score >= h.score);
      }
    }
    REQUIRE(checked >= 1);
  }

  // what the layer and the ABI refuse
  {
    by_scored_terms many;
    for (uint32_t t = 0; t < 65; ++t) many.terms.push_back(by_term{t});
    REQUIRE(throws<not_supported>([&] { prepare({filter{many}}, scorer, index); }));
    by_scored_terms none;
    REQUIRE(throws<illegal_argument>([&] { prepare({filter{none}}, scorer, index); }));
    by_scored_terms bad = seventeen;
    bad.min_match = 0;
    REQUIRE(throws<illegal_argument>([&] { prepare({filter{bad}}, scorer, index); }));
    bad.min_match = 18;
    REQUIRE(throws<illegal_argument>([&] { prepare({filter{bad}}, scorer, index); }));
    // MAX merge and an excluded entry on such a query: refused by batch create
    auto one = prepare({filter{seventeen}}, scorer, index);
    one[0].merge = IRS_HIP_MERGE_MAX;
    REQUIRE(throws<not_supported>([&] { QueryBatch({a.reader.get()}, one, kTop); }));
    one[0].merge = IRS_HIP_MERGE_SUM;
    irs_hip_term_scorer e{};
    e.term = 3;
    e.kind = IRS_HIP_EXCLUDE;
    one[0].terms.push_back(e);
    REQUIRE(throws<not_supported>([&] { QueryBatch({a.reader.get()}, one, kTop); }));
    // an Or of 17 by_terms stays what it was
    Or wide_or;
    for (uint32_t t = 0; t < 17; ++t) wide_or.subs.push_back(by_term{t});
    const auto seventeen_or = prepare({filter{wide_or}}, scorer, index);
    REQUIRE(throws<illegal_argument>([&] { QueryBatch({a.reader.get()}, seventeen_or, kTop); }));
    // match sets of a batch with such a query
    QueryBatch mb({a.reader.get()}, prepare({filter{seventeen}}, scorer, index), kTop);
    REQUIRE(throws<not_supported>([&] { mb.match_sets((uint64_t(a.num_docs) + 64) / 64); }));
  }
  std::printf("test_multiterm OK\n");
  return 0;
}
