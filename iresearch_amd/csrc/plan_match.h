// plan_match.h — host side of unscored execution (match.h): the units' records, built from the
// batch's query records the first time match sets are asked for, and the launches.
// Included by irs_hip.hip (one translation unit).
#pragma once

namespace {

// (irs_hip.hip: the deal of a batch's units; the plan stage's launch of k_excl_mask)
bool ensure_scratch(irs_hip_batch* b);
bool launch_excl_masks(irs_hip_batch* b, rt::stream_t st);

// MatchUnit records of every unit, from what create left in b->queries / b->qterms: query_run of
// DevQuery::op tells doc tiles (Or), doc tiles with match counters (min-match, its query_need) or a
// conjunction; a grouped one has its groups' first rows in AnyWork::opens
static int build_match_work(irs_hip_batch* b) {
  MatchWork& m = b->match;
  if (m.built) return IRS_HIP_OK;
  std::vector<uint8_t> grouped(b->nq, 0);
  for (uint32_t u : b->any.units) grouped[u] = 1;
  m.units.clear();
  m.rows.clear();
  m.maps = 1;
  m.max_docs = 0;
  for (const irs_hip_segment* sg : b->segs) m.max_docs = std::max(m.max_docs, sg->dev.num_docs);
  if (b->phrase) {   // (phrase units run on the lead-item tables of the scored path)
    m.built = true;
    return IRS_HIP_OK;
  }
  for (uint32_t q = 0; q < b->nq; ++q) {
    const DevQuery& dq = b->queries[q];
    MatchUnit mu{};
    mu.dead = dq.dead;
    mu.seg = dq.seg;
    mu.first = uint32_t(m.rows.size());
    mu.n_rows = dq.n_terms;
    if (query_run(dq.op) == kRunConj) {
      mu.op = kMatchAnd;
      mu.opens = grouped[q] ? b->any.opens[q] : (1u << dq.n_terms) - 1u;
    } else if (query_run(dq.op) == kRunCount) {
      mu.op = kMatchMin;
      mu.need = query_need(dq.op);
    } else {
      mu.op = kMatchOr;
    }
    if (mu.n_rows > kMaxTerms) return IRS_HIP_EUNSUPPORTED;
    for (uint32_t j = 0; j < dq.n_terms; ++j) m.rows.push_back(b->qterms[dq.first_term + j].term);
    if (mu.n_rows) m.maps = std::max(m.maps, match_maps(mu.op));
    m.units.push_back(mu);
  }
  if (m.rows.empty()) m.rows.push_back(0);
  m.slice_words = b->knobs.match_slice;
  while (m.slice_words > 64u && uint64_t(m.maps) * m.slice_words * 4u + kMatchLdsExtra > kMatchLdsBytes) m.slice_words >>= 1;
  if (!m.d_units.alloc(m.units.size() * sizeof(MatchUnit)) || !m.d_rows.alloc(m.rows.size() * 4))
    return IRS_HIP_ENOMEM;
  m.built = true;
  m.sent = false;
  return IRS_HIP_OK;
}

// by_phrase units: the plan tables and lead-item records of a scored run (k_plan, k_conj_seek /
// k_vphrase_seek: the same words every run writes), then the match-only kernels over every lead
// item.  No pilot pass, no threshold, no candidates.
template<int LAYOUT>
static bool launch_phrase_match(irs_hip_batch* b, rt::stream_t st, uint32_t* sets32, uint64_t words32,
                                unsigned long long* counts) {
  BlockWork& w = b->blocks;
  if (w.n_phrase_wgs == 0) return true;   // no query has all its terms in its segment
  RT_LAUNCH(k_plan, b->nq * b->jt, kThreads, 0, st, b->d_segs.as<DevSegment>(),
            b->d_queries.as<DevQuery>(), b->d_qterms.as<DevQTerm>(), b->jt, b->tiles.docs,
            b->d_first.as<uint32_t>(), b->d_tails.as<DevTail>());
  ConjArgs a = block_args(b, w, 1u);
  a.touched = nullptr;
  if (w.variadic) {
    RT_LAUNCH(k_vphrase_seek, (w.n_items + kThreads - 1) / kThreads, kThreads, 0, st,
              b->d_segs.as<DevSegment>(), b->d_queries.as<DevQuery>(), b->d_tails.as<DevTail>(), b->jt,
              w.d_units.as<uint32_t>(), w.d_item_base.as<uint32_t>(), uint32_t(w.units.size()),
              w.d_lead_rows.as<uint32_t>(), w.d_seek.as<uint32_t>(), w.d_recs.as<ConjItem>());
    RT_LAUNCH(k_vphrase_match<LAYOUT>, w.n_phrase_wgs, kPhraseWaves * 64, 0, st, a,
              w.d_opens.as<uint32_t>(), sets32, words32, counts);
    return rt::last_error_ok();
  }
  if (w.disj) {   // (a batch with several phrases in one Or: every unit on k_phrases_or_match)
    RT_LAUNCH(k_phrases_or_seek, (w.n_items + kThreads - 1) / kThreads, kThreads, 0, st,
              b->d_segs.as<DevSegment>(), b->d_queries.as<DevQuery>(), b->d_tails.as<DevTail>(), b->jt,
              w.d_units.as<uint32_t>(), w.d_item_base.as<uint32_t>(), uint32_t(w.units.size()),
              w.d_lead_rows.as<uint32_t>(), w.d_seek.as<uint32_t>(), w.d_recs.as<ConjItem>());
    if (b->jt <= 4) {
      RT_LAUNCH((k_phrases_or_match<LAYOUT, 4>), w.n_phrase_wgs, kPhraseWaves * 64, 0, st, a,
                w.d_opens.as<uint32_t>(), sets32, words32, counts);
    } else {
      RT_LAUNCH((k_phrases_or_match<LAYOUT, int(kPhraseMaxTerms)>), w.n_phrase_wgs, kPhraseWaves * 64, 0, st, a,
                w.d_opens.as<uint32_t>(), sets32, words32, counts);
    }
    return rt::last_error_ok();
  }
  a.lead_of = w.d_lead_of.as<uint32_t>();
  RT_LAUNCH(k_conj_seek, (w.n_items + kThreads - 1) / kThreads, kThreads, 0, st,
            b->d_segs.as<DevSegment>(), b->d_queries.as<DevQuery>(), b->d_tails.as<DevTail>(), b->jt,
            w.d_units.as<uint32_t>(), w.d_item_base.as<uint32_t>(), uint32_t(w.units.size()),
            w.d_lead_of.as<uint32_t>(), static_cast<const uint32_t*>(nullptr), w.d_seek.as<uint32_t>(),
            w.d_recs.as<ConjItem>());
  if (w.several) {   // (a batch with several phrases in one And: every unit on k_phrases_and_match)
    if (b->jt <= 4) {
      RT_LAUNCH((k_phrases_and_match<LAYOUT, 4>), w.n_phrase_wgs, kPhraseWaves * 64, 0, st, a,
                w.d_n_phrase.as<uint32_t>(), w.d_opens.as<uint32_t>(), sets32, words32, counts);
    } else {
      RT_LAUNCH((k_phrases_and_match<LAYOUT, int(kPhraseMaxTerms)>), w.n_phrase_wgs, kPhraseWaves * 64, 0, st, a,
                w.d_n_phrase.as<uint32_t>(), w.d_opens.as<uint32_t>(), sets32, words32, counts);
    }
    return rt::last_error_ok();
  }
  if (w.required) {   // (a batch with required terms: every unit on the REQ form)
    if (b->jt <= 4) {
      RT_LAUNCH((k_phrase_and_match<LAYOUT, 4>), w.n_phrase_wgs, kPhraseWaves * 64, 0, st, a,
                w.d_n_phrase.as<uint32_t>(), sets32, words32, counts);
    } else {
      RT_LAUNCH((k_phrase_and_match<LAYOUT, int(kPhraseMaxTerms)>), w.n_phrase_wgs, kPhraseWaves * 64, 0, st, a,
                w.d_n_phrase.as<uint32_t>(), sets32, words32, counts);
    }
    return rt::last_error_ok();
  }
  if (w.optional) {   // (a batch with optional terms: the words' rows only, OR-ed into the term pass's sets)
    if (b->jt <= 4) {
      RT_LAUNCH((k_phrase_or_match<LAYOUT, 4>), w.n_phrase_wgs, kPhraseWaves * 64, 0, st, a,
                w.d_n_phrase.as<uint32_t>(), sets32, words32);
    } else {
      RT_LAUNCH((k_phrase_or_match<LAYOUT, int(kPhraseMaxTerms)>), w.n_phrase_wgs, kPhraseWaves * 64, 0, st, a,
                w.d_n_phrase.as<uint32_t>(), sets32, words32);
    }
    return rt::last_error_ok();
  }
  if (b->jt <= 2) {
    RT_LAUNCH((k_phrase_match<LAYOUT, 2>), w.n_phrase_wgs, kPhraseWaves * 64, 0, st, a, sets32, words32, counts);
  } else if (b->jt <= 4) {
    RT_LAUNCH((k_phrase_match<LAYOUT, 4>), w.n_phrase_wgs, kPhraseWaves * 64, 0, st, a, sets32, words32, counts);
  } else {
    RT_LAUNCH((k_phrase_match<LAYOUT, int(kPhraseMaxTerms)>), w.n_phrase_wgs, kPhraseWaves * 64, 0, st, a,
              sets32, words32, counts);
  }
  return rt::last_error_ok();
}

// irs_hip_batch_match_sets (sets / counts: host memory, synchronous) and _to_device (d_sets /
// d_counts: device memory, queued on `st`).  Reads the segments, the batch's exclusion masks
// (rebuilt here: the same words every plan stage writes) and tables of its own — nothing a run
// leaves behind, nothing a run reads is changed.
static int batch_match_sets_impl(irs_hip_batch* b, uint64_t* sets, void* d_sets, uint64_t n_words,
                                 uint64_t* counts, void* d_counts, rt::stream_t st, bool to_device) {
  if (!b) return IRS_HIP_EINVAL;
  const bool want_sets = to_device ? d_sets != nullptr : sets != nullptr;
  const bool want_counts = to_device ? d_counts != nullptr : counts != nullptr;
  if (!want_sets && !want_counts) return IRS_HIP_EINVAL;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  if (const int rc = build_match_work(b)) return rc;
  MatchWork& m = b->match;
  // (a phrase batch: the units' records, plan tables and lead items are those of its runs)
  if (b->phrase && !ensure_scratch(b)) return IRS_HIP_ENOMEM;
  // every doc of the largest segment has a bit: 64 * n_words > num_docs
  if (n_words == 0 || n_words > 0x4000000ull || 64u * n_words <= uint64_t(m.max_docs)) return IRS_HIP_EINVAL;
  const uint32_t slices = b->phrase ? 0u : uint32_t((2u * n_words + m.slice_words - 1u) / m.slice_words);
  if (uint64_t(slices) * b->nq > 0x7FFFFFFFull) return IRS_HIP_EUNSUPPORTED;
  const size_t set_bytes = size_t(b->nq) * n_words * 8u, count_bytes = size_t(b->nq) * 8u;
  if (!to_device) {
    if ((want_sets && !m.d_sets.alloc(set_bytes)) || (want_counts && !m.d_counts.alloc(count_bytes)))
      return IRS_HIP_ENOMEM;
    d_sets = want_sets ? m.d_sets.p : nullptr;
    d_counts = want_counts ? m.d_counts.p : nullptr;
  }
  // (optional terms: the counts are those of the united rows, so the rows are made either way)
  const bool own_rows = b->opt && !d_sets;
  if (own_rows) {
    if (!m.d_sets.alloc(set_bytes)) return IRS_HIP_ENOMEM;
    d_sets = m.d_sets.p;
  }
  // behind the batch's own queued work — a run or a plan stage writes the masks and may have the
  // batch's tables in flight, an earlier call on another stream reads this one's tables
  bool ok = match_get_behind(b, st) && b->up.flush(st);   // (the segments' records and the masks' tables, staged since create)
  if (ok && !b->phrase && !m.sent) {
    ok = rt::h2d(m.d_units.p, m.units.data(), m.units.size() * sizeof(MatchUnit), st) &&
         rt::h2d(m.d_rows.p, m.rows.data(), m.rows.size() * 4, st);
    m.sent = ok;
  }
  if (ok && b->excl.on()) ok = launch_excl_masks(b, st);
  if (ok && want_counts) ok = rt::dmemset(d_counts, 0, count_bytes, st);
  if (ok && b->opt) {
    // the term pass's rows first — its doc sets all ones, or what a run left: the docs missing from
    // them are docs of the phrase — every word of every row written; the phrase's docs OR-ed in,
    // the united rows counted
    if (!b->ran) ok = rt::dmemset(b->d_taken.p, 0xFF, b->d_taken.n, st);
    ok = ok && batch_match_sets_impl(b->opt, nullptr, d_sets, n_words, nullptr, nullptr, st, true) == IRS_HIP_OK &&
         with_layout(b->seg->dev.layout, [&](auto L) {
           return launch_phrase_match<decltype(L)::value>(b, st, static_cast<uint32_t*>(d_sets), 2u * n_words, nullptr);
         });
    if (ok && want_counts) {
      const uint32_t cs = uint32_t((2u * n_words + 8u * kThreads - 1u) / (8u * kThreads));
      RT_LAUNCH(k_count_rows, cs * b->nq, kThreads, 0, st, static_cast<const uint32_t*>(d_sets), 2u * n_words, cs,
                static_cast<unsigned long long*>(d_counts));
      ok = rt::last_error_ok();
    }
  } else if (ok && b->phrase) {
    ok = (!want_sets || rt::dmemset(d_sets, 0, set_bytes, st)) &&
         with_layout(b->seg->dev.layout, [&](auto L) {
           return launch_phrase_match<decltype(L)::value>(b, st, static_cast<uint32_t*>(d_sets), 2u * n_words,
                                                          static_cast<unsigned long long*>(d_counts));
         });
  } else if (ok) {
    const size_t smem = size_t(m.maps) * m.slice_words * 4u + kMatchLdsExtra;
    ok = with_layout(b->seg->dev.layout, [&](auto L) {
      if (!big_smem(k_match_slice<decltype(L)::value>, smem)) return false;
      RT_LAUNCH((k_match_slice<decltype(L)::value>), slices * b->nq, kThreads, smem, st,
                b->d_segs.as<DevSegment>(), m.d_units.as<MatchUnit>(), m.d_rows.as<uint32_t>(), slices,
                m.slice_words, static_cast<uint32_t*>(d_sets), n_words,
                static_cast<unsigned long long*>(d_counts));
      return rt::last_error_ok();
    });
  }
  if (!ok) {
    if (!to_device) m.d_sets.release();
    return IRS_HIP_EHIP;
  }
  if (to_device && own_rows) {   // (the rows were scratch: nothing queued may outlive the block)
    const bool synced = rt::sync(st);
    m.d_sets.release();
    return synced ? IRS_HIP_OK : IRS_HIP_EHIP;
  }
  if (to_device) {
    // (a later run, setter or destroy gets behind this: the masks and the tables are still read)
    return b->sync.matched.mark(st) ? IRS_HIP_OK : IRS_HIP_EHIP;
  }
  const bool copied = (!want_sets || rt::d2h(sets, d_sets, set_bytes, st)) &&
                      (!want_counts || rt::d2h(counts, d_counts, count_bytes, st));
  const bool synced = rt::sync(st);   // (also after a failed copy: nothing queued may outlive the block)
  m.d_sets.release();   // (units x docs / 8 bytes: back to the pool, not kept for the batch's life)
  return copied && synced ? IRS_HIP_OK : IRS_HIP_EHIP;
}

}  // namespace
