// plan_blocks.h — host half of the block-driven units (conj.h conjunctions, phrase.h phrases): the
// lead-item work lists, the pilot pass's sample of them, the k_conj / k_phrase launches.
// Included by irs_hip.hip (one translation unit).
#pragma once

namespace {

// The rows of the seek table — the lead items of w.units, unit after unit — and the tables of
// the block-driven kernels; `per_unit` goes to `d_per_unit` (a conjunction's lead-block cut /
// a phrase's lead term / a variadic phrase's or grouped conjunction's lead rows).  w: b->blocks,
// or b->any (grouped conjunctions, plan_any.h)
int stage_lead_items(irs_hip_batch* b, BlockWork& w, DevBuf& d_per_unit, const std::vector<uint32_t>& per_unit) {
  const uint32_t nq = b->nq;
  std::vector<uint32_t> item_base(w.units.size() + 1, 0), unit_items(nq, 0);
  uint64_t total = 0;
  for (size_t c = 0; c < w.units.size(); ++c) {
    item_base[c] = uint32_t(total);
    unit_items[w.units[c]] = uint32_t(total);
    total += w.items[c];
  }
  if (total > 0x7FFFFFFFull) return IRS_HIP_EUNSUPPORTED;
  item_base[w.units.size()] = uint32_t(total);
  w.n_items = uint32_t(total);
  if (!w.d_item_base.alloc(item_base.size() * 4) ||
      !w.d_unit_items.alloc(unit_items.size() * 4) ||
      !w.d_seek.alloc((total + 2) * uint64_t(kMaxTerms) * 4) ||
      !w.d_recs.alloc((total + 1) * sizeof(ConjItem)) ||
      !w.d_item_hits.alloc((total + 1) * 4) ||
      !w.d_units.alloc(w.units.size() * 4) ||
      !w.d_items.alloc(w.items.size() * 4) ||
      !d_per_unit.alloc(per_unit.size() * 4) ||
      !w.d_hist.alloc(uint64_t(nq) * kBins * 4))
    return IRS_HIP_ENOMEM;
  if (!b->up.copy(w.d_item_base.p, item_base.data(), item_base.size() * 4) ||
      !b->up.copy(w.d_unit_items.p, unit_items.data(), unit_items.size() * 4) ||
      !b->up.copy(w.d_units.p, w.units.data(), w.units.size() * 4) ||
      !b->up.copy(w.d_items.p, w.items.data(), w.items.size() * 4) ||
      !b->up.copy(d_per_unit.p, per_unit.data(), per_unit.size() * 4))
    return IRS_HIP_ENOMEM;
  return IRS_HIP_OK;
}

// The lead-group planning of k_vphrase (variadic phrases) and k_conj_any (grouped conjunctions,
// conj_any.h) over the units `cand` (those without rows are skipped): the iteration lead of a unit
// is the part / group with the smallest sum of its members' docs_count (a disjunction costs the sum
// of its members, Conjunction sorts by cost; the first such one on ties); one wavefront per block
// (+ tail) of every member of it.  The pilot pass samples those items like any others.  w.opens
// holds every unit's `opens` word; w.d_lead_rows gets lead rows lo | end << 8.
int build_lead_groups(irs_hip_batch* b, BlockWork& w, const std::vector<uint32_t>& cand) {
  std::vector<uint32_t> lead_rows(b->nq, 0);
  for (uint32_t u : cand) {
    const DevQuery& dq = b->queries[u];
    if (!dq.n_terms) continue;
    const irs_hip_segment* sg = b->segs[dq.seg];
    const uint32_t opens = w.opens[u] | 1u;
    uint64_t best = ~uint64_t(0);
    uint32_t items = 0;
    for (uint32_t lo = 0; lo < dq.n_terms;) {
      uint32_t end = lo + 1;
      while (end < dq.n_terms && !((opens >> end) & 1u)) ++end;
      uint64_t cost = 0;
      uint32_t k = 0;
      for (uint32_t r = lo; r < end; ++r) {
        const DevTerm& t = sg->terms[b->qterms[dq.first_term + r].term];
        cost += t.docs_count;
        k += t.nblk + ((t.docs_count == 1 || t.tail_n) ? 1u : 0u);
      }
      if (cost < best) {
        best = cost;
        items = k;
        lead_rows[u] = lo | (end << 8);
      }
      lo = end;
    }
    w.units.push_back(u);
    w.items.push_back(items);
  }
  if (w.units.empty()) return IRS_HIP_OK;
  if (!w.d_opens.alloc(uint64_t(b->nq) * 4) ||
      !b->up.copy(w.d_opens.p, w.opens.data(), uint64_t(b->nq) * 4))
    return IRS_HIP_ENOMEM;
  return stage_lead_items(b, w, w.d_lead_rows, lead_rows);
}

// k_vphrase work (vphrase.h) of a batch with variadic phrases: every unit of it
int build_vphrase_work(irs_hip_batch* b) {
  std::vector<uint32_t> all(b->nq);
  for (uint32_t u = 0; u < b->nq; ++u) all[u] = u;
  const int rc = build_lead_groups(b, b->blocks, all);
  if (b->blocks.units.empty()) return rc;
  b->blocks.n_phrase_wgs = (b->blocks.n_items + kPhraseWaves - 1) / kPhraseWaves;
  return rc;
}

// k_phrases_or work (phrases_or.h) of a batch with several phrases in one Or: EVERY present phrase of
// a unit leads with its own rarest row (the first such one on ties); the unit's lead items are the
// blocks (+ tail / single doc) of each phrase's lead row, phrase after phrase.  The lead rows are
// not contiguous: d_lead_rows carries them as a mask (bit r = row r leads its phrase), which
// k_phrases_or_seek turns into records and seek rows; d_opens says which rows open a phrase.
int build_phrases_or_work(irs_hip_batch* b) {
  BlockWork& w = b->blocks;
  std::vector<uint32_t> lead_mask(b->nq, 0);
  for (uint32_t u = 0; u < b->nq; ++u) {
    const DevQuery& dq = b->queries[u];
    if (!dq.n_terms) continue;
    const irs_hip_segment* sg = b->segs[dq.seg];
    const uint32_t opens = w.phrase_opens[u] | 1u;
    uint32_t items = 0;
    for (uint32_t lo = 0; lo < dq.n_terms;) {
      uint32_t end = lo + 1;
      while (end < dq.n_terms && !((opens >> end) & 1u)) ++end;
      uint32_t best = 0xFFFFFFFFu, lead = lo, k = 0;
      for (uint32_t r = lo; r < end; ++r) {
        const DevTerm& t = sg->terms[b->qterms[dq.first_term + r].term];
        if (t.docs_count < best) {
          best = t.docs_count;
          k = t.nblk + ((t.docs_count == 1 || t.tail_n) ? 1u : 0u);
          lead = r;
        }
      }
      lead_mask[u] |= 1u << lead;
      items += k;
      lo = end;
    }
    w.units.push_back(u);
    w.items.push_back(items);
  }
  if (w.units.empty()) return IRS_HIP_OK;   // (no query has a phrase with all its words in its segment)
  if (!w.d_opens.alloc(uint64_t(b->nq) * 4) || !b->up.copy(w.d_opens.p, w.phrase_opens.data(), uint64_t(b->nq) * 4))
    return IRS_HIP_ENOMEM;
  const int rc = stage_lead_items(b, w, w.d_lead_rows, lead_mask);
  w.n_phrase_wgs = (w.n_items + kPhraseWaves - 1) / kPhraseWaves;
  return rc;
}

// k_phrase work of a phrase batch, built at create: the lead term of a unit is its rarest one; one
// wavefront per 128-posting block of it (+ one for its vint tail / single doc); records and start
// blocks of the other terms written by k_conj_seek every run
int build_phrase_work(irs_hip_batch* b) {
  if (b->blocks.variadic) return build_vphrase_work(b);
  if (b->blocks.disj) return build_phrases_or_work(b);
  std::vector<uint32_t> lead_of(b->nq, 0);
  for (uint32_t u = 0; u < b->nq; ++u) {
    const DevQuery& dq = b->queries[u];
    if (!dq.n_terms) continue;
    const irs_hip_segment* sg = b->segs[dq.seg];
    uint32_t best = 0xFFFFFFFFu, items = 0;
    // (optional terms never lead: the rarest of the phrase's words)
    const uint32_t n_lead = b->blocks.optional ? b->blocks.n_phrase[u] : dq.n_terms;
    for (uint32_t j = 0; j < n_lead; ++j) {
      const DevTerm& t = sg->terms[b->qterms[dq.first_term + j].term];
      if (t.docs_count < best) {
        best = t.docs_count;
        items = t.nblk + ((t.docs_count == 1 || t.tail_n) ? 1u : 0u);
        lead_of[u] = j;
      }
    }
    // (the lists of the pilot pass: same bookkeeping as for conjunctions)
    b->blocks.units.push_back(u);
    b->blocks.items.push_back(items);
  }
  if (b->blocks.units.empty()) return IRS_HIP_OK;   // (no query has all its terms in its segment)
  const int rc = stage_lead_items(b, b->blocks, b->blocks.d_lead_of, lead_of);
  b->blocks.n_phrase_wgs = (b->blocks.n_items + kPhraseWaves - 1) / kPhraseWaves;
  // (required terms: the lead above is the rarest of the phrase words AND the required terms)
  if (rc == IRS_HIP_OK && (b->blocks.required || b->blocks.optional || b->blocks.several) &&
      (!b->blocks.d_n_phrase.alloc(uint64_t(b->nq) * 4) ||
       !b->up.copy(b->blocks.d_n_phrase.p, b->blocks.n_phrase.data(), uint64_t(b->nq) * 4)))
    return IRS_HIP_ENOMEM;
  // (several phrases in one And: ... and which rows open a phrase)
  if (rc == IRS_HIP_OK && b->blocks.several &&
      (!b->blocks.d_opens.alloc(uint64_t(b->nq) * 4) ||
       !b->up.copy(b->blocks.d_opens.p, b->blocks.phrase_opens.data(), uint64_t(b->nq) * 4)))
    return IRS_HIP_ENOMEM;
  return rc;
}

// k_conj work of the batch's block-driven conjunctions (blocks.units): the lead term of a unit is
// its first one (sorted by cost at create); one wavefront per 128-posting block of it (+ one for
// its vint tail / single doc), its record and the other terms' start blocks written by
// k_conj_seek every run.  Rebuilt whenever ensure_scratch deals the conjunctions anew.
int build_conj_work(irs_hip_batch* b) {
  int rc = IRS_HIP_OK;
  b->blocks.items.clear();
  b->blocks.n_items = 0;
  b->blocks.n_wgs = 0;
  b->blocks.n_pilot = 0;
  b->blocks.pilot_stride = 0;
  if (b->blocks.units.empty()) return rc;
  try {
    // A lead block whose 128 docs fall into many blocks of the other terms — a rare lead against
    // frequent terms — is one wavefront decoding those blocks one after the other: it is cut into
    // 2^lg pieces, a wavefront each (ConjItem).  A lead doc falls into at most one block per term,
    // and a term has df_j / df_lead blocks per lead doc: W = sum_j min(128, df_j / df_lead) blocks
    // per lead block; pieces of about 16.  (Measured on the reference's AndHighLow class — lead df
    // ~280 against 720 k: 0.98 -> 0.11 ms per 256 queries.)  Only while the batch cannot fill the
    // chip anyway: with more lead blocks than wavefront slots every wavefront's chain hides behind
    // the others', and the pieces' repeated lead decodes and shared border blocks only add work
    // (config 5's AND batch: 13.4 -> 15.7 ms with the cut applied to every unit).
    uint64_t lead_items = 0;
    for (uint32_t u : b->blocks.units) {
      const DevQuery& dq = b->queries[u];
      if (dq.n_terms) lead_items += b->segs[dq.seg]->terms[b->qterms[dq.first_term].term].nblk + 1u;
    }
    const bool roomy = lead_items < 2ull * 32ull * b->seg->cus;   // (8 wavefronts per SIMD)
    const int forced_lg = b->knobs.conj_split_log2;   // tuning / test knob
    std::vector<uint32_t> split_lg;
    for (uint32_t u : b->blocks.units) {
      const DevQuery& dq = b->queries[u];
      uint32_t items = 0, lg = 0;
      if (dq.n_terms) {
        const irs_hip_segment* sg = b->segs[dq.seg];
        const DevTerm& t = sg->terms[b->qterms[dq.first_term].term];
        items = t.nblk + ((t.docs_count == 1 || t.tail_n) ? 1u : 0u);
        uint64_t want = 0;
        for (uint32_t j = 1; j < dq.n_terms; ++j) {
          const uint64_t df = sg->terms[b->qterms[dq.first_term + j].term].docs_count;
          want += std::min<uint64_t>(kBlock, df / std::max<uint32_t>(1u, t.docs_count));
        }
        while (roomy && lg < kConjSplitMax && (want >> lg) > 16u) ++lg;
        if (forced_lg >= 0) lg = uint32_t(forced_lg);
      }
      split_lg.push_back(lg);
      b->blocks.items.push_back(items << lg);
    }
    if (const int rc = stage_lead_items(b, b->blocks, b->blocks.d_lg, split_lg)) return rc;
    b->blocks.n_wgs = (b->blocks.n_items + kConjWaves - 1) / kConjWaves;
  } catch (...) {
    rc = IRS_HIP_ENOMEM;
  }
  return rc;
}

// The pilot pass's work list of a block-driven batch (And / by_phrase / grouped And): lead items
// {phase, phase + P, ...} of every unit in w.units.
bool ensure_pilot_list(irs_hip_batch* b, BlockWork& w, uint32_t stride, rt::stream_t st) {
  if (w.pilot_stride == stride) return true;
  std::vector<PhraseWg> pl;
  for (size_t c = 0; c < w.units.size(); ++c) {
    const uint32_t u = w.units[c];
    for (uint32_t it = (u * 7u) % stride; it < w.items[c]; it += stride)
      pl.push_back(PhraseWg{u, it});
  }
  // (the list being replaced may still be read by a run in flight: recoveries come here)
  if ((w.d_pilot.p && !rt::sync(st)) ||
      !w.d_pilot.alloc(std::max<size_t>(1, pl.size()) * sizeof(PhraseWg)) ||
      !b->up.copy(w.d_pilot.p, pl.data(), pl.size() * sizeof(PhraseWg)) || !b->up.flush(st))
    return false;
  w.n_pilot = uint32_t(pl.size());
  w.pilot_stride = stride;
  return true;
}

// What k_conj, k_phrase and k_conj_any read of the batch, the same for all (ConjArgs: passed by
// value); w: the tables of their units
ConjArgs block_args(const irs_hip_batch* b, const BlockWork& w, uint32_t pilot_stride) {
  ConjArgs a{};
  a.segs = b->d_segs.as<DevSegment>();
  a.queries = b->d_queries.as<DevQuery>();
  a.qterms = b->d_qterms.as<DevQTerm>();
  a.wgs = nullptr;
  a.n_items = w.n_items;
  a.tails = b->d_tails.as<DevTail>();
  a.bstar = b->d_bstar.as<uint32_t>();
  a.cands = b->d_cands.as<uint64_t>();
  a.cand_count = b->d_cand_count.as<uint32_t>();
  a.hits = b->d_hits.as<unsigned long long>();
  a.hist = w.d_hist.as<uint32_t>();
  a.touched = b->count_touched ? b->d_touched.as<unsigned long long>() : nullptr;
  if (b->excl.leads_counted && b->excl.d_leads.p) {   // (zeroed by the run)
    a.leads = b->excl.d_leads.as<unsigned long long>();
    a.restricted = b->excl.d_restricted.as<uint8_t>();
  }
  a.seek = w.d_seek.as<uint32_t>();
  a.recs = w.d_recs.as<ConjItem>();
  a.unit_items = w.d_unit_items.as<uint32_t>();
  a.item_hits = w.d_item_hits.as<uint32_t>();
  a.jt = b->jt;
  a.cand_cap = b->cand_cap;
  a.pilot_stride = pilot_stride;
  return a;
}

// A counting run of a batch with doc sets: the lead pieces of the restricted units among the
// records the seek kernel has just written (irs_hip_batch_doc_set_stats)
void count_leads(const BlockWork& w, const ConjArgs& a, rt::stream_t st) {
  if (!a.leads || !w.n_items) return;
  RT_LAUNCH(k_count_leads, (w.n_items + kThreads - 1) / kThreads, kThreads, 0, st, w.d_recs.as<ConjItem>(),
            w.n_items, a.restricted, a.leads);
}

// Conjunctions: [pilot pass over every P-th lead block -> threshold bins] -> full pass.
template<int LAYOUT>
bool launch_conj(irs_hip_batch* b, rt::stream_t st) {
  if (b->blocks.n_wgs == 0) return true;
  ConjArgs a = block_args(b, b->blocks, b->stride_eff);
  a.wand = b->wand ? 1u : 0u;
  a.pruned = b->d_pruned.as<uint32_t>();
  if (!ensure_pilot_list(b, b->blocks, a.pilot_stride, st)) return false;
  if (!rt::dmemset(b->blocks.d_hist.p, 0, b->blocks.d_hist.n, st) ||
      !rt::dmemset(b->blocks.d_item_hits.p, 0, b->blocks.d_item_hits.n, st))
    return false;
  RT_LAUNCH(k_conj_seek, (b->blocks.n_items + kThreads - 1) / kThreads, kThreads, 0, st,
            b->d_segs.as<DevSegment>(), b->d_queries.as<DevQuery>(), b->d_tails.as<DevTail>(),
            b->jt, b->blocks.d_units.as<uint32_t>(), b->blocks.d_item_base.as<uint32_t>(),
            uint32_t(b->blocks.units.size()), static_cast<const uint32_t*>(nullptr),
            b->blocks.d_lg.as<uint32_t>(), b->blocks.d_seek.as<uint32_t>(), b->blocks.d_recs.as<ConjItem>());
  count_leads(b->blocks, a, st);
  if (b->blocks.n_pilot) {
    ConjArgs p = a;
    p.wgs = b->blocks.d_pilot.as<PhraseWg>();
    p.n_pilot = b->blocks.n_pilot;
    RT_LAUNCH((k_conj<LAYOUT>), (b->blocks.n_pilot + kConjWaves - 1) / kConjWaves, kConjWaves * 64, 0,
              st, p, 1u);
  }
  RT_LAUNCH(k_conj_threshold, uint32_t(b->blocks.units.size()), 64, 0, st,
            b->d_queries.as<DevQuery>(), b->blocks.d_units.as<uint32_t>(),
            b->blocks.d_items.as<uint32_t>(), b->blocks.d_hist.as<uint32_t>(), a.pilot_stride,
            b->estimate ? kPilotMargin : 0u, b->d_bstar.as<uint32_t>(), min_bins(b));
  RT_LAUNCH((k_conj<LAYOUT>), (b->blocks.n_items + kConjWaves - 1) / kConjWaves, kConjWaves * 64,
            0, st, a, 0u);
  RT_LAUNCH(k_conj_hits, uint32_t(b->blocks.units.size()), 64, 0, st, b->blocks.d_units.as<uint32_t>(),
            b->blocks.d_item_base.as<uint32_t>(), b->blocks.d_item_hits.as<uint32_t>(),
            b->d_hits.as<unsigned long long>());
  return rt::last_error_ok();
}

// by_phrase: lead-item records + start blocks -> pilot pass over every P-th lead block ->
// threshold bins -> full pass.
// REQ: a batch with required terms (IRS_HIP_PHRASE_REQUIRED), every unit on k_phrase_and.
// REQ == kPhraseOpt: a batch with optional terms (IRS_HIP_PHRASE_OPTIONAL), every unit on k_phrase_or.
// REQ == kPhraseSeveral: a batch with several phrases in one And (IRS_HIP_PHRASE_NEXT), every unit on
// k_phrases_and (phrases.h).
template<int LAYOUT, int MT, int REQ = 0>
bool launch_phrase(irs_hip_batch* b, rt::stream_t st) {
  if (b->blocks.n_phrase_wgs == 0) return true;  // no query has all its terms in its segment
  const uint32_t stride = b->stride_eff;
  if (!ensure_pilot_list(b, b->blocks, stride, st) || !rt::dmemset(b->blocks.d_hist.p, 0, b->blocks.d_hist.n, st))
    return false;
  ConjArgs a = block_args(b, b->blocks, stride);
  a.lead_of = b->blocks.d_lead_of.as<uint32_t>();
  if (!rt::dmemset(b->blocks.d_item_hits.p, 0, b->blocks.d_item_hits.n, st)) return false;
  RT_LAUNCH(k_conj_seek, (b->blocks.n_items + kThreads - 1) / kThreads, kThreads, 0, st,
            b->d_segs.as<DevSegment>(), b->d_queries.as<DevQuery>(), b->d_tails.as<DevTail>(),
            b->jt, b->blocks.d_units.as<uint32_t>(), b->blocks.d_item_base.as<uint32_t>(),
            uint32_t(b->blocks.units.size()), b->blocks.d_lead_of.as<uint32_t>(),
            static_cast<const uint32_t*>(nullptr), b->blocks.d_seek.as<uint32_t>(),
            b->blocks.d_recs.as<ConjItem>());
  count_leads(b->blocks, a, st);
  if (b->blocks.n_pilot) {
    ConjArgs p = a;
    p.wgs = b->blocks.d_pilot.as<PhraseWg>();
    p.n_pilot = b->blocks.n_pilot;
    p.touched = nullptr;
    if constexpr (REQ == kPhraseSeveral) {
      RT_LAUNCH((k_phrases_and<LAYOUT, MT>), (b->blocks.n_pilot + kPhraseWaves - 1) / kPhraseWaves,
                kPhraseWaves * 64, 0, st, p, b->blocks.d_n_phrase.as<uint32_t>(),
                b->blocks.d_opens.as<uint32_t>(), 1u);
    } else if constexpr (REQ == kPhraseOpt) {
      RT_LAUNCH((k_phrase_or<LAYOUT, MT>), (b->blocks.n_pilot + kPhraseWaves - 1) / kPhraseWaves,
                kPhraseWaves * 64, 0, st, p, b->blocks.d_n_phrase.as<uint32_t>(),
                b->d_taken.as<uint32_t>(), 2u * b->taken_words, 1u);
    } else if constexpr (REQ) {
      RT_LAUNCH((k_phrase_and<LAYOUT, MT>), (b->blocks.n_pilot + kPhraseWaves - 1) / kPhraseWaves,
                kPhraseWaves * 64, 0, st, p, b->blocks.d_n_phrase.as<uint32_t>(), 1u);
    } else if (MT == 2) {
      RT_LAUNCH(k_phrase2<LAYOUT>, (b->blocks.n_pilot + kPhraseWaves - 1) / kPhraseWaves,
                kPhraseWaves * 64, 0, st, p, 1u);
    } else {
      RT_LAUNCH((k_phrase<LAYOUT, MT>), (b->blocks.n_pilot + kPhraseWaves - 1) / kPhraseWaves,
                kPhraseWaves * 64, 0, st, p, 1u);
    }
  }
  RT_LAUNCH(k_conj_threshold, uint32_t(b->blocks.units.size()), 64, 0, st,
            b->d_queries.as<DevQuery>(), b->blocks.d_units.as<uint32_t>(),
            b->blocks.d_items.as<uint32_t>(), b->blocks.d_hist.as<uint32_t>(), stride,
            b->estimate ? kPilotMargin : 0u, b->d_bstar.as<uint32_t>(), min_bins(b));
  if constexpr (REQ == kPhraseSeveral) {
    RT_LAUNCH((k_phrases_and<LAYOUT, MT>), b->blocks.n_phrase_wgs, kPhraseWaves * 64, 0, st, a,
              b->blocks.d_n_phrase.as<uint32_t>(), b->blocks.d_opens.as<uint32_t>(), 0u);
  } else if constexpr (REQ == kPhraseOpt) {
    RT_LAUNCH((k_phrase_or<LAYOUT, MT>), b->blocks.n_phrase_wgs, kPhraseWaves * 64, 0, st, a,
              b->blocks.d_n_phrase.as<uint32_t>(), b->d_taken.as<uint32_t>(), 2u * b->taken_words, 0u);
  } else if constexpr (REQ) {
    RT_LAUNCH((k_phrase_and<LAYOUT, MT>), b->blocks.n_phrase_wgs, kPhraseWaves * 64, 0, st, a,
              b->blocks.d_n_phrase.as<uint32_t>(), 0u);
  } else if (MT == 2) {
    RT_LAUNCH(k_phrase2<LAYOUT>, b->blocks.n_phrase_wgs, kPhraseWaves * 64, 0, st, a, 0u);
  } else {
    RT_LAUNCH((k_phrase<LAYOUT, MT>), b->blocks.n_phrase_wgs, kPhraseWaves * 64, 0, st, a, 0u);
  }
  RT_LAUNCH(k_conj_hits, uint32_t(b->blocks.units.size()), 64, 0, st, b->blocks.d_units.as<uint32_t>(),
            b->blocks.d_item_base.as<uint32_t>(), b->blocks.d_item_hits.as<uint32_t>(),
            b->d_hits.as<unsigned long long>());
  return rt::last_error_ok();
}
// Several phrases in one Or (k_phrases_or<LAYOUT, MT>, phrases_or.h): the same stages — pilot list,
// threshold, full pass, hit counts — with the lead items of every phrase; records and seek rows from
// k_phrases_or_seek.
template<int LAYOUT, int MT>
bool launch_phrases_or(irs_hip_batch* b, rt::stream_t st) {
  if (b->blocks.n_phrase_wgs == 0) return true;
  const uint32_t stride = b->stride_eff;
  if (!ensure_pilot_list(b, b->blocks, stride, st) || !rt::dmemset(b->blocks.d_hist.p, 0, b->blocks.d_hist.n, st) ||
      !rt::dmemset(b->blocks.d_item_hits.p, 0, b->blocks.d_item_hits.n, st))
    return false;
  ConjArgs a = block_args(b, b->blocks, stride);
  const uint32_t* opens = b->blocks.d_opens.as<uint32_t>();
  RT_LAUNCH(k_phrases_or_seek, (b->blocks.n_items + kThreads - 1) / kThreads, kThreads, 0, st,
            b->d_segs.as<DevSegment>(), b->d_queries.as<DevQuery>(), b->d_tails.as<DevTail>(),
            b->jt, b->blocks.d_units.as<uint32_t>(), b->blocks.d_item_base.as<uint32_t>(),
            uint32_t(b->blocks.units.size()), b->blocks.d_lead_rows.as<uint32_t>(),
            b->blocks.d_seek.as<uint32_t>(), b->blocks.d_recs.as<ConjItem>());
  count_leads(b->blocks, a, st);
  if (b->blocks.n_pilot) {
    ConjArgs p = a;
    p.wgs = b->blocks.d_pilot.as<PhraseWg>();
    p.n_pilot = b->blocks.n_pilot;
    p.touched = nullptr;
    RT_LAUNCH((k_phrases_or<LAYOUT, MT>), (b->blocks.n_pilot + kPhraseWaves - 1) / kPhraseWaves,
              kPhraseWaves * 64, 0, st, p, opens, 1u);
  }
  RT_LAUNCH(k_conj_threshold, uint32_t(b->blocks.units.size()), 64, 0, st,
            b->d_queries.as<DevQuery>(), b->blocks.d_units.as<uint32_t>(),
            b->blocks.d_items.as<uint32_t>(), b->blocks.d_hist.as<uint32_t>(), stride,
            b->estimate ? kPilotMargin : 0u, b->d_bstar.as<uint32_t>(), min_bins(b));
  RT_LAUNCH((k_phrases_or<LAYOUT, MT>), b->blocks.n_phrase_wgs, kPhraseWaves * 64, 0, st, a, opens, 0u);
  RT_LAUNCH(k_conj_hits, uint32_t(b->blocks.units.size()), 64, 0, st, b->blocks.d_units.as<uint32_t>(),
            b->blocks.d_item_base.as<uint32_t>(), b->blocks.d_item_hits.as<uint32_t>(),
            b->d_hits.as<unsigned long long>());
  return rt::last_error_ok();
}
// Variadic phrases (k_vphrase): the same stages, with the items of every lead member.
template<int LAYOUT>
bool launch_vphrase(irs_hip_batch* b, rt::stream_t st) {
  if (b->blocks.n_phrase_wgs == 0) return true;
  const uint32_t stride = b->stride_eff;
  if (!ensure_pilot_list(b, b->blocks, stride, st) || !rt::dmemset(b->blocks.d_hist.p, 0, b->blocks.d_hist.n, st) ||
      !rt::dmemset(b->blocks.d_item_hits.p, 0, b->blocks.d_item_hits.n, st))
    return false;
  ConjArgs a = block_args(b, b->blocks, stride);
  const uint32_t* opens = b->blocks.d_opens.as<uint32_t>();
  RT_LAUNCH(k_vphrase_seek, (b->blocks.n_items + kThreads - 1) / kThreads, kThreads, 0, st,
            b->d_segs.as<DevSegment>(), b->d_queries.as<DevQuery>(), b->d_tails.as<DevTail>(),
            b->jt, b->blocks.d_units.as<uint32_t>(), b->blocks.d_item_base.as<uint32_t>(),
            uint32_t(b->blocks.units.size()), b->blocks.d_lead_rows.as<uint32_t>(),
            b->blocks.d_seek.as<uint32_t>(), b->blocks.d_recs.as<ConjItem>());
  count_leads(b->blocks, a, st);
  if (b->blocks.n_pilot) {
    ConjArgs p = a;
    p.wgs = b->blocks.d_pilot.as<PhraseWg>();
    p.n_pilot = b->blocks.n_pilot;
    p.touched = nullptr;
    RT_LAUNCH(k_vphrase<LAYOUT>, (b->blocks.n_pilot + kPhraseWaves - 1) / kPhraseWaves,
              kPhraseWaves * 64, 0, st, p, opens, 1u);
  }
  RT_LAUNCH(k_conj_threshold, uint32_t(b->blocks.units.size()), 64, 0, st,
            b->d_queries.as<DevQuery>(), b->blocks.d_units.as<uint32_t>(),
            b->blocks.d_items.as<uint32_t>(), b->blocks.d_hist.as<uint32_t>(), stride,
            b->estimate ? kPilotMargin : 0u, b->d_bstar.as<uint32_t>(), min_bins(b));
  RT_LAUNCH(k_vphrase<LAYOUT>, b->blocks.n_phrase_wgs, kPhraseWaves * 64, 0, st, a, opens, 0u);
  RT_LAUNCH(k_conj_hits, uint32_t(b->blocks.units.size()), 64, 0, st, b->blocks.d_units.as<uint32_t>(),
            b->blocks.d_item_base.as<uint32_t>(), b->blocks.d_item_hits.as<uint32_t>(),
            b->d_hits.as<unsigned long long>());
  return rt::last_error_ok();
}
template<int LAYOUT>
bool launch_phrase_terms(irs_hip_batch* b, rt::stream_t st) {
  if (b->blocks.variadic) return launch_vphrase<LAYOUT>(b, st);
  if (b->blocks.disj)   // (every unit on k_phrases_or)
    return b->jt <= 4 ? launch_phrases_or<LAYOUT, 4>(b, st) : launch_phrases_or<LAYOUT, int(kPhraseMaxTerms)>(b, st);
  if (b->blocks.several)   // (with or without required terms: every unit on k_phrases_and)
    return b->jt <= 4 ? launch_phrase<LAYOUT, 4, kPhraseSeveral>(b, st)
                      : launch_phrase<LAYOUT, int(kPhraseMaxTerms), kPhraseSeveral>(b, st);
  if (b->blocks.required)
    return b->jt <= 4 ? launch_phrase<LAYOUT, 4, kPhraseReq>(b, st)
                      : launch_phrase<LAYOUT, int(kPhraseMaxTerms), kPhraseReq>(b, st);
  if (b->blocks.optional)
    return b->jt <= 4 ? launch_phrase<LAYOUT, 4, kPhraseOpt>(b, st)
                      : launch_phrase<LAYOUT, int(kPhraseMaxTerms), kPhraseOpt>(b, st);
  if (b->jt <= 2) return launch_phrase<LAYOUT, 2>(b, st);
  if (b->jt <= 4) return launch_phrase<LAYOUT, 4>(b, st);
  return launch_phrase<LAYOUT, int(kPhraseMaxTerms)>(b, st);
}

}  // namespace
