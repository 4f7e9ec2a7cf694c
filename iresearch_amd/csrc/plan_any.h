// plan_any.h — host half of the grouped conjunctions (an And of Ors of by_term, IRS_HIP_GROUP_ALT;
// conj_any.h): the lead-item work list, the pilot pass's sample of it, the k_conj_any launches.
// Included by irs_hip.hip (one translation unit).
#pragma once

namespace {

// k_conj_any work of the batch's grouped units, built at create (their path never changes): the
// lead planning of the variadic phrases (build_lead_groups) — the cheapest group leads, a wavefront
// per block (+ tail) of every member of it
int build_any_work(irs_hip_batch* b, const std::vector<uint32_t>& grouped) {
  const int rc = build_lead_groups(b, b->any, grouped);
  if (b->any.units.empty()) return rc;
  b->any.n_wgs = (b->any.n_items + kConjWaves - 1) / kConjWaves;
  return rc;
}

// Grouped conjunctions: lead-item records + start blocks -> pilot pass over every P-th lead item ->
// threshold bins -> full pass -> match counts.  No block-max pruning: they run exhaustively.
template<int LAYOUT>
bool launch_any(irs_hip_batch* b, rt::stream_t st) {
  AnyWork& w = b->any;
  if (w.n_wgs == 0) return true;
  const uint32_t stride = b->stride_eff;
  if (!ensure_pilot_list(b, w, stride, st) || !rt::dmemset(w.d_hist.p, 0, w.d_hist.n, st) ||
      !rt::dmemset(w.d_item_hits.p, 0, w.d_item_hits.n, st))
    return false;
  ConjArgs a = block_args(b, w, stride);
  const uint32_t* opens = w.d_opens.as<uint32_t>();
  RT_LAUNCH(k_vphrase_seek, (w.n_items + kThreads - 1) / kThreads, kThreads, 0, st,
            b->d_segs.as<DevSegment>(), b->d_queries.as<DevQuery>(), b->d_tails.as<DevTail>(),
            b->jt, w.d_units.as<uint32_t>(), w.d_item_base.as<uint32_t>(), uint32_t(w.units.size()),
            w.d_lead_rows.as<uint32_t>(), w.d_seek.as<uint32_t>(), w.d_recs.as<ConjItem>());
  count_leads(w, a, st);
  if (w.n_pilot) {
    ConjArgs p = a;
    p.wgs = w.d_pilot.as<PhraseWg>();
    p.n_pilot = w.n_pilot;
    p.touched = nullptr;
    RT_LAUNCH(k_conj_any<LAYOUT>, (w.n_pilot + kConjWaves - 1) / kConjWaves, kConjWaves * 64, 0, st,
              p, opens, 1u);
  }
  RT_LAUNCH(k_conj_threshold, uint32_t(w.units.size()), 64, 0, st, b->d_queries.as<DevQuery>(),
            w.d_units.as<uint32_t>(), w.d_items.as<uint32_t>(), w.d_hist.as<uint32_t>(), stride,
            b->estimate ? kPilotMargin : 0u, b->d_bstar.as<uint32_t>(), min_bins(b));
  RT_LAUNCH(k_conj_any<LAYOUT>, w.n_wgs, kConjWaves * 64, 0, st, a, opens, 0u);
  RT_LAUNCH(k_conj_hits, uint32_t(w.units.size()), 64, 0, st, w.d_units.as<uint32_t>(),
            w.d_item_base.as<uint32_t>(), w.d_item_hits.as<uint32_t>(), b->d_hits.as<unsigned long long>());
  return rt::last_error_ok();
}

}  // namespace
