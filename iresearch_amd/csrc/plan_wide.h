// plan_wide.h — host half of the scored multi-term units of up to 64 terms (wide.h): what create
// refuses of such a query, the units' geometry, the k_wide_pilot / k_wide_score launches.  Their
// posting streams are the batch's (plan_join.h build_streams).  Included by irs_hip.hip (one
// translation unit).
#pragma once

namespace {

bool unit_is_wide(const DevQuery& dq) { return query_run(dq.op) == kRunWide; }

// What batch_create refuses of an IRS_HIP_OP_MULTITERM query's present terms (`row`, table slots
// assigned): the per-term rules are unit_joinable's — a scorer of the table family with a slot of
// its own (at most kMaxCaches distinct (kind, norm_const, norm_length): wide and legacy norm
// columns resolve to kinds outside the family), every frequency within an entry's 8 bits — plus
// the constant scores of BM1 (k = 0), which read no table (wide.h kWideConst).
int wide_terms_ok(const irs_hip_segment* seg, const std::vector<DevQTerm>& row) {
  for (const DevQTerm& qt : row) {
    if (qt.kind != kBM1 && (!table_kind(qt.kind) || qt.cache_id >= kMaxCaches)) return IRS_HIP_EUNSUPPORTED;
    if (seg->terms[qt.term].tf_bound > kJoinTfMax) return IRS_HIP_EUNSUPPORTED;
  }
  return IRS_HIP_OK;
}

// The tiles of a wide unit (size_units): kJoinTile docs each, no plan table, no work items
void size_wide_unit(irs_hip_batch* b, DevQuery& dq) {
  dq.n_tiles = dq.n_terms ? (b->segs[dq.seg]->dev.num_docs + kJoinTile - 1) / kJoinTile : 0u;
  dq.first_off = kNoPlan;
  dq.tile_base = 0;
  b->wide.n_max = std::max(b->wide.n_max, dq.n_tiles);
  if (dq.n_tiles) b->wide.n_min = std::min(b->wide.n_min, dq.n_tiles);
}

bool alloc_wide(irs_hip_batch* b) {
  if (!b->wide.on()) return true;
  return b->wide.d_units.alloc(b->wide.units.size() * 4) &&
         b->up.copy(b->wide.d_units.p, b->wide.units.data(), b->wide.units.size() * 4);
}

// The pilot samples every P-th tile: the batch's stride (a recovery tightens it), at least two
// sampled tiles per unit where its segment has them
uint32_t wide_stride(const irs_hip_batch* b) {
  const uint32_t most = b->wide.n_min == 0xFFFFFFFFu ? 1u : std::max<uint32_t>(1, b->wide.n_min / 2);
  return std::max<uint32_t>(1, std::min<uint32_t>(b->stride_eff, most));
}

bool launch_wide_pilot(irs_hip_batch* b, rt::stream_t st) {
  const size_t smem = WideOff::end + kBins * sizeof(uint32_t);
  if (!big_smem(k_wide_pilot, smem)) return false;
  RT_LAUNCH(k_wide_pilot, uint32_t(b->wide.units.size()), kWideThreads, smem, st,
            b->wide.d_units.as<uint32_t>(), b->d_queries.as<DevQuery>(), b->d_qterms.as<DevQTerm>(),
            b->join.d_jterms.as<JoinTerm>(), wide_stride(b), b->d_bstar.as<uint32_t>(),
            b->estimate ? kPilotMargin : 0u, min_bins(b));
  return rt::last_error_ok();
}

bool launch_wide_score(irs_hip_batch* b, rt::stream_t st) {
  const size_t smem = WideOff::end;
  if (!big_smem(k_wide_score, smem)) return false;
  // chunks of up to kWideChunkTiles tiles, the unit's tiles cut evenly (k_join_score's rule)
  const uint32_t n_max = std::max<uint32_t>(1, b->wide.n_max);
  const uint32_t cpq = (n_max + kWideChunkTiles - 1) / kWideChunkTiles;
  const uint64_t grid = uint64_t(b->wide.units.size()) * cpq;
  if (grid > 0x7FFFFFFFull) return false;
  WideArgs a{};
  a.units = b->wide.d_units.as<uint32_t>();
  a.queries = b->d_queries.as<DevQuery>();
  a.qterms = b->d_qterms.as<DevQTerm>();
  a.jterms = b->join.d_jterms.as<JoinTerm>();
  a.bstar = b->d_bstar.as<uint32_t>();
  a.cands = b->d_cands.as<uint64_t>();
  a.cand_count = b->d_cand_count.as<uint32_t>();
  a.hits = b->d_hits.as<unsigned long long>();
  a.cpq = cpq;
  a.chunk_tiles = (n_max + cpq - 1) / cpq;
  a.cand_cap = b->cand_cap;
  RT_LAUNCH(k_wide_score, uint32_t(grid), kWideThreads, smem, st, a);
  return rt::last_error_ok();
}

}  // namespace
