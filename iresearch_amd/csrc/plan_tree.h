// plan_tree.h — host half of the tree queries (tree.h): the units' geometry, their node tables on
// the device, the k_tree_pilot / k_tree_score launches.  What create refuses of such a query:
// tree_shape.h (its shape) and plan_wide.h wide_terms_ok (its leaves: they are scored from decoded
// streams as a wide unit's terms are).  Their posting streams are the batch's (plan_join.h
// build_streams).  Included by irs_hip.hip (one translation unit).
#pragma once

namespace {

bool unit_is_tree(const DevQuery& dq) { return query_run(dq.op) == kRunTree; }

// The tiles of a tree unit (size_units): kJoinTile docs each, no plan table, no work items
void size_tree_unit(irs_hip_batch* b, DevQuery& dq) {
  dq.n_tiles = dq.n_terms ? (b->segs[dq.seg]->dev.num_docs + kJoinTile - 1) / kJoinTile : 0u;
  dq.first_off = kNoPlan;
  dq.tile_base = 0;
  b->tree.n_max = std::max(b->tree.n_max, dq.n_tiles);
  if (dq.n_tiles) b->tree.n_min = std::min(b->tree.n_min, dq.n_tiles);
}

bool alloc_tree(irs_hip_batch* b) {
  if (!b->tree.on()) return true;
  return b->tree.d_units.alloc(b->tree.units.size() * 4) &&
         b->up.copy(b->tree.d_units.p, b->tree.units.data(), b->tree.units.size() * 4) &&
         b->tree.d_nodes.alloc(b->tree.nodes.size() * sizeof(TreeNode)) &&
         b->up.copy(b->tree.d_nodes.p, b->tree.nodes.data(), b->tree.nodes.size() * sizeof(TreeNode));
}

// (wide_stride's rule over these units' tiles)
uint32_t tree_stride(const irs_hip_batch* b) {
  const uint32_t most = b->tree.n_min == 0xFFFFFFFFu ? 1u : std::max<uint32_t>(1, b->tree.n_min / 2);
  return std::max<uint32_t>(1, std::min<uint32_t>(b->stride_eff, most));
}

bool launch_tree_pilot(irs_hip_batch* b, rt::stream_t st) {
  const size_t smem = TreeOff::end + kBins * sizeof(uint32_t);
  if (!big_smem(k_tree_pilot, smem)) return false;
  RT_LAUNCH(k_tree_pilot, uint32_t(b->tree.units.size()), kWideThreads, smem, st,
            b->tree.d_units.as<uint32_t>(), b->d_queries.as<DevQuery>(), b->d_qterms.as<DevQTerm>(),
            b->join.d_jterms.as<JoinTerm>(), b->tree.d_nodes.as<TreeNode>(), tree_stride(b),
            b->d_bstar.as<uint32_t>(), b->estimate ? kPilotMargin : 0u, min_bins(b));
  return rt::last_error_ok();
}

bool launch_tree_score(irs_hip_batch* b, rt::stream_t st) {
  const size_t smem = TreeOff::end;
  if (!big_smem(k_tree_score, smem)) return false;
  // chunks of up to kWideChunkTiles tiles, the unit's tiles cut evenly (launch_wide_score's rule)
  const uint32_t n_max = std::max<uint32_t>(1, b->tree.n_max);
  const uint32_t cpq = (n_max + kWideChunkTiles - 1) / kWideChunkTiles;
  const uint64_t grid = uint64_t(b->tree.units.size()) * cpq;
  if (grid > 0x7FFFFFFFull) return false;
  TreeArgs ta{};
  WideArgs& a = ta.w;
  a.units = b->tree.d_units.as<uint32_t>();
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
  ta.nodes = b->tree.d_nodes.as<TreeNode>();
  RT_LAUNCH(k_tree_score, uint32_t(grid), kWideThreads, smem, st, ta);
  return rt::last_error_ok();
}

}  // namespace
