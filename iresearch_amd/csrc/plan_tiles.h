// plan_tiles.h — host half of the doc-tile units that run as work items (score.h): the work-item
// lists (k_items_count / k_items_fill) and the k_pilot / k_score launches.
// Included by irs_hip.hip (one translation unit).
#pragma once

namespace {

// The tile kernels' template arguments: one instantiation per (accumulator width, layout, tile, AND)
template<typename A, int L, int T, bool N>
struct TileKernel {
  using ACC = A;
  static constexpr int LAYOUT = L, TILE = T;
  static constexpr bool AND = N;
};
// f(TileKernel<...>{}) with the batch's arguments
template<typename F>
auto with_tile_kernel(const irs_hip_batch* b, F&& f) {
  auto by_and = [&](auto acc, auto layout, auto tile) {
    using A = decltype(acc);
    constexpr int L = decltype(layout)::value, T = decltype(tile)::value;
    return b->tiles.any_and ? f(TileKernel<A, L, T, true>{}) : f(TileKernel<A, L, T, false>{});
  };
  auto by_tile = [&](auto acc, auto layout) {
    switch (b->tiles.docs) {
      case 12288: return by_and(acc, layout, std::integral_constant<int, 12288>{});
      case 8192: return by_and(acc, layout, std::integral_constant<int, 8192>{});
      case 6144: return by_and(acc, layout, std::integral_constant<int, 6144>{});
      default: return by_and(acc, layout, std::integral_constant<int, 4096>{});
    }
  };
  auto by_layout = [&](auto acc) { return with_layout(b->seg->dev.layout, [&](auto l) { return by_tile(acc, l); }); };
  return b->acc32 ? by_layout(uint32_t{0}) : by_layout(0ull);
}

// The per-tile "some doc can match" bytes of a batch with doc sets (k_tile_live), else null
const uint8_t* tile_live(const irs_hip_batch* b) {
  return b->excl.sets_on() ? b->excl.d_tile_live.as<uint8_t>() : nullptr;
}

template<typename ACC, int LAYOUT, int TILE, bool AND>
bool launch_pilot(irs_hip_batch* b, rt::stream_t st, TileKernel<ACC, LAYOUT, TILE, AND>) {
  const size_t smem = tile_smem_bytes<ACC, TILE, AND>() + kBins * sizeof(uint32_t);
  auto kern = k_pilot<ACC, LAYOUT, TILE, AND>;
  if (!big_smem(kern, smem)) return false;
  RT_LAUNCH(kern, uint32_t(b->tiles.units.size()), b->tiles.threads, smem, st,
            b->tiles.d_units.as<uint32_t>(), b->d_segs.as<DevSegment>(),
            b->d_queries.as<DevQuery>(), b->d_qterms.as<DevQTerm>(), b->stride_eff,
            b->tiles.nw_log2, b->tiles.d_off.as<uint32_t>(), reinterpret_cast<uint64_t>(b->tiles.d_items.p),
            b->d_bstar.as<uint32_t>(), b->estimate ? kPilotMargin : 0u, min_bins(b), tile_live(b));
  return rt::last_error_ok();
}

template<typename ACC, int LAYOUT, int TILE, bool AND>
bool launch_score(irs_hip_batch* b, rt::stream_t st, TileKernel<ACC, LAYOUT, TILE, AND>) {
  const size_t smem = score_smem_bytes<ACC, TILE, AND>();
  auto kern = k_score<ACC, LAYOUT, TILE, AND>;
  if (!big_smem(kern, smem)) return false;
  // persistent grid: as many workgroups as stay resident on the chip at once
  const uint32_t waves = b->tiles.threads / 64;
  uint32_t per_cu = uint32_t((160u * 1024u) / smem);
  per_cu = std::max<uint32_t>(1, std::min<uint32_t>(per_cu, 16u / waves));  // 128 VGPRs: 4 waves/SIMD
  const uint32_t cpq = (b->tiles.n_max + kChunkTiles - 1) / kChunkTiles;  // chunk ids per unit
  const uint32_t n_units = uint32_t(b->tiles.units.size());
  const uint64_t chunks = uint64_t(n_units) * cpq;
  if (chunks > 0xFFFF0000ull) return false;
  const uint32_t grid = uint32_t(std::min<uint64_t>(chunks, uint64_t(b->seg->cus) * per_cu));
  ScoreArgs& a = b->tiles.args;   // read by the kernel from device memory (score.h)
  a.segs = b->d_segs.as<DevSegment>();
  a.queries = b->d_queries.as<DevQuery>();
  a.qterms = b->d_qterms.as<DevQTerm>();
  a.tile_off = b->tiles.d_off.as<uint32_t>();
  a.items = reinterpret_cast<uint64_t>(b->tiles.d_items.p);
  a.bstar = b->d_bstar.as<uint32_t>();
  a.cands = b->d_cands.as<uint64_t>();
  a.cand_count = b->d_cand_count.as<uint32_t>();
  a.hits = b->d_hits.as<unsigned long long>();
  a.work_counter = b->tiles.d_work.as<uint32_t>();
  a.tile_ub = b->wand ? b->tiles.d_ub.as<float>() : nullptr;
  a.pruned = b->d_pruned.as<uint32_t>();
  a.tile_live = tile_live(b);
  a.cpq = cpq;
  a.n_units = n_units;
  a.nw_log2 = b->tiles.nw_log2;
  a.cand_cap = b->cand_cap;
  // (the arguments only change with the batch's geometry or a regrown candidate buffer)
  if (std::memcmp(&a, &b->tiles.args_sent, sizeof a) != 0 || !b->tiles.args_valid) {
    if (!b->up.copy(b->tiles.d_args.p, &a, sizeof a) || !b->up.flush(st)) return false;
    std::memcpy(&b->tiles.args_sent, &a, sizeof a);
    b->tiles.args_valid = true;
  }
  if (!rt::dmemset(b->tiles.d_work.p, 0, 4, st)) return false;
  RT_LAUNCH(kern, grid, b->tiles.threads, smem, st, reinterpret_cast<uint64_t>(b->tiles.d_args.p));
  return rt::last_error_ok();
}

// LDS byte offset of the table rows in the tile kernels' layout (what k_items_fill writes
// into the work items' `tab` field)
uint32_t caches_off(const irs_hip_batch* b) {
  return with_tile_kernel(b, [](auto k) {
    using K = decltype(k);
    return TileOff<typename K::ACC, K::TILE, K::AND>::caches;
  });
}

// Work-item lists of every (unit, doc tile): count -> exclusive scan (all on the device, no
// host round trip: the buffer is sized by an upper bound) -> fill.
bool launch_items(irs_hip_batch* b, rt::stream_t st) {
  uint32_t* off = b->tiles.d_off.as<uint32_t>();
  const uint64_t n = uint64_t(b->tiles.n_total) + 1;   // [n_total] = 0 -> the grand total
  if (!rt::dmemset(off + b->tiles.n_total, 0, 4, st)) return false;
  const uint32_t tb4 = (b->tiles.n_max + kWaves - 1) / kWaves;
  // doc sets: which tiles hold a doc their unit's mask leaves (the masks are built: plan_stage)
  if (b->excl.sets_on())
    RT_LAUNCH(k_tile_live, b->nq * tb4, kThreads, 0, st, b->d_queries.as<DevQuery>(),
              b->excl.d_restricted.as<uint8_t>(), b->tiles.docs, tb4, b->excl.d_tile_live.as<uint8_t>());
  const uint32_t tb = (b->tiles.n_max + kThreads - 1) / kThreads;
  RT_LAUNCH(k_items_count, b->nq * tb, kThreads, 0, st, b->d_queries.as<DevQuery>(), b->jt,
            b->tiles.docs, tb, b->d_first.as<uint32_t>(), b->d_tails.as<DevTail>(), off, tile_live(b));
  const uint32_t parts = uint32_t((n + kScanChunk - 1) / kScanChunk);
  uint64_t* totals = b->tiles.d_scan_parts.as<uint64_t>();
  RT_LAUNCH(k_scan_totals, parts, kThreads, 0, st, off, n, totals);
  RT_LAUNCH(k_scan_parts, 1, 64, 0, st, totals, parts);
  RT_LAUNCH(k_scan_apply, parts, kThreads, 0, st, off, n, totals);
  RT_LAUNCH(k_items_fill, b->nq * tb4, kThreads, 0, st, b->d_segs.as<DevSegment>(),
            b->d_queries.as<DevQuery>(), b->d_qterms.as<DevQTerm>(), b->jt, b->tiles.docs, tb4,
            b->tiles.nw_log2, caches_off(b), b->d_first.as<uint32_t>(), b->d_tails.as<DevTail>(), off,
            b->tiles.n_total, b->tiles.d_items.as<ItemG>(), b->wand ? b->tiles.d_ub.as<float>() : nullptr,
            tile_live(b));
  return rt::last_error_ok();
}

}  // namespace
