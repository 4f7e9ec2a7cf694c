// wide.h — scored multi-term queries of up to 64 terms (IRS_HIP_OP_MULTITERM): by_terms
// (terms_filter.cpp:110-153, MultiTermQuery::execute multiterm_query.cpp:114-181: a
// min_match_iterator over one scored iterator per term) and the scored part of by_range /
// by_prefix / by_wildcard / by_edit_distance beyond IRS_HIP_MAX_TERMS states.
//
//   k_wide_pilot  scores every P-th doc tile of a unit, derives its score-bin threshold
//                 (k_join_pilot's histogram, margin / sound rule and min_bin handling)
//   k_wide_score  accumulates the streams of a unit's terms tile by tile in LDS, counts the hits,
//                 stages the candidates at or above the threshold bin; k_select follows unchanged
//
// A path of its own next to join.h: the 32-bit kernels deal lane j = term j inside 16-entry LDS
// tables and run only while upper / min_score <= 1000 holds for the whole batch; a 50-term sum
// breaks both.  Here lane j = term j over all 64 lanes, and the accumulators are 64-bit fixed
// point whatever the rest of the batch runs on: 2^(61-e) units per score unit (DevQuery::fx_mul /
// fx_inv of THIS unit), the low 7 bits of a sum counting the terms that hold the doc — 64 terms
// count to 64 < 128, and the 7 bits a contribution loses are 2^-54 of the range, so min_match
// needs no second array and no precision rule.
//
// The entries are join.h's (k_join decodes every distinct (segment, term) of the batch once,
// wide units' terms included; the stream cache serves them): [(doc - tile start) * 4 : 16 |
// tf : 6 + 2 | norm : 8], bounds[t] = the entry index at which tile t of kJoinTile docs begins.
// A posting's accumulator is at (e >> 16) * 2; the postings of deleted docs carry the address of
// one of 64 dummy words behind the tile's accumulators.  The contribution is join_post's: the
// table row for a term whose frequencies all have one, else row 0 and the v_rcp / v_sqrt form —
// and the constant c0 for a BM1 term (BM25 with k = 0), which needs no table at all.
//
// One workgroup of 1024 threads per (unit, chunk of consecutive tiles), a plain grid: a chunk's
// cost is known to nobody before it runs, the dispatcher hands the next workgroup to whichever CU
// frees up, and without a prefetch that reaches across chunks a persistent grid with a work counter
// would only add its atomics.  LDS: 96 KB of accumulators + 16 KB of score tables + the records,
// the chunk's ranges and the candidate staging = WideOff::end (~126 KB): ONE workgroup per CU, 16
// wavefronts = 4 per SIMD, at most 128 VGPRs each.
#pragma once
#include "join.h"

namespace irs_hip {

constexpr uint32_t kMaxWideTerms = 64;     // IRS_HIP_MAX_WIDE_TERMS: one lane per term
constexpr uint32_t kWideThreads = 1024;    // 16 wavefronts share a tile's entries
constexpr uint32_t kWideWavesLog2 = 4;
constexpr uint32_t kWideChunkTiles = 16;   // consecutive tiles per k_wide_score workgroup, at most
constexpr uint32_t kWideCands = 512;       // candidate staging slots per chunk
constexpr unsigned long long kWideCountMask = 127ull;
constexpr uint32_t kWideConst = 1u << 28;  // JoinTerm::mode of a wide unit's term: a constant score (BM1: k = 0)
static_assert(kMaxWideTerms <= kWideCountMask, "the low bits of a sum count its terms");
static_assert(kMaxWideTerms == 64u, "lane j = term j");

struct WideOff {
  static constexpr uint32_t acc = 0;                                  // [kJoinTile] u64
  static constexpr uint32_t dummy = 8u * kJoinTile;                   // [64] u64 (deleted docs' postings)
  static constexpr uint32_t qts = dummy + 512u;                       // DevQTerm[kMaxWideTerms]
  static constexpr uint32_t jts = qts + uint32_t(sizeof(DevQTerm)) * kMaxWideTerms;   // JoinTerm[kMaxWideTerms]
  static constexpr uint32_t row_a = jts + uint32_t(sizeof(JoinTerm)) * kMaxWideTerms; // [chunk tiles][64] first entry
  static constexpr uint32_t row_n = row_a + 4u * kWideChunkTiles * kMaxWideTerms;     // [chunk tiles][64] entries
  static constexpr uint32_t cand = row_n + 4u * kWideChunkTiles * kMaxWideTerms;      // [kWideCands] u64
  static constexpr uint32_t vars = cand + 8u * kWideCands;            // [16] u32
  static constexpr uint32_t caches = vars + 64u;                      // [kTableRows][256] f32
  static constexpr uint32_t end = caches + 4u * 256u * kTableRows;
};
static_assert(WideOff::cand % 8u == 0u && WideOff::jts % 16u == 0u && WideOff::caches % 16u == 0u, "WideOff alignment");
static_assert(2u * (4u * kJoinTile + 4u * 63u) + 8u <= WideOff::qts, "a deleted doc's posting lands on a dummy word");
static_assert(WideOff::end + 4u * kBins <= 160u * 1024u, "one workgroup's LDS");
static_assert(2u * WideOff::end > 160u * 1024u, "... and one workgroup per CU: 4 wavefronts per SIMD");

enum : int { kWConst = 3 };   // wide_post FORM next to kJTable / kJRcp / kJSqrt: the score is cs
enum : uint32_t { kWNc = 0, kWBase = 1 };   // WideOff::vars: candidates staged, their reserved base

// The per-lane view of a unit: lane j holds term j (zeros beyond the unit's terms)
__device__ __forceinline__ JoinLane wide_lane(const unsigned char* smem, unsigned lane) {
  const JoinQuad lo = reinterpret_cast<const JoinQuad*>(smem + WideOff::jts)[kJoinTermQuads * lane];
  const JoinQuad hi = reinterpret_cast<const JoinQuad*>(smem + WideOff::jts)[kJoinTermQuads * lane + 1u];
  JoinLane T;
  T.ent_lo = lo.x;   // JoinTerm::entries
  T.ent_hi = lo.y;
  T.cs = __uint_as_float(hi.x);
  T.mode = hi.y;
  return T;
}

// The unit's term scorers and stream records to LDS, its score tables built.  Ends with every
// thread seeing all of it.
__device__ __forceinline__ void wide_prologue(unsigned char* smem, const DevQuery& qd,
                                              const DevQTerm* qterms, const JoinTerm* jterms) {
  DevQTerm* qts = reinterpret_cast<DevQTerm*>(smem + WideOff::qts);
  JoinQuad* jts = reinterpret_cast<JoinQuad*>(smem + WideOff::jts);
  const uint32_t tid = threadIdx.x;
  if (tid < qd.n_terms) qts[tid] = qterms[qd.first_term + tid];
  if (tid < kJoinTermQuads * kMaxWideTerms) {   // a JoinTerm = two 16-byte halves
    const uint32_t j = tid / kJoinTermQuads;
    uint32_t x = 0, y = 0, z = 0, w = 0;
    if (j < qd.n_terms) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(jterms + qd.first_term) + 4u * tid;
      x = src[0]; y = src[1]; z = src[2]; w = src[3];
    }
    jts[tid].x = x; jts[tid].y = y; jts[tid].z = z; jts[tid].w = w;
  }
  __syncthreads();
  JoinSm sm;
  sm.qts = qts;
  sm.caches = reinterpret_cast<float*>(smem + WideOff::caches);
  build_tables(sm, qd.n_caches, qd.n_terms);
  __syncthreads();
}

// One posting: join_post's arithmetic (FORM kJTable: the entry's low 16 bits are the offset of
// T_tf[norm] inside the term's table slot; else row 0 and the general expression), converted to
// the 64-bit fixed point with the term counted in the low bits.
template<int FORM>
__device__ __forceinline__ void wide_post(const unsigned char* lds, uint32_t e, float cs, uint32_t tabofs) {
  float scaled;
  float t = 0.f;
  if (FORM != kWConst) {
    const uint32_t at = (FORM == kJTable) ? ((e & 0xFFFFu) | tabofs) : ((e & 0x3FCu) | tabofs);
    t = wave::lds_f32(lds, WideOff::caches + at);
  }
  if (FORM == kWConst) {
    scaled = cs;
  } else if (FORM == kJTable) {
    scaled = cs * t;
  } else {
    const float tf = static_cast<float>(join_tf(e));
    scaled = (FORM == kJSqrt) ? wave::fast_sqrt(tf) * cs * t
                              : wave::fma(-cs, wave::fast_rcp(wave::fma(tf, t, 1.f)), cs);
  }
  const unsigned long long fx = (fixed_from_scaled<unsigned long long>(scaled) & ~kWideCountMask) | 1ull;
  wave::lds_add(lds, WideOff::acc + (e >> 16) * 2u, fx);
}

// `count` consecutive entries from address `base` (wave-uniform), 256 per step: the loads of a
// step first, then its postings
template<int FORM>
__device__ __forceinline__ void wide_run(const unsigned char* lds, uint64_t base, uint32_t count,
                                         float cs, uint32_t tabofs, unsigned lane) {
  for (uint32_t i = 0; i < count; i += 256u) {
    uint32_t e[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t at = i + 64u * k + lane;
      if (at < count) e[k] = wave::gload_u32(base, at * 4u);
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
      if (i + 64u * k + lane < count) wide_post<FORM>(lds, e[k], cs, tabofs);
  }
}

// A wavefront's share of one tile.  The entries of the unit's terms in the tile, term after term,
// are one sequence of N entries; wavefront w of 16 takes [N w / 16, N (w + 1) / 16), as join_begin
// cuts them: lane j = term j intersects that piece with its term's range [a, a + n) of the stream,
// and the one to few terms the piece touches are run one after the other.  All 64 lanes active.
__device__ __forceinline__ void wide_tile(const unsigned char* lds, const JoinLane& T, uint32_t a,
                                          uint32_t n, uint32_t wv, unsigned lane) {
  const uint32_t c = wave::inclusive_scan(n);
  const uint32_t total = wave::read_lane(c, 63u);
  const uint32_t lo = uint32_t((uint64_t(total) * wv) >> kWideWavesLog2);
  const uint32_t hi = uint32_t((uint64_t(total) * (wv + 1u)) >> kWideWavesLog2);
  const uint32_t t0 = c - n;   // the term's first entry within the sequence
  const uint32_t s = t0 > lo ? t0 : lo, t = c < hi ? c : hi;
  uint64_t touched = wave::ballot(s < t);
  while (touched) {   // (wave-uniform)
    const uint32_t j = wave::uniform(uint32_t(__builtin_ctzll(touched)));
    touched &= touched - 1ull;
    const uint32_t sj = wave::read_lane(s, j), tj = wave::read_lane(t, j);
    const uint32_t first = wave::read_lane(a, j) + (sj - wave::read_lane(t0, j));
    const uint64_t base = ((uint64_t(wave::read_lane(T.ent_hi, j)) << 32) | wave::read_lane(T.ent_lo, j)) +
                          4ull * first;
    const float cs = wave::read_lane_f(T.cs, j);
    const uint32_t mode = wave::read_lane(T.mode, j);
    const uint32_t tabofs = mode & kJoinTabMask;
    const int form = join_form(mode);
    if (mode & kWideConst) wide_run<kWConst>(lds, base, tj - sj, cs, 0u, lane);
    else if (form == kJTable) wide_run<kJTable>(lds, base, tj - sj, cs, tabofs, lane);
    else if (form == kJRcp) wide_run<kJRcp>(lds, base, tj - sj, cs, tabofs, lane);
    else wide_run<kJSqrt>(lds, base, tj - sj, cs, tabofs, lane);
  }
}

// The ranges of `ntile` tiles of the unit — tile i is first + i * step — for every term, to LDS
__device__ __forceinline__ void wide_ranges(unsigned char* smem, const DevQuery& qd, uint32_t first,
                                            uint32_t step, uint32_t ntile) {
  uint32_t* row_a = reinterpret_cast<uint32_t*>(smem + WideOff::row_a);
  uint32_t* row_n = reinterpret_cast<uint32_t*>(smem + WideOff::row_n);
  for (uint32_t e = threadIdx.x; e < ntile * kMaxWideTerms; e += blockDim.x) {
    const uint32_t i = e / kMaxWideTerms, j = e % kMaxWideTerms;
    uint32_t a = 0, n = 0;
    if (j < qd.n_terms) {
      const uint32_t* bnd = reinterpret_cast<const uint32_t*>(
          reinterpret_cast<const JoinTerm*>(smem + WideOff::jts)[j].bounds);
      const uint32_t tile = first + i * step;
      a = bnd[tile];
      n = bnd[tile + 1u] - a;
    }
    row_a[e] = a;
    row_n[e] = n;
  }
}

__device__ __forceinline__ void wide_clear(unsigned char* smem) {
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem + WideOff::acc);
  for (uint32_t i = threadIdx.x; i < kJoinTile + 64u; i += blockDim.x) acc[i] = 0ull;   // (+ the dummies)
}

// One workgroup per unit scores the tiles {phase, phase + P, ...} and picks the threshold bin
// (k_join_pilot: same histogram, same rule; a threshold of its own whatever the batch's groups).
__global__ void __launch_bounds__(kWideThreads)
k_wide_pilot(const uint32_t* units, const DevQuery* queries, const DevQTerm* qterms,
             const JoinTerm* jterms, uint32_t stride, uint32_t* bstar, uint32_t margin,
             const uint32_t* min_bin) {
  RT_DYN_SMEM(smem);
  if (!wave::lds_is_at_zero(smem)) __builtin_trap();
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem + WideOff::acc);
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem + WideOff::end);   // [kBins]
  const uint32_t* row_a = reinterpret_cast<const uint32_t*>(smem + WideOff::row_a);
  const uint32_t* row_n = reinterpret_cast<const uint32_t*>(smem + WideOff::row_n);
  const uint32_t tid = threadIdx.x;
  const unsigned lane = tid & 63u;
  const uint32_t wv = wave::uniform(tid >> 6);
  const uint32_t q = units[blockIdx.x];
  const DevQuery qd = queries[q];
  const uint32_t n_tiles = qd.n_tiles;
  const uint32_t need_matches = query_need(qd.op);
  for (uint32_t i = tid; i < kBins; i += blockDim.x) hist[i] = 0u;
  wide_clear(smem);
  __syncthreads();
  wide_prologue(smem, qd, qterms, jterms);
  const JoinLane T = wide_lane(smem, lane);
  const uint32_t first_tile = (q * 7u) % stride;
  const uint32_t sampled = first_tile < n_tiles ? (n_tiles - first_tile + stride - 1) / stride : 0u;
  for (uint32_t s0 = 0; s0 < sampled; s0 += kWideChunkTiles) {
    const uint32_t ns = sampled - s0 < kWideChunkTiles ? sampled - s0 : kWideChunkTiles;
    __syncthreads();   // (the previous pass is through with the rows)
    wide_ranges(smem, qd, first_tile + s0 * stride, stride, ns);
    __syncthreads();
    for (uint32_t u = 0; u < ns; ++u) {
      wide_tile(smem, T, row_a[u * kMaxWideTerms + lane], row_n[u * kMaxWideTerms + lane], wv, lane);
      __syncthreads();
      for (uint32_t i = tid; i < kJoinTile; i += blockDim.x) {
        const unsigned long long v = acc[i];
        if (!v) continue;
        acc[i] = 0ull;
        if ((v & kWideCountMask) >= need_matches)
          atomicAdd(&hist[score_bin(from_fixed<unsigned long long>(v & ~kWideCountMask, qd.fx_inv), qd.bin_scale)], 1u);
      }
      __syncthreads();
    }
  }
  uint32_t need = qd.k;
  if (margin) {
    const uint64_t est = (uint64_t(margin) * qd.k * sampled + n_tiles - 1) / (n_tiles ? n_tiles : 1u);
    const uint32_t lo = est < kPilotMinSample ? kPilotMinSample : uint32_t(est < 0xFFFFFFFFull ? est : 0xFFFFFFFFull);
    need = lo < qd.k ? lo : qd.k;
  }
  if (tid < 64) {   // suffix search: lane L owns the 8 bins of chunk 63-L (k_pilot)
    const uint32_t chunk = 63u - lane;
    uint32_t s = 0;
    for (uint32_t i = 0; i < kBins / 64; ++i) s += hist[chunk * (kBins / 64) + i];
    const uint32_t incl = wave::inclusive_scan(s);
    const uint64_t reach = wave::ballot(incl >= need);
    uint32_t result = 0;
    if (reach) {
      const int src = __builtin_ctzll(reach);
      const uint32_t above = wave::bcast(incl - s, src);
      const uint32_t c = 63u - uint32_t(src);
      uint32_t cum = above;
      for (int i = int(kBins / 64) - 1; i >= 0; --i) {
        cum += hist[c * (kBins / 64) + uint32_t(i)];
        if (cum >= need) { result = c * (kBins / 64) + uint32_t(i); break; }
      }
    }
    if (lane == 0) bstar[q] = (min_bin && min_bin[q] > result) ? min_bin[q] : result;
  }
}

struct WideArgs {
  const uint32_t* units;
  const DevQuery* queries;
  const DevQTerm* qterms;
  const JoinTerm* jterms;
  const uint32_t* bstar;
  uint64_t* cands;
  uint32_t* cand_count;
  unsigned long long* hits;
  uint32_t cpq;           // chunks per unit
  uint32_t chunk_tiles;   // tiles per chunk, <= kWideChunkTiles: the units' tiles cut evenly
  uint32_t cand_cap;
};

// One workgroup per (unit, chunk).  Per tile: every wavefront accumulates its share; barrier; the
// epilogue reads and clears the 64-bit words, counts the docs held by enough terms, compares them
// with the fixed-point image of the threshold bin's lower edge and applies the exact bin test to
// the few that pass (join_tiles' candidate()); barrier.  Every candidate is counted, also those the
// unit's buffer has no room for: k_select's overflow recovery sizes the re-run by that count.
__global__ void __launch_bounds__(kWideThreads)
k_wide_score(const WideArgs a) {
  RT_DYN_SMEM(smem);
  if (!wave::lds_is_at_zero(smem)) __builtin_trap();
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem + WideOff::acc);
  const uint32_t* row_a = reinterpret_cast<const uint32_t*>(smem + WideOff::row_a);
  const uint32_t* row_n = reinterpret_cast<const uint32_t*>(smem + WideOff::row_n);
  uint64_t* lc = reinterpret_cast<uint64_t*>(smem + WideOff::cand);
  uint32_t* vars = reinterpret_cast<uint32_t*>(smem + WideOff::vars);
  const uint32_t tid = threadIdx.x;
  const unsigned lane = tid & 63u;
  const uint32_t wv = wave::uniform(tid >> 6);
  const uint32_t q = a.units[blockIdx.x / a.cpq];
  const uint32_t tile0 = (blockIdx.x % a.cpq) * a.chunk_tiles;
  const DevQuery qd = a.queries[q];
  if (tile0 >= qd.n_tiles) return;   // (the whole workgroup: a unit with fewer tiles, an empty unit)
  const uint32_t ntile = qd.n_tiles - tile0 < a.chunk_tiles ? qd.n_tiles - tile0 : a.chunk_tiles;
  const uint32_t cap = a.cand_cap;
  wide_clear(smem);
  if (tid < 16u) vars[tid] = 0u;
  __syncthreads();
  wide_prologue(smem, qd, a.qterms, a.jterms);
  wide_ranges(smem, qd, tile0, 1u, ntile);
  __syncthreads();
  const JoinLane T = wide_lane(smem, lane);
  const uint32_t need = query_need(qd.op);
  const uint32_t bs = a.bstar[q];
  const unsigned long long thr = bin_threshold<unsigned long long>(bs, qd);
  uint32_t my_hits = 0;
  for (uint32_t u = 0; u < ntile; ++u) {
    wide_tile(smem, T, row_a[u * kMaxWideTerms + lane], row_n[u * kMaxWideTerms + lane], wv, lane);
    __syncthreads();   // every accumulation of the tile has landed
    const uint32_t doc0 = kDocMin + (tile0 + u) * kJoinTile;
    for (uint32_t i = tid; i < kJoinTile; i += blockDim.x) {
      const unsigned long long v = acc[i];
      if (!v) continue;
      acc[i] = 0ull;
      if ((v & kWideCountMask) < need) continue;   // only docs held by enough terms exist
      ++my_hits;
      if (v < thr) continue;   // (v, its count included, bounds the sum from above)
      // a sum that is all count scores 0 (zero boosts)
      const float score = from_fixed<unsigned long long>(v & ~kWideCountMask, qd.fx_inv);
      if (score_bin(score, qd.bin_scale) >= bs) {
        const uint64_t key = make_key(score, doc0 + i);
        const uint32_t slot = atomicAdd(&vars[kWNc], 1u);
        if (slot < kWideCands) {
          lc[slot] = key;
        } else {   // rarer: more candidates in one chunk than staging slots
          const uint32_t g = atomicAdd(&a.cand_count[q], 1u);
          if (g < cap) a.cands[uint64_t(q) * cap + g] = key;
        }
      }
    }
    __syncthreads();   // the accumulators are clear again
  }
  my_hits = wave::reduce_add(my_hits);
  if (lane == 0 && my_hits) atomicAdd(&a.hits[q], static_cast<unsigned long long>(my_hits));
  if (tid == 0) {
    const uint32_t raw = vars[kWNc];
    const uint32_t n = raw < kWideCands ? raw : kWideCands;
    vars[kWNc] = n;
    vars[kWBase] = n ? atomicAdd(&a.cand_count[q], n) : 0u;
  }
  __syncthreads();
  const uint32_t n = vars[kWNc], gbase = vars[kWBase];
  uint64_t* out = a.cands + uint64_t(q) * cap;
  for (uint32_t i = tid; i < n; i += blockDim.x) {
    const uint32_t g = gbase + i;
    if (g < cap) out[g] = lc[i];
  }
}

}  // namespace irs_hip
