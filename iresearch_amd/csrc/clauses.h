// clauses.h — a disjunction of clauses (IRS_HIP_CLAUSE_AND): an irs::Or whose children are by_term
// filters and irs::And filters of by_term — `(a AND b) OR c`.  Or::prepare prepares every child on
// its own (boolean_filter.cpp:150-210), an And child becomes a conjunction (boolean_query.cpp:60-145,
// conjunction.hpp:436-490), the Or a disjunction or min-match disjunction over the children
// (boolean_query.cpp:212-247, disjunction.hpp:1411-1467): a posting's score counts only if its WHOLE
// clause is on the doc.
//
//   k_clause_pilot  scores every P-th doc tile of a unit, derives its score-bin threshold
//                   (k_wide_pilot's histogram and rule)
//   k_clause_score  two passes per tile over the streams of the unit's entries in LDS, counts the
//                   hits, stages the candidates at or above the threshold bin; k_select follows
//
// Shaped like wide.h and on its helpers (wide_prologue, wide_ranges, wide_clear, wide_lane, the piece
// cutting of wide_tile): lane j = entry j, at most 16 of them; one workgroup of 1024 threads per unit
// (pilot) or per (unit, chunk of consecutive tiles) (score), a plain grid; the WideOff LDS layout and
// behind it the clause table — one 16-bit need-mask per clause: the entries it is made of.  The
// accumulators are the unit's own 64-bit fixed point (DevQuery::fx_mul / fx_inv); the low 16 bits of
// a sum are the PRESENCE MASK of the doc: bit j = entry j holds it.
//
// Per tile:
//   1. presence pass: every posting of entry j adds 1 << j to the low 32-bit word of the doc's
//      accumulator (a stream holds a doc once: the adds never carry).  An entry whose clause has no
//      other member is satisfied wherever it is: it adds its score here too, with one 64-bit add of
//      (fx & ~0xFFFF) | 1 << j, and takes no part in pass 2.
//   2. barrier
//   3. score pass: the entries of the clauses with two or more members once more (their second read
//      comes from L2 at best).  Per posting the doc's mask is read (lds_bits32: wave::lds_f32 and a
//      bit cast, lds_bits.h); where it covers the need-mask of the entry's clause, fx & ~0xFFFF is
//      added with a 64-bit add — the low 16
//      bits of these adds are zero, so the masks the other wavefronts are reading stay as they are.
//   4. barrier; the epilogue reads and clears the words, counts the clauses whose need-mask the
//      doc's mask covers — a doc that holds entries but completes no clause is no hit — and goes on
//      as k_wide_score does.
// A contribution loses its low 16 bits: 2^-45 of the unit's fixed-point range of 2^61 (wide.h's 7
// count bits: 2^-54), 16 of them 2^-41 — far below the 1e-5 the scores are held to.
// Postings of deleted docs carry the address of a dummy word (join.h): whatever both passes leave
// there is never read as a doc.
#pragma once
#include "lds_bits.h"
#include "wide.h"

namespace irs_hip {

constexpr uint32_t kMaxClauseTerms = 16;   // IRS_HIP_MAX_TERMS entries: the low 16 bits of a sum
constexpr unsigned long long kClauseMask = 0xFFFFull;
static_assert(kMaxClauseTerms <= kMaxWideTerms, "lane j = entry j on wide.h's records");

struct ClauseOff {
  static constexpr uint32_t need = WideOff::end;          // [kMaxClauseTerms] u16: the clauses' need-masks
  static constexpr uint32_t n = need + 2u * kMaxClauseTerms;   // u32: clauses
  static constexpr uint32_t end = need + 64u;
};
static_assert(ClauseOff::end + 4u * kBins <= 160u * 1024u, "one workgroup's LDS");

enum : int { kCPresence = 0, kCSingle = 1, kCScore = 2 };   // clause_run WHAT

// The need-mask of lane j's clause (DevQTerm::pad0 of a clause unit's row, units.h clause_masks; 0
// beyond the unit's entries) — per-lane state next to JoinLane's fields
__device__ __forceinline__ uint32_t clause_lane_need(const unsigned char* smem, uint32_t n_terms, unsigned lane) {
  return lane < n_terms ? reinterpret_cast<const DevQTerm*>(smem + WideOff::qts)[lane].pad0 : 0u;
}

// The clause table out of the rows' need-masks: the row that is the lowest bit of its mask opens
// its clause.  (One thread: at most 16 rows.)  Followed by a barrier at the caller's.
__device__ __forceinline__ void clause_table(unsigned char* smem, uint32_t n_terms) {
  if (threadIdx.x != 0) return;
  const DevQTerm* qts = reinterpret_cast<const DevQTerm*>(smem + WideOff::qts);
  uint16_t* tab = reinterpret_cast<uint16_t*>(smem + ClauseOff::need);
  uint32_t n = 0;
  for (uint32_t j = 0; j < n_terms && j < kMaxClauseTerms; ++j) {
    const uint32_t m = qts[j].pad0 & 0xFFFFu;
    if (m && (m & (0u - m)) == (1u << j)) tab[n++] = uint16_t(m);
  }
  *reinterpret_cast<uint32_t*>(smem + ClauseOff::n) = n;
}

// The clauses of the table that `mask` covers
__device__ __forceinline__ uint32_t clauses_covered(const unsigned char* smem, uint32_t n_clauses, uint32_t mask) {
  const uint16_t* tab = reinterpret_cast<const uint16_t*>(smem + ClauseOff::need);
  uint32_t c = 0;
  for (uint32_t i = 0; i < n_clauses; ++i) {   // (uniform)
    const uint32_t m = tab[i];
    c += (mask & m) == m ? 1u : 0u;
  }
  return c;
}

// wide_post's arithmetic (join_post's: the table row, or row 0 and the v_rcp / v_sqrt form, or the
// constant of a BM1 term) up to the 64-bit fixed point, its low 16 bits cleared
template<int FORM>
__device__ __forceinline__ unsigned long long clause_fx(const unsigned char* lds, uint32_t e, float cs, uint32_t tabofs) {
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
  return fixed_from_scaled<unsigned long long>(scaled) & ~kClauseMask;
}

// One posting of entry j (bit = 1 << j, need = its clause's mask):
//   kCPresence  the doc holds the entry
//   kCSingle    ... and the entry is its whole clause: its score with it
//   kCScore     pass 2: the score where the doc's mask covers the clause
template<int FORM, int WHAT>
__device__ __forceinline__ void clause_post(const unsigned char* lds, uint32_t e, float cs, uint32_t tabofs,
                                            uint32_t bit, uint32_t need) {
  const uint32_t at = WideOff::acc + (e >> 16) * 2u;
  if (WHAT == kCPresence) {
    wave::lds_add(lds, at, bit);
  } else if (WHAT == kCSingle) {
    wave::lds_add(lds, at, clause_fx<FORM>(lds, e, cs, tabofs) | static_cast<unsigned long long>(bit));
  } else {
    const uint32_t mask = lds_bits32(lds, at);
    if ((mask & need) == need) wave::lds_add(lds, at, clause_fx<FORM>(lds, e, cs, tabofs));
  }
}

// wide_run: `count` consecutive entries from address `base` (wave-uniform), 256 per step
template<int FORM, int WHAT>
__device__ __forceinline__ void clause_run(const unsigned char* lds, uint64_t base, uint32_t count, float cs,
                                           uint32_t tabofs, uint32_t bit, uint32_t need, unsigned lane) {
  for (uint32_t i = 0; i < count; i += 256u) {
    uint32_t e[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t at = i + 64u * k + lane;
      if (at < count) e[k] = wave::gload_u32(base, at * 4u);
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k)
      if (i + 64u * k + lane < count) clause_post<FORM, WHAT>(lds, e[k], cs, tabofs, bit, need);
  }
}

template<int WHAT>
__device__ __forceinline__ void clause_forms(const unsigned char* lds, uint64_t base, uint32_t count, float cs,
                                             uint32_t mode, uint32_t bit, uint32_t need, unsigned lane) {
  const uint32_t tabofs = mode & kJoinTabMask;
  const int form = join_form(mode);
  if (mode & kWideConst) clause_run<kWConst, WHAT>(lds, base, count, cs, 0u, bit, need, lane);
  else if (form == kJTable) clause_run<kJTable, WHAT>(lds, base, count, cs, tabofs, bit, need, lane);
  else if (form == kJRcp) clause_run<kJRcp, WHAT>(lds, base, count, cs, tabofs, bit, need, lane);
  else clause_run<kJSqrt, WHAT>(lds, base, count, cs, tabofs, bit, need, lane);
}

// A wavefront's share of one pass over one tile, cut as wide_tile cuts it: the entries of the lanes
// with n > 0, entry after entry, are one sequence; wavefront w of 16 takes its sixteenth.  PASS 1:
// every entry (n = its range in the tile); PASS 2: the caller passes n = 0 for the entries that are
// their whole clause, so the sequence — and the cut — is that of the others.  `need` per lane; read
// with read_lane once per run, it is wave-uniform there.  All 64 lanes active.
template<int PASS>
__device__ __forceinline__ void clause_tile(const unsigned char* lds, const JoinLane& T, uint32_t need,
                                            uint32_t a, uint32_t n, uint32_t wv, unsigned lane) {
  const uint32_t c = wave::inclusive_scan(n);
  const uint32_t total = wave::read_lane(c, 63u);
  const uint32_t lo = uint32_t((uint64_t(total) * wv) >> kWideWavesLog2);
  const uint32_t hi = uint32_t((uint64_t(total) * (wv + 1u)) >> kWideWavesLog2);
  const uint32_t t0 = c - n;   // the entry's first posting within the sequence
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
    const uint32_t need_j = wave::read_lane(need, j);
    const uint32_t bit = 1u << j;
    if (PASS == 2) clause_forms<kCScore>(lds, base, tj - sj, cs, mode, bit, need_j, lane);
    else if (need_j == bit) clause_forms<kCSingle>(lds, base, tj - sj, cs, mode, bit, need_j, lane);
    else clause_run<kWConst, kCPresence>(lds, base, tj - sj, 0.f, 0u, bit, need_j, lane);
  }
}

// Both passes of one tile; ends behind the barrier that lets the epilogue read the sums
__device__ __forceinline__ void clause_passes(const unsigned char* lds, const JoinLane& T, uint32_t need,
                                              uint32_t a, uint32_t n, uint32_t wv, unsigned lane) {
  clause_tile<1>(lds, T, need, a, n, wv, lane);
  __syncthreads();   // every doc's mask is whole
  const bool alone = need == (1u << (lane & 31u));
  clause_tile<2>(lds, T, need, a, alone ? 0u : n, wv, lane);
  __syncthreads();   // every accumulation of the tile has landed
}

// One workgroup per unit scores the tiles {phase, phase + P, ...} and picks the threshold bin
// (k_wide_pilot: same histogram, same rule).
__global__ void __launch_bounds__(kWideThreads)
k_clause_pilot(const uint32_t* units, const DevQuery* queries, const DevQTerm* qterms,
               const JoinTerm* jterms, uint32_t stride, uint32_t* bstar, uint32_t margin,
               const uint32_t* min_bin) {
  RT_DYN_SMEM(smem);
  if (!wave::lds_is_at_zero(smem)) __builtin_trap();
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem + WideOff::acc);
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem + ClauseOff::end);   // [kBins]
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
  clause_table(smem, qd.n_terms);
  __syncthreads();
  const JoinLane T = wide_lane(smem, lane);
  const uint32_t lane_need = clause_lane_need(smem, qd.n_terms, lane);
  const uint32_t n_clauses = *reinterpret_cast<const uint32_t*>(smem + ClauseOff::n);
  const uint32_t first_tile = (q * 7u) % stride;
  const uint32_t sampled = first_tile < n_tiles ? (n_tiles - first_tile + stride - 1) / stride : 0u;
  for (uint32_t s0 = 0; s0 < sampled; s0 += kWideChunkTiles) {
    const uint32_t ns = sampled - s0 < kWideChunkTiles ? sampled - s0 : kWideChunkTiles;
    __syncthreads();   // (the previous pass is through with the rows)
    wide_ranges(smem, qd, first_tile + s0 * stride, stride, ns);
    __syncthreads();
    for (uint32_t u = 0; u < ns; ++u) {
      clause_passes(smem, T, lane_need, row_a[u * kMaxWideTerms + lane], row_n[u * kMaxWideTerms + lane], wv, lane);
      for (uint32_t i = tid; i < kJoinTile; i += blockDim.x) {
        const unsigned long long v = acc[i];
        if (!v) continue;
        acc[i] = 0ull;
        if (clauses_covered(smem, n_clauses, uint32_t(v & kClauseMask)) >= need_matches)
          atomicAdd(&hist[score_bin(from_fixed<unsigned long long>(v & ~kClauseMask, qd.fx_inv), qd.bin_scale)], 1u);
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

// One workgroup per (unit, chunk): WideArgs, k_wide_score's grid.  Per tile the two passes, then the
// epilogue: the docs whose mask covers enough clauses exist; their sums — the mask included, so an
// upper bound — against the fixed-point image of the threshold bin's lower edge, the exact bin test
// for the few that pass.  Every candidate is counted, also those the unit's buffer has no room for:
// k_select's overflow recovery sizes the re-run by that count.
__global__ void __launch_bounds__(kWideThreads)
k_clause_score(const WideArgs a) {
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
  clause_table(smem, qd.n_terms);
  __syncthreads();
  const JoinLane T = wide_lane(smem, lane);
  const uint32_t lane_need = clause_lane_need(smem, qd.n_terms, lane);
  const uint32_t n_clauses = *reinterpret_cast<const uint32_t*>(smem + ClauseOff::n);
  const uint32_t need = query_need(qd.op);
  const uint32_t bs = a.bstar[q];
  const unsigned long long thr = bin_threshold<unsigned long long>(bs, qd);
  uint32_t my_hits = 0;
  for (uint32_t u = 0; u < ntile; ++u) {
    clause_passes(smem, T, lane_need, row_a[u * kMaxWideTerms + lane], row_n[u * kMaxWideTerms + lane], wv, lane);
    const uint32_t doc0 = kDocMin + (tile0 + u) * kJoinTile;
    for (uint32_t i = tid; i < kJoinTile; i += blockDim.x) {
      const unsigned long long v = acc[i];
      if (!v) continue;
      acc[i] = 0ull;
      // only docs that complete enough clauses exist
      if (clauses_covered(smem, n_clauses, uint32_t(v & kClauseMask)) < need) continue;
      ++my_hits;
      if (v < thr) continue;   // (v, its mask included, bounds the sum from above)
      // a sum that is all mask scores 0 (zero boosts)
      const float score = from_fixed<unsigned long long>(v & ~kClauseMask, qd.fx_inv);
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
