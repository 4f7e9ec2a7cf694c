// tree.h — boolean filters nested to any depth over by_term leaves (IRS_HIP_TREE_NODE): And, Or with
// min_match, Not at any level — `a AND (b OR (c AND d))`, `(a AND NOT b) OR c`, `+a +(b c d)~2`.
// And::prepare / Or::prepare prepare every child on its own (boolean_filter.cpp:55-312); an And
// becomes a conjunction with its Not children as an exclusion, an Or a disjunction or min-match
// disjunction (boolean_query.cpp:127-247, conjunction.hpp:436-490, disjunction.hpp:1411-1467,
// exclusion.hpp).  For at most 16 leaves every such tree is a function of the 16-bit PRESENCE MASK
// clauses.h keeps per doc — whether the doc matches, and which leaves score.
//
//   k_tree_pilot  scores every P-th doc tile of a unit, derives its score-bin threshold
//                 (k_clause_pilot's histogram and rule)
//   k_tree_score  four steps per tile over the streams of the unit's leaves in LDS, counts the hits,
//                 stages the candidates at or above the threshold bin; k_select follows
//
// Shaped like clauses.h and on the same helpers (wide_prologue, wide_ranges, wide_clear, wide_lane,
// the piece cutting of wide_tile, clause_run / clause_forms, lds_bits32): lane j = row j, a row per
// leaf present in the segment, negated leaves included; one workgroup of 1024 threads per unit
// (pilot) or per (unit, chunk of consecutive tiles) (score), a plain grid; the WideOff LDS layout
// and behind it the unit's node table (tree_shape.h: at most 16 records, children before parents,
// the root last).  A row carries the bit of its LEAF (DevQTerm::pad0; bit 16: the leaf is negated):
// a leaf absent from the segment is no row, keeps its bit and never sets it.
//
// Per tile:
//   1. presence: every posting of row j, negated rows included, adds its leaf's bit to the low word
//      of the doc's 64-bit sum (a stream holds a doc once: the adds never carry); barrier
//   2. evaluate: one thread per doc word with a nonzero low half walks the node table upward — which
//      nodes match — then downward from the root — which matching nodes are active — and replaces
//      the low 16 bits by the SCORING MASK: the positive leaves present under active nodes, 0 when
//      the root does not match.  A matching node has a matching positive child, so the mask is
//      nonzero exactly for hits; barrier
//   3. score: every posting of a positive row reads the word (lds_bits32) and adds fx & ~0xFFFF where
//      its leaf's bit is set — the low 16 bits of these adds are zero, the masks the other
//      wavefronts are reading stay as they are; barrier
//   4. the epilogue reads and clears the words; a doc is a hit iff its low 16 bits are nonzero; then
//      as k_clause_score does.
// A contribution loses its low 16 bits, as in clauses.h.  Postings of deleted docs carry the address
// of a dummy word (join.h): step 2 never visits it, whatever steps 1 and 3 leave there is never read
// as a doc.
#pragma once
#include "clauses.h"
#include "tree_shape.h"

namespace irs_hip {

static_assert(kTreeMaxLeaves == kMaxClauseTerms, "a leaf's bit lies in the mask clauses.h reads");

struct TreeOff {
  static constexpr uint32_t nodes = WideOff::end;   // TreeNode[kTreeMaxNodes]
  static constexpr uint32_t end = nodes + uint32_t(sizeof(TreeNode)) * kTreeMaxNodes;
};
static_assert(TreeOff::nodes % 16u == 0u, "TreeOff alignment");
static_assert(TreeOff::end + 4u * kBins <= 160u * 1024u, "one workgroup's LDS");

constexpr uint32_t kTreeNegated = 1u << 16;   // DevQTerm::pad0 of a tree unit's row, next to its leaf's bit index

// The unit's node table to LDS (16 bytes per record).  Followed by a barrier at the caller's.
__device__ __forceinline__ void tree_table(unsigned char* smem, const TreeNode* nodes, uint32_t n_nodes) {
  const uint32_t tid = threadIdx.x;
  if (tid < 4u * kTreeMaxNodes) {
    const uint32_t i = tid / 4u;
    reinterpret_cast<uint32_t*>(smem + TreeOff::nodes)[tid] =
        i < n_nodes ? reinterpret_cast<const uint32_t*>(nodes)[tid] : 0u;
  }
}

// Lane j's leaf: its bit, 0 beyond the unit's rows; *positive: the leaf scores
__device__ __forceinline__ uint32_t tree_lane_bit(const unsigned char* smem, uint32_t n_terms, unsigned lane, bool* positive) {
  const uint32_t p = lane < n_terms ? reinterpret_cast<const DevQTerm*>(smem + WideOff::qts)[lane].pad0 : kTreeNegated;
  *positive = !(p & kTreeNegated);
  return lane < n_terms ? 1u << (p & 15u) : 0u;
}

// tree_shape.h tree_eval on the table in LDS (every lane reads the same records: broadcasts)
__device__ __forceinline__ uint32_t tree_scoring_mask(const unsigned char* smem, uint32_t n_nodes, uint32_t present) {
  const uint32_t* tab = reinterpret_cast<const uint32_t*>(smem + TreeOff::nodes);
  uint32_t sat = 0;
  for (uint32_t i = 0; i < n_nodes; ++i) {   // (uniform)
    const uint32_t leaves = tab[4u * i], nodes = tab[4u * i + 1u], need = (tab[4u * i + 2u] >> 8) & 0xFFu;
    const uint32_t cnt = uint32_t(__builtin_popcount(present & leaves & 0xFFFFu)) +
                         uint32_t(__builtin_popcount(sat & nodes & 0xFFFFu));
    const bool ok = cnt >= need && !(present & (leaves >> 16)) && !(sat & (nodes >> 16));
    sat |= (ok ? 1u : 0u) << i;
  }
  if (!((sat >> (n_nodes - 1u)) & 1u)) return 0u;
  uint32_t active = 1u << (n_nodes - 1u), score = 0;
  for (uint32_t i = n_nodes; i-- > 0u;) {
    if (!((active >> i) & 1u)) continue;
    score |= present & tab[4u * i] & 0xFFFFu;
    active |= sat & tab[4u * i + 1u] & 0xFFFFu;
  }
  return score;
}

// A wavefront's share of one pass over one tile, cut as wide_tile cuts it (clause_tile): PASS 1 the
// presence of every row (n = its range in the tile), PASS 3 the scores of the positive rows (the
// caller passes n = 0 for the negated ones).  `bit` per lane; read with read_lane once per run, it
// is wave-uniform there.  All 64 lanes active.
template<int PASS>
__device__ __forceinline__ void tree_tile(const unsigned char* lds, const JoinLane& T, uint32_t bit,
                                          uint32_t a, uint32_t n, uint32_t wv, unsigned lane) {
  const uint32_t c = wave::inclusive_scan(n);
  const uint32_t total = wave::read_lane(c, 63u);
  const uint32_t lo = uint32_t((uint64_t(total) * wv) >> kWideWavesLog2);
  const uint32_t hi = uint32_t((uint64_t(total) * (wv + 1u)) >> kWideWavesLog2);
  const uint32_t t0 = c - n;   // the row's first posting within the sequence
  const uint32_t s = t0 > lo ? t0 : lo, t = c < hi ? c : hi;
  uint64_t touched = wave::ballot(s < t);
  while (touched) {   // (wave-uniform)
    const uint32_t j = wave::uniform(uint32_t(__builtin_ctzll(touched)));
    touched &= touched - 1ull;
    const uint32_t sj = wave::read_lane(s, j), tj = wave::read_lane(t, j);
    const uint32_t first = wave::read_lane(a, j) + (sj - wave::read_lane(t0, j));
    const uint64_t base = ((uint64_t(wave::read_lane(T.ent_hi, j)) << 32) | wave::read_lane(T.ent_lo, j)) +
                          4ull * first;
    const uint32_t bit_j = wave::read_lane(bit, j);
    if (PASS == 1) {
      clause_run<kWConst, kCPresence>(lds, base, tj - sj, 0.f, 0u, bit_j, bit_j, lane);
    } else {
      const float cs = wave::read_lane_f(T.cs, j);
      const uint32_t mode = wave::read_lane(T.mode, j);
      clause_forms<kCScore>(lds, base, tj - sj, cs, mode, bit_j, bit_j, lane);
    }
  }
}

// Steps 1 to 3 of one tile; ends behind the barrier that lets the epilogue read the sums
__device__ __forceinline__ void tree_passes(unsigned char* smem, const JoinLane& T, uint32_t bit, bool positive,
                                            uint32_t n_nodes, uint32_t a, uint32_t n, uint32_t wv, unsigned lane) {
  tree_tile<1>(smem, T, bit, a, n, wv, lane);
  __syncthreads();   // every doc's presence mask is whole
  uint32_t* words = reinterpret_cast<uint32_t*>(smem + WideOff::acc);
  for (uint32_t i = threadIdx.x; i < kJoinTile; i += blockDim.x) {
    const uint32_t present = words[2u * i];   // (nothing has scored yet: the low word is the mask)
    if (present) words[2u * i] = tree_scoring_mask(smem, n_nodes, present & 0xFFFFu);
  }
  __syncthreads();   // every doc's scoring mask stands
  tree_tile<3>(smem, T, bit, a, positive ? n : 0u, wv, lane);
  __syncthreads();   // every accumulation of the tile has landed
}

// One workgroup per unit scores the tiles {phase, phase + P, ...} and picks the threshold bin
// (k_clause_pilot: same histogram, same rule).  `nodes`: kTreeMaxNodes records per unit of `units`.
__global__ void __launch_bounds__(kWideThreads)
k_tree_pilot(const uint32_t* units, const DevQuery* queries, const DevQTerm* qterms,
             const JoinTerm* jterms, const TreeNode* nodes, uint32_t stride, uint32_t* bstar, uint32_t margin,
             const uint32_t* min_bin) {
  RT_DYN_SMEM(smem);
  if (!wave::lds_is_at_zero(smem)) __builtin_trap();
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem + WideOff::acc);
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem + TreeOff::end);   // [kBins]
  const uint32_t* row_a = reinterpret_cast<const uint32_t*>(smem + WideOff::row_a);
  const uint32_t* row_n = reinterpret_cast<const uint32_t*>(smem + WideOff::row_n);
  const uint32_t tid = threadIdx.x;
  const unsigned lane = tid & 63u;
  const uint32_t wv = wave::uniform(tid >> 6);
  const uint32_t q = units[blockIdx.x];
  const DevQuery qd = queries[q];
  const uint32_t n_tiles = qd.n_tiles;
  const uint32_t n_nodes = query_need(qd.op);   // (1..kTreeMaxNodes: unit_run)
  for (uint32_t i = tid; i < kBins; i += blockDim.x) hist[i] = 0u;
  wide_clear(smem);
  __syncthreads();
  wide_prologue(smem, qd, qterms, jterms);
  tree_table(smem, nodes + size_t(blockIdx.x) * kTreeMaxNodes, n_nodes);
  __syncthreads();
  const JoinLane T = wide_lane(smem, lane);
  bool positive;
  const uint32_t bit = tree_lane_bit(smem, qd.n_terms, lane, &positive);
  const uint32_t first_tile = (q * 7u) % stride;
  const uint32_t sampled = first_tile < n_tiles ? (n_tiles - first_tile + stride - 1) / stride : 0u;
  for (uint32_t s0 = 0; s0 < sampled; s0 += kWideChunkTiles) {
    const uint32_t ns = sampled - s0 < kWideChunkTiles ? sampled - s0 : kWideChunkTiles;
    __syncthreads();   // (the previous pass is through with the rows)
    wide_ranges(smem, qd, first_tile + s0 * stride, stride, ns);
    __syncthreads();
    for (uint32_t u = 0; u < ns; ++u) {
      tree_passes(smem, T, bit, positive, n_nodes, row_a[u * kMaxWideTerms + lane], row_n[u * kMaxWideTerms + lane], wv, lane);
      for (uint32_t i = tid; i < kJoinTile; i += blockDim.x) {
        const unsigned long long v = acc[i];
        if (!v) continue;
        acc[i] = 0ull;
        if (v & kClauseMask)
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

struct TreeArgs {
  WideArgs w;
  const TreeNode* nodes;   // kTreeMaxNodes records per unit of w.units
};

// One workgroup per (unit, chunk): k_clause_score's grid.  Per tile the three steps, then the
// epilogue: the docs with a nonzero scoring mask exist; their sums — the mask included, so an upper
// bound — against the fixed-point image of the threshold bin's lower edge, the exact bin test for the
// few that pass.  Every candidate is counted, also those the unit's buffer has no room for: k_select's
// overflow recovery sizes the re-run by that count.
__global__ void __launch_bounds__(kWideThreads)
k_tree_score(const TreeArgs ta) {
  RT_DYN_SMEM(smem);
  if (!wave::lds_is_at_zero(smem)) __builtin_trap();
  const WideArgs& a = ta.w;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem + WideOff::acc);
  const uint32_t* row_a = reinterpret_cast<const uint32_t*>(smem + WideOff::row_a);
  const uint32_t* row_n = reinterpret_cast<const uint32_t*>(smem + WideOff::row_n);
  uint64_t* lc = reinterpret_cast<uint64_t*>(smem + WideOff::cand);
  uint32_t* vars = reinterpret_cast<uint32_t*>(smem + WideOff::vars);
  const uint32_t tid = threadIdx.x;
  const unsigned lane = tid & 63u;
  const uint32_t wv = wave::uniform(tid >> 6);
  const uint32_t slot_u = blockIdx.x / a.cpq;
  const uint32_t q = a.units[slot_u];
  const uint32_t tile0 = (blockIdx.x % a.cpq) * a.chunk_tiles;
  const DevQuery qd = a.queries[q];
  if (tile0 >= qd.n_tiles) return;   // (the whole workgroup: a unit with fewer tiles, an empty unit)
  const uint32_t ntile = qd.n_tiles - tile0 < a.chunk_tiles ? qd.n_tiles - tile0 : a.chunk_tiles;
  const uint32_t cap = a.cand_cap;
  const uint32_t n_nodes = query_need(qd.op);   // (1..kTreeMaxNodes: unit_run)
  wide_clear(smem);
  if (tid < 16u) vars[tid] = 0u;
  __syncthreads();
  wide_prologue(smem, qd, a.qterms, a.jterms);
  wide_ranges(smem, qd, tile0, 1u, ntile);
  tree_table(smem, ta.nodes + size_t(slot_u) * kTreeMaxNodes, n_nodes);
  __syncthreads();
  const JoinLane T = wide_lane(smem, lane);
  bool positive;
  const uint32_t bit = tree_lane_bit(smem, qd.n_terms, lane, &positive);
  const uint32_t bs = a.bstar[q];
  const unsigned long long thr = bin_threshold<unsigned long long>(bs, qd);
  uint32_t my_hits = 0;
  for (uint32_t u = 0; u < ntile; ++u) {
    tree_passes(smem, T, bit, positive, n_nodes, row_a[u * kMaxWideTerms + lane], row_n[u * kMaxWideTerms + lane], wv, lane);
    const uint32_t doc0 = kDocMin + (tile0 + u) * kJoinTile;
    for (uint32_t i = tid; i < kJoinTile; i += blockDim.x) {
      const unsigned long long v = acc[i];
      if (!v) continue;
      acc[i] = 0ull;
      if (!(v & kClauseMask)) continue;   // only docs the root matches exist
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
