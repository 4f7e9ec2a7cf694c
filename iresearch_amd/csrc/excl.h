// excl.h — the doc masks of units with excluded terms (IRS_HIP_EXCLUDE: irs::Not under an And,
// boolean_query.cpp:121-141 — exclusion(incl, disjunction(excluded)), exclusion.hpp) and of units
// restricted to a doc set (irs_hip_batch_set_doc_sets: the unscored child of a conjunction —
// bitset_doc_iterator.hpp, left out of the score by MakeConjunction, conjunction.hpp:461-467).
// Either is a per-unit deletion: a unit's mask is its segment's deleted docs plus every doc of its
// excluded terms plus every doc that is not in its set, laid out like DevSegment::dead (bit
// doc - kDocMin, padded the same), and the kernels that decide a unit's matches test
// DevQuery::dead instead of the segment's.
//
//   k_excl_mask   every distinct mask of a run in one launch: a workgroup per (mask, doc slice)
//                 builds its slice in LDS and writes each word once
//   k_tile_live   per (work-item unit, doc tile) of a batch with doc sets: does the tile hold a
//                 doc the unit's mask leaves?  (k_items_*, k_pilot and k_score skip the others)
#pragma once
#include "kernels.h"

namespace irs_hip {

// Words of a bitmap laid out like DevSegment::dead: bit (doc - kDocMin); a whole doc tile behind the
// last doc stays readable (the tile kernels test their accumulators' docs group by group)
inline uint64_t dead_words(uint32_t num_docs) { return (uint64_t(num_docs) + 12288u + 31u) / 32u + 16u; }

constexpr uint32_t kExclSliceWords = 8192;   // 32 KB of LDS per workgroup: 262144 docs, five per CU

// One distinct mask: (segment, doc set, excluded terms), terms[first .. first + n) of the launch's list
struct ExclMask {
  uint32_t* out;          // words of the mask
  const uint32_t* dead;   // the segment's deleted docs (null: none), `words` words like `out`
  // the unit's doc set (null: unrestricted): 64-bit little-endian words, bit = doc id
  // (irs_hip_bit_union's layout), set_words of them — 64 * set_words > the segment's num_docs
  const uint64_t* set;
  uint64_t set_words;
  uint64_t words;
  uint32_t seg;
  uint32_t first;
  uint32_t n;
  uint32_t num_docs;      // of the segment (a restricted mask: every bit behind it is set)
};
static_assert(sizeof(ExclMask) == 56, "ExclMask: 56 bytes");

// Word w of a doc set re-laid like DevSegment::dead: bit j = doc 32 w + j + kDocMin, i.e. bits
// [32 w + kDocMin, 32 w + kDocMin + 32) of the set's bit string — a funnel shift by kDocMin across
// two of its 32-bit halves (match.h's last loop does the inverse); halves behind the set read as 0
static_assert(kDocMin >= 1u && kDocMin < 32u, "the re-laying shifts by kDocMin bits");
__device__ __forceinline__ uint32_t set_word32(const uint64_t* set, uint64_t set_words, uint64_t w) {
  auto half = [&](uint64_t h) {
    return (h >> 1) < set_words ? uint32_t(set[h >> 1] >> (32u * uint32_t(h & 1u))) : 0u;
  };
  return (half(w) >> kDocMin) | (half(w + 1u) << (32u - kDocMin));
}

// Workgroup g: mask g / slices, doc slice g % slices of `slice_words` words (dynamic LDS).
// The slice starts from the segment's deleted docs — of a restricted unit: dead | ~set, and all
// ones behind the segment's last doc (whoever reads a whole last tile finds nothing there); each
// excluded term's blocks that overlap the
// slice (binary search on blk_last, as k_plan does) are decoded a wavefront per block, and its
// tail / single doc gone through, their docs set with LDS atomics; then every word goes out once.
// No global atomics: those execute at the memory side, uncached.
template<int LAYOUT>
__global__ void __launch_bounds__(kThreads)
k_excl_mask(const DevSegment* segs, const ExclMask* masks, const uint32_t* terms, uint32_t slices,
            uint32_t slice_words) {
  RT_DYN_SMEM(smem);
  uint32_t* bm = reinterpret_cast<uint32_t*>(smem);
  const unsigned lane = threadIdx.x & 63u;
  const uint32_t wv = wave::uniform(threadIdx.x >> 6);
  const ExclMask m = masks[blockIdx.x / slices];
  const uint64_t w0 = uint64_t(blockIdx.x % slices) * slice_words;
  if (w0 >= m.words) return;   // (a mask of a smaller segment: fewer slices)
  const uint32_t nw = m.words - w0 < slice_words ? uint32_t(m.words - w0) : slice_words;
  if (m.set) {   // (workgroup-uniform)
    for (uint32_t i = threadIdx.x; i < nw; i += kThreads) {
      const uint64_t w = w0 + i;
      // bits of docs behind num_docs: bit j of word w is doc 32 w + j + kDocMin, so the word's first
      // `in` bits are docs of the segment
      const uint64_t docs = uint64_t(m.num_docs) + 1u - kDocMin;   // bits that are docs, all words
      const uint64_t in = docs > 32u * w ? docs - 32u * w : 0u;
      const uint32_t behind = in >= 32u ? 0u : ~((1u << uint32_t(in)) - 1u);
      bm[i] = (m.dead ? m.dead[w] : 0u) | ~set_word32(m.set, m.set_words, w) | behind;
    }
  } else {
    for (uint32_t i = threadIdx.x; i < nw; i += kThreads) bm[i] = m.dead ? m.dead[w0 + i] : 0u;
  }
  __syncthreads();
  const DevSegment& seg = segs[m.seg];
  // docs of the slice: bits [w0 * 32, (w0 + nw) * 32) = docs [lo, hi]
  const uint64_t lo64 = w0 * 32u + kDocMin, hi64 = lo64 + uint64_t(nw) * 32u - 1u;
  const uint32_t lo = lo64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(lo64);
  const uint32_t hi = hi64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(hi64);
  auto mark = [&](uint32_t doc) {
    if (doc >= lo && doc <= hi) {
      const uint32_t j = doc - lo;
      atomicOr(&bm[j >> 5], 1u << (j & 31u));
    }
  };
  for (uint32_t i = 0; i < m.n; ++i) {
    const DevTerm t = seg.terms[terms[m.first + i]];
    const uint32_t* last = seg.blk_last + t.dir_off;
    // blocks [b0, b1): the first whose last doc reaches lo, through the first whose last doc
    // reaches hi (every later block starts behind hi)
    uint32_t a = 0, b = t.nblk;
    while (a < b) {
      const uint32_t c = (a + b) >> 1;
      if (last[c] < lo) a = c + 1; else b = c;
    }
    const uint32_t b0 = a;
    b = t.nblk;
    while (a < b) {
      const uint32_t c = (a + b) >> 1;
      if (last[c] < hi) a = c + 1; else b = c;
    }
    const uint32_t b1 = a < t.nblk ? a + 1u : t.nblk;
    for (uint32_t k = b0 + wv; k < b1; k += kWaves) {
      const uint64_t e = t.dir_off + k;
      const uint32_t base = k ? seg.blk_last[e - 1] : kDocMin;
      uint32_t d0, d1, f0, f1;
      decode_block<LAYOUT, false>(seg.doc + t.doc_start + seg.blk_off[e], seg.blk_bits[e] & 0xFFu,
                                  0, base, lane, d0, d1, f0, f1);
      mark(d0);
      mark(d1);
    }
    // the decoded vint tail (or the single doc): at most 127 docs, all behind the last block
    const uint32_t n = t.docs_count == 1 ? 1u : t.tail_n;
    if (n && (t.nblk == 0 || last[t.nblk - 1] < hi))
      for (uint32_t j = threadIdx.x; j < n; j += kThreads) mark(seg.tail_docs[t.tail_row + j]);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < nw; i += kThreads) m.out[w0 + i] = bm[i];
}

// One wavefront per (unit, doc tile) of the units that run as work items, grid = n_units * tb
// workgroups, tb = ceil(max tiles / kWaves) — k_items_fill's geometry.  live[tile_base + tile] = 1:
// the tile holds a doc the unit's mask leaves (always, for a unit without a doc set: `restricted`
// is [unit] bytes); 0: nothing in the tile can match — no work items, no visit.  The mask's bits
// behind the segment's last doc are set (k_excl_mask), and its words reach a whole tile behind it
// (dead_words).
__global__ void __launch_bounds__(kThreads)
k_tile_live(const DevQuery* queries, const uint8_t* restricted, uint32_t tile_docs, uint32_t tb,
            uint8_t* live) {
  const unsigned lane = threadIdx.x & 63u;
  const uint32_t unit = blockIdx.x / tb;
  const uint32_t tile = (blockIdx.x % tb) * kWaves + wave::uniform(threadIdx.x >> 6);
  const DevQuery qd = queries[unit];
  if (tile >= qd.n_tiles || qd.first_off == kNoPlan) return;   // whole wavefront
  bool any = !restricted[unit] || !qd.dead;
  if (!any) {
    const uint32_t tw = tile_docs / 32u;
    const uint32_t* w = qd.dead + uint64_t(tile) * tw;
    for (uint32_t i = lane; i < tw; i += 64u) any = any || w[i] != 0xFFFFFFFFu;
  }
  const bool some = wave::ballot(any) != 0;
  if (lane == 0) live[qd.tile_base + tile] = some ? 1u : 0u;
}

}  // namespace irs_hip
