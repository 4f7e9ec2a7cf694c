// excl.h — the doc masks of units with excluded terms (IRS_HIP_EXCLUDE: irs::Not under an And,
// boolean_query.cpp:121-141 — exclusion(incl, disjunction(excluded)), exclusion.hpp).
// An exclusion is a per-unit deletion: a unit's mask is its segment's deleted docs plus every
// doc of its excluded terms, laid out like DevSegment::dead (bit doc - kDocMin, padded the same),
// and the kernels that decide a unit's matches test DevQuery::dead instead of the segment's.
//
//   k_excl_mask   every distinct mask of a run in one launch: a workgroup per (mask, doc slice)
//                 builds its slice in LDS and writes each word once
#pragma once
#include "kernels.h"

namespace irs_hip {

// Words of a bitmap laid out like DevSegment::dead: bit (doc - kDocMin); a whole doc tile behind the
// last doc stays readable (the tile kernels test their accumulators' docs group by group)
inline uint64_t dead_words(uint32_t num_docs) { return (uint64_t(num_docs) + 12288u + 31u) / 32u + 16u; }

constexpr uint32_t kExclSliceWords = 8192;   // 32 KB of LDS per workgroup: 262144 docs, five per CU

// One distinct mask: (segment, excluded terms), terms[first .. first + n) of the launch's list
struct ExclMask {
  uint32_t* out;          // words of the mask
  const uint32_t* dead;   // the segment's deleted docs (null: none), `words` words like `out`
  uint64_t words;
  uint32_t seg;
  uint32_t first;
  uint32_t n;
  uint32_t pad;
};

// Workgroup g: mask g / slices, doc slice g % slices of `slice_words` words (dynamic LDS).
// The slice starts from the segment's deleted docs; each excluded term's blocks that overlap the
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
  for (uint32_t i = threadIdx.x; i < nw; i += kThreads) bm[i] = m.dead ? m.dead[w0 + i] : 0u;
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

}  // namespace irs_hip
