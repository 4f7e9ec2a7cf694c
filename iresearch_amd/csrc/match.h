// match.h — unscored execution: the docs every unit of a batch matches, all of them, as bitsets
// (filter::prepared::execute with Scorers::kUnordered, filter.hpp:52-78 — what a SEARCH without a
// SORT, a COLLECT WITH COUNT and proxy_filter's cached bitsets run: bitset_doc_iterator.hpp).
// Nothing is scored: no frequency payload, no norm, no threshold, no candidate list.
//
//   k_match_slice   boolean units (Or, And flat or grouped, min-match): a workgroup per (unit, doc
//                   slice) builds the slice of the unit's set in LDS — k_excl_mask's scheme (excl.h)
//                   carried from "union of the excluded terms" to the unit's whole filter — and
//                   writes every output word once
//   k_phrase_match  by_phrase units: the match-only instantiation of phrase_item (phrase.h) —
//   k_phrase_and_match ... with required terms (IRS_HIP_PHRASE_REQUIRED: phrase_item's REQ form),
//   k_vphrase_match ... and of vphrase_item (vphrase.h, variadic phrases): phrase frequency > 0
//                   sets the doc's bit in the unit's zeroed row
//   k_phrases_and_match (phrases.h) several phrases in one And: every phrase's frequency > 0
//   k_phrases_or_match (phrases_or.h) several phrases in one Or: some phrase's frequency > 0, the
//                   doc set and counted by the item that owns it
#pragma once
#include "kernels.h"
#include "phrase.h"
#include "vphrase.h"
#include "phrases.h"
#include "phrases_or.h"

namespace irs_hip {

enum MatchOp : uint32_t { kMatchOr = 0, kMatchMin = 1, kMatchAnd = 2 };

// Bitmaps of one slice a workgroup keeps in LDS: the set itself; a conjunction also the current
// group's; a min-match five counter planes (counts up to kMaxTerms = 16) and the current entry's
constexpr uint32_t kMatchPlanes = 5;
static_assert(kMaxTerms < (1u << kMatchPlanes), "the counter planes hold a count of every entry");
__host__ __device__ inline uint32_t match_maps(uint32_t op) {
  return op == kMatchOr ? 1u : op == kMatchAnd ? 2u : kMatchPlanes + 1u;
}
// 32-bit words of one bitmap per workgroup (IRS_HIP_MATCH_SLICE): 131072 docs, 16 KB.  Halved
// until a workgroup's bitmaps fit kMatchLdsBytes — two workgroups share a CU's 160 KB of LDS
// whatever the filter (a min-match batch: 2048 words, 48 KB, three per CU)
constexpr uint32_t kMatchSliceWords = 4096;
constexpr uint32_t kMatchSliceMax = 8192;
constexpr uint32_t kMatchLdsBytes = 80u * 1024u - 64u;
constexpr uint32_t kMatchLdsExtra = 4u * (1u + 2u * kMaxTerms) + 12u;   // 144 bytes behind the bitmaps

// One unit as k_match_slice reads it: rows[first .. first + n_rows) are the term ordinals of its
// present included entries, in the order the scored path runs them (a conjunction's cheapest
// term / group first)
struct MatchUnit {
  const uint32_t* dead;   // DevQuery::dead: the segment's deleted docs, or the unit's exclusion mask
  uint32_t seg;
  uint32_t first;
  uint32_t n_rows;        // 0: the unit matches nothing (an absent term, an empty group)
  uint32_t op;            // MatchOp
  uint32_t need;          // kMatchMin: entries that must hold a doc
  uint32_t opens;         // kMatchAnd: bit r set = row r opens a group (a flat And: every row)
};
static_assert(sizeof(MatchUnit) == 32, "MatchUnit: 32 bytes");

// Workgroup g: unit g / slices, doc slice g % slices of `slice_words` 32-bit words of the unit's
// row of `sets` ([units][n_words] 64-bit little-endian words, bit = doc: irs_hip_bit_union's
// layout).  Dynamic LDS: match_maps(widest op of the launch) bitmaps of slice_words words +
// kMatchLdsExtra bytes (a flag, the rows' block bounds).
//   per group (Or: every row; And: a group's rows; min-match: one row) the members' blocks that
//   overlap the slice — binary search on blk_last — are decoded a wavefront per block (doc parts
//   only), tails and single docs read from tail_docs, their docs set with LDS atomics;
//   the groups are combined a word per thread: And = a running AND, left as soon as the slice is
//   empty; min-match = bit-sliced counters, ripple-carry added per entry and compared with `need`;
//   the unit's mask (bit doc - kDocMin of 32-bit words) is taken out, every word written once and
//   the slice's population added to the unit's count (zeroed by the caller).
// No global atomics on the set: those execute at the memory side, uncached (excl.h).
// The doc parts are decoded from the staged `.doc` bytes (decode_block<LAYOUT, false>, which skips
// the frequency payload), as k_excl_mask and k_bit_union do — not from the packed-payload image: that
// image is laid out for decoders that read a block's two parts together, and holds only the blocks
// whose two parts are both packed, so a doc-only reader would need both paths anyway.
template<int LAYOUT>
__global__ void __launch_bounds__(kThreads)
k_match_slice(const DevSegment* segs, const MatchUnit* units, const uint32_t* rows, uint32_t slices,
              uint32_t slice_words, uint32_t* sets32 /*null: counts only*/, uint64_t n_words,
              unsigned long long* counts /*null: sets only*/) {
  RT_DYN_SMEM(smem);
  uint32_t* maps = reinterpret_cast<uint32_t*>(smem);
  const unsigned lane = threadIdx.x & 63u;
  const uint32_t wv = wave::uniform(threadIdx.x >> 6);
  const uint32_t unit = blockIdx.x / slices;
  const MatchUnit u = units[unit];
  const uint64_t words32 = n_words * 2u;
  const uint64_t w0 = uint64_t(blockIdx.x % slices) * slice_words;
  if (w0 >= words32) return;
  const uint32_t nw = words32 - w0 < slice_words ? uint32_t(words32 - w0) : slice_words;
  // behind the bitmaps: the workgroup's "slice not empty" flag, and per row the blocks [b0, b1) of
  // its list that overlap the slice
  uint32_t* any = maps + match_maps(u.op) * slice_words;
  uint32_t* bounds = any + 1;
  const DevSegment& seg = segs[u.seg];
  // docs of the slice: bits [w0 * 32, (w0 + nw) * 32) = docs [lo, hi]
  const uint64_t lo64 = w0 * 32u, hi64 = lo64 + uint64_t(nw) * 32u - 1u;
  const uint32_t lo = lo64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(lo64);
  const uint32_t hi = hi64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(hi64);
  const uint32_t num_docs = seg.num_docs;
  auto clear = [&](uint32_t* bm) {
    for (uint32_t i = threadIdx.x; i < nw; i += kThreads) bm[i] = 0u;
  };
  // the docs of rows [r0, r1) that fall into the slice, into bm
  auto fill = [&](uint32_t* bm, uint32_t r0, uint32_t r1) {
    auto mark = [&](uint32_t doc) {
      if (doc >= lo && doc <= hi) {
        const uint32_t j = doc - lo;
        atomicOr(&bm[j >> 5], 1u << (j & 31u));
      }
    };
    for (uint32_t r = r0; r < r1; ++r) {
      const DevTerm t = seg.terms[rows[u.first + r]];
      const uint32_t* last = seg.blk_last + t.dir_off;
      const uint32_t b0 = bounds[2u * r], b1 = bounds[2u * r + 1u];
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
  };
  uint32_t* set = maps;
  clear(set);
  // the rows' directory searches side by side, a thread each (a chain of dependent loads per row:
  // one after the other they were most of a sparse slice's time)
  if (threadIdx.x < u.n_rows && lo <= num_docs) {
    const DevTerm t = seg.terms[rows[u.first + threadIdx.x]];
    const uint32_t* last = seg.blk_last + t.dir_off;
    // blocks [b0, b1): the first whose last doc reaches lo, through the first whose last doc
    // reaches hi (every later block starts behind hi)
    uint32_t a = 0, b = t.nblk;
    while (a < b) {
      const uint32_t c = (a + b) >> 1;
      if (last[c] < lo) a = c + 1; else b = c;
    }
    bounds[2u * threadIdx.x] = a;
    b = t.nblk;
    while (a < b) {
      const uint32_t c = (a + b) >> 1;
      if (last[c] < hi) a = c + 1; else b = c;
    }
    bounds[2u * threadIdx.x + 1u] = a < t.nblk ? a + 1u : t.nblk;
  }
  __syncthreads();
  if (lo <= num_docs && u.n_rows) {   // (workgroup-uniform: a slice behind the segment stays empty)
    if (u.op == kMatchOr) {
      fill(set, 0, u.n_rows);
    } else if (u.op == kMatchAnd) {
      // group after group, the cheapest first: set &= group
      uint32_t* cur = maps + slice_words;
      uint32_t r0 = 0;
      bool first = true;
      while (r0 < u.n_rows) {
        uint32_t r1 = r0 + 1u;
        while (r1 < u.n_rows && !((u.opens >> r1) & 1u)) ++r1;
        if (!first) {
          clear(cur);
          __syncthreads();
        }
        fill(first ? set : cur, r0, r1);
        if (threadIdx.x == 0) *any = 0u;
        __syncthreads();
        uint32_t left = 0;
        for (uint32_t i = threadIdx.x; i < nw; i += kThreads) {
          const uint32_t v = first ? set[i] : (set[i] & cur[i]);
          if (!first) set[i] = v;
          left |= v;
        }
        if (left) *any = 1u;
        __syncthreads();
        if (*any == 0u) break;   // no doc of the slice is in every group so far
        first = false;
        r0 = r1;
      }
    } else {
      // planes[p] bit = bit p of the number of entries that hold the doc
      uint32_t* cur = maps + kMatchPlanes * slice_words;
      for (uint32_t p = 1; p < kMatchPlanes; ++p) clear(maps + p * slice_words);
      for (uint32_t r = 0; r < u.n_rows; ++r) {
        clear(cur);
        __syncthreads();
        fill(cur, r, r + 1u);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nw; i += kThreads) {
          uint32_t c = cur[i];
#pragma unroll
          for (uint32_t p = 0; p < kMatchPlanes; ++p) {
            const uint32_t x = maps[p * slice_words + i];
            maps[p * slice_words + i] = x ^ c;
            c &= x;
          }
        }
      }
      __syncthreads();
      // count >= need, from the lowest plane up: a set need bit asks for the plane's bit and what
      // the lower planes said, a clear one is satisfied by either
      for (uint32_t i = threadIdx.x; i < nw; i += kThreads) {
        uint32_t ge = 0xFFFFFFFFu;
#pragma unroll
        for (uint32_t p = 0; p < kMatchPlanes; ++p) {
          const uint32_t x = maps[p * slice_words + i];
          ge = ((u.need >> p) & 1u) ? (x & ge) : (x | ge);
        }
        set[i] = ge;
      }
    }
  }
  __syncthreads();
  uint32_t pop = 0;
  uint32_t* out = sets32 ? sets32 + uint64_t(unit) * words32 + w0 : nullptr;
  for (uint32_t i = threadIdx.x; i < nw; i += kThreads) {
    uint32_t v = set[i];
    const uint64_t w = w0 + i;   // word w: docs [32 w, 32 w + 31], mask bits [32 w - 1, 32 w + 30]
    if (v && u.dead) v &= ~((u.dead[w] << 1) | (w ? u.dead[w - 1] >> 31 : 0u));
    if (out) out[i] = v;
    pop += uint32_t(__builtin_popcount(v));
  }
  if (counts) {
    pop = wave::reduce_add(pop);
    if (lane == 0 && pop) atomicAdd(&counts[unit], static_cast<unsigned long long>(pop));
  }
}

// by_phrase units: a wavefront per lead block as in a scored run (the records and start blocks of
// k_conj_seek / k_vphrase_seek), no pilot pass.  sets32: [units][words32] 32-bit words, zeroed;
// counts: [units], zeroed (every matching doc belongs to exactly one lead item).
template<int LAYOUT, int MT>
__global__ void __launch_bounds__(kPhraseWaves * 64)
k_phrase_match(ConjArgs A, uint32_t* sets32, uint64_t words32, unsigned long long* counts) {
  __shared__ PhraseWave<MT> s_wave[kPhraseWaves];
  phrase_item<LAYOUT, MT, true>(A, 0u, s_wave, sets32, words32, counts);
}
// ... with required terms (k_phrase_and, phrase.h): a doc must also be held by every required row
template<int LAYOUT, int MT>
__global__ void __launch_bounds__(kPhraseWaves * 64)
k_phrase_and_match(ConjArgs A, const uint32_t* n_phrase, uint32_t* sets32, uint64_t words32,
                   unsigned long long* counts) {
  __shared__ PhraseWave<MT> s_wave[kPhraseWaves];
  phrase_item<LAYOUT, MT, true, true>(A, 0u, s_wave, sets32, words32, counts, n_phrase);
}
// ... with optional terms (k_phrase_or, phrase.h): the phrase's own matches, OR-ed into rows that
// hold the optional terms' docs already (the term pass's k_match_slice wrote every word of them)
template<int LAYOUT, int MT>
__global__ void __launch_bounds__(kPhraseWaves * 64)
k_phrase_or_match(ConjArgs A, const uint32_t* n_phrase, uint32_t* sets32, uint64_t words32) {
  __shared__ PhraseWave<MT> s_wave[kPhraseWaves];
  phrase_item<LAYOUT, MT, true, kPhraseOpt>(A, 0u, s_wave, sets32, words32, nullptr, n_phrase);
}
// ... and the counts of the united rows: a workgroup per (unit, slice of 8 * kThreads words)
__global__ void __launch_bounds__(kThreads)
k_count_rows(const uint32_t* sets32, uint64_t words32, uint32_t slices, unsigned long long* counts) {
  const uint32_t unit = blockIdx.x / slices;
  const uint64_t w0 = uint64_t(blockIdx.x % slices) * (8u * kThreads);
  uint32_t pop = 0;
  for (uint32_t i = threadIdx.x; i < 8u * kThreads && w0 + i < words32; i += kThreads)
    pop += uint32_t(__builtin_popcount(sets32[uint64_t(unit) * words32 + w0 + i]));
  pop = wave::reduce_add(pop);
  if ((threadIdx.x & 63u) == 0 && pop) atomicAdd(&counts[unit], static_cast<unsigned long long>(pop));
}
template<int LAYOUT>
__global__ void __launch_bounds__(kPhraseWaves * 64)
k_vphrase_match(ConjArgs A, const uint32_t* opens, uint32_t* sets32, uint64_t words32,
                unsigned long long* counts) {
  __shared__ VPhraseWave s_wave[kPhraseWaves];
  vphrase_item<LAYOUT, true>(A, opens, 0u, s_wave, sets32, words32, counts);
}

}  // namespace irs_hip
