// nested.h — the block join: ByNestedFilter (core/search/nested_filter.{hpp,cpp}).  Child docs are
// stored in front of their parent; a child filter runs over the children; the hits are the parents
// whose block of children satisfies Match{min, max}, scored by a merge of their children's scores.
// The semantics are stated once, in include/irs_hip.h (irs_hip_batch_nested_*).
//
// A segmented reduction over doc-id space, on rows of 64-bit words (bit = doc id, irs_hip_bit_union's
// layout): the unit's child row (irs_hip_batch_match_sets' words) and its segment's parent row.
//
//   k_nested_match  a workgroup per unit streams both rows in tiles of kNestedTile words, a word a
//                   thread, low docs first.  C = child & ~parent.  Per tile: popcounts of C, a
//                   workgroup scan (the child RANK in front of every word), and for every word the
//                   rank AT the last parent of an earlier word — found with a ballot inside the
//                   wavefront, a table of the wavefronts' last parents across them, and two carries
//                   across tiles (the rank so far, the rank at the last parent seen).  Per parent
//                   bit c(p) = the rank difference; the match rule and the segment's deleted docs
//                   decide the hit.  Every output word is written once; the unit's hits and the
//                   children under its hit parents (what sizes the lists) are counted.
//   k_nested_list   the same walk from the HIGH docs down — whether a child counts is known at its
//                   parent, which comes after it: the carry is "the nearest parent above is a hit".
//                   The children under hit parents compacted to an ascending doc list; per hit parent
//                   its doc and the END of its run in that list (runs are contiguous, in doc order).
//   k_nested_merge  a lane per hit parent merges its run of child scores (irs_hip_batch_score_docs'
//                   device form made them) in doc order, float32, starting from the first child's
//                   (nested_filter.cpp:292-296, 426-436; {0, none}: from 0, :477-485); runs longer
//                   than kNestedLongRun are merged by the whole wavefront, 64 coalesced scores a
//                   step, in the same order.  Writes make_key(score, parent) for k_select.
// No global atomics on the sets (excl.h: they execute at the memory side, uncached); a unit is one
// workgroup, so its counters are plain stores too.
#pragma once
#include "kernels.h"
#include "score.h"

namespace irs_hip {

constexpr uint32_t kNestedTile = kThreads;   // 64-bit words per tile: one per thread, 16384 docs
constexpr uint32_t kNestedLongRun = 32;      // children of one hit beyond which a wavefront merges them
constexpr uint32_t kNestedNoMax = 0xFFFFFFFFu;   // IRS_HIP_NESTED_NO_MAX

struct NestedArgs {
  const DevSegment* segs;
  const uint64_t* child;     // [n_units][n_words]: irs_hip_batch_match_sets' rows
  const uint64_t* parents;   // [n_segs][n_words], the caller's
  uint64_t n_words;
  uint32_t nq_user;          // units per segment: unit = segment * nq_user + query
  uint32_t match_min, match_max;   // kNestedNoMax: no maximum (no count reaches it)
};

// Word w of a unit's rows: its parents P (bit 0 and docs above num_docs dropped), its children
// C = child & ~P, and the parents that are not deleted.  DevSegment::dead is shifted by one bit
// against the sets (bit doc - kDocMin of 32-bit words), as k_match_slice applies it; only words that
// hold a bit of a doc <= num_docs are read.
struct NestedWord {
  uint64_t p, c, live;
};
__device__ __forceinline__ NestedWord nested_word(const NestedArgs& A, const DevSegment& seg, uint32_t unit,
                                                  uint64_t w) {
  NestedWord r{0, 0, 0};
  const uint64_t num_docs = seg.num_docs, lo = w * 64u;
  if (w >= A.n_words || lo > num_docs) return r;
  uint64_t valid = ~uint64_t(0);
  if (w == 0) valid &= ~uint64_t(1);
  if (num_docs - lo < 63u) valid &= (uint64_t(2) << (num_docs - lo)) - 1u;
  r.p = A.parents[uint64_t(unit / A.nq_user) * A.n_words + w] & valid;
  r.c = A.child[uint64_t(unit) * A.n_words + w] & valid & ~r.p;
  r.live = r.p;
  if (r.p && seg.dead) {
    const uint64_t nd = (num_docs + 31u) / 32u;   // mask words that hold a doc
    const uint64_t d0 = 2u * w < nd ? seg.dead[2u * w] : 0u;
    const uint64_t d1 = 2u * w + 1u < nd ? seg.dead[2u * w + 1u] : 0u;
    const uint64_t dp = w ? seg.dead[2u * w - 1u] : 0u;   // (w > 0 and lo <= num_docs: 2w - 1 < nd)
    r.live = r.p & ~(((d0 | (d1 << 32)) << 1) | (dp >> 31));
  }
  return r;
}
__device__ __forceinline__ uint64_t bits_below(uint32_t b) { return (uint64_t(1) << b) - 1u; }   // b < 64

// Workgroup g = unit g.  sets: [n_units][n_words] or null; counts / listed: [n_units] or null — the
// unit's hit parents / the children under them (both < 2^32: they are docs of one segment).
__global__ void __launch_bounds__(kThreads)
k_nested_match(NestedArgs A, uint64_t* sets, unsigned long long* counts, unsigned long long* listed) {
  __shared__ uint32_t s_sum[kWaves];    // children of the wavefront's words
  __shared__ uint32_t s_has[kWaves];    // the wavefront's words hold a parent ...
  __shared__ uint32_t s_at[kWaves];     // ... the child rank at the last of them
  __shared__ uint32_t s_tot[2][kWaves];
  const unsigned lane = threadIdx.x & 63u;
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t unit = blockIdx.x;
  const DevSegment& seg = A.segs[unit / A.nq_user];
  uint32_t rank = 0;      // children in front of the tile
  uint32_t at_last = 0;   // the child rank at the last parent in front of the tile (none: prev(p) = 0)
  uint32_t n_hits = 0, n_listed = 0;
  const uint64_t n_tiles = (A.n_words + kNestedTile - 1u) / kNestedTile;
  for (uint64_t t = 0; t < n_tiles; ++t) {   // (uniform)
    const uint64_t w = t * kNestedTile + threadIdx.x;
    const NestedWord x = nested_word(A, seg, unit, w);
    const uint32_t nc = uint32_t(__builtin_popcountll(x.c));
    const uint32_t incl = wave::inclusive_scan(nc);
    // the rank at my word's last parent, counted from the wavefront's first word for now
    const uint32_t top = x.p ? 63u - uint32_t(__builtin_clzll(x.p)) : 0u;
    const uint32_t mine = incl - nc + uint32_t(__builtin_popcountll(x.c & bits_below(top)));
    const uint64_t has = wave::ballot(x.p != 0);
    const uint64_t below = has & bits_below(lane);
    const uint32_t src = below ? 63u - uint32_t(__builtin_clzll(below)) : lane;
    const uint32_t from = wave::bcast(mine, int(src));   // the nearest earlier word of the wavefront with a parent
    if (lane == 63u) s_sum[wv] = incl;
    if (lane == (has ? 63u - uint32_t(__builtin_clzll(has)) : 0u)) {
      s_has[wv] = has ? 1u : 0u;
      s_at[wv] = mine;
    }
    __syncthreads();
    uint32_t base = rank;   // children in front of the wavefront's first word
    for (uint32_t v = 0; v < wv; ++v) base += s_sum[v];
    uint32_t at = at_last;
    if (below) {
      at = base + from;
    } else {
      uint32_t b2 = rank;
      for (uint32_t v = 0; v < wv; ++v) {
        if (s_has[v]) at = b2 + s_at[v];
        b2 += s_sum[v];
      }
    }
    // the carries of the next tile, the same in every thread
    uint32_t b2 = rank;
    for (uint32_t v = 0; v < kWaves; ++v) {
      if (s_has[v]) at_last = b2 + s_at[v];
      b2 += s_sum[v];
    }
    rank = b2;
    // per parent bit, ascending: c(p) = rank at p - rank at prev(p)
    const uint32_t before = base + incl - nc;
    uint64_t hit = 0;
    for (uint64_t pp = x.p; pp; pp &= pp - 1u) {
      const uint32_t b = uint32_t(__builtin_ctzll(pp));
      const uint32_t r = before + uint32_t(__builtin_popcountll(x.c & bits_below(b)));
      const uint32_t c = r - at;
      at = r;
      if (c >= A.match_min && c <= A.match_max && ((x.live >> b) & 1u)) {
        hit |= uint64_t(1) << b;
        n_listed += c;
      }
    }
    n_hits += uint32_t(__builtin_popcountll(hit));
    if (sets && w < A.n_words) sets[uint64_t(unit) * A.n_words + w] = hit;
    __syncthreads();   // (the tables are rewritten by the next tile)
  }
  n_hits = wave::reduce_add(n_hits);
  n_listed = wave::reduce_add(n_listed);
  if (lane == 0u) {
    s_tot[0][wv] = n_hits;
    s_tot[1][wv] = n_listed;
  }
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t h = 0, l = 0;
    for (uint32_t v = 0; v < kWaves; ++v) {
      h += s_tot[0][v];
      l += s_tot[1][v];
    }
    if (counts) counts[unit] = h;
    if (listed) listed[unit] = l;
  }
}

// Workgroup g = unit first_unit + g of a group of units.  hit: k_nested_match's rows.  The unit's list
// is docs[offsets[unit] .. offsets[unit + 1]) and its hit parents are entries [hoff[g], hoff[g + 1])
// of pdoc / ends, both ascending; ends[i] = the list position behind the last child of hit i — its
// run starts where the hit before it ends (the unit's first: at offsets[unit]).
__global__ void __launch_bounds__(kThreads)
k_nested_list(NestedArgs A, const uint64_t* hit, uint32_t first_unit, const uint64_t* offsets,
              const uint32_t* hoff, uint32_t* docs, uint32_t* pdoc, uint32_t* ends) {
  __shared__ uint32_t s_nl[kWaves], s_nh[kWaves];   // listed children / hit parents of the wavefront's words
  __shared__ uint32_t s_has[kWaves];                // the wavefront's words hold a parent ...
  __shared__ uint32_t s_low[kWaves];                // ... the lowest of them is a hit
  const unsigned lane = threadIdx.x & 63u;
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t unit = first_unit + blockIdx.x;
  const DevSegment& seg = A.segs[unit / A.nq_user];
  uint32_t end_pos = uint32_t(offsets[unit + 1u]);   // the list is filled from its end
  uint32_t end_hit = hoff[blockIdx.x + 1u];
  uint32_t above_hit = 0;   // the nearest parent above the tile is a hit (none: such docs belong to nobody)
  const uint64_t n_tiles = (A.n_words + kNestedTile - 1u) / kNestedTile;
  for (uint64_t t = n_tiles; t-- > 0u;) {   // (uniform)
    const uint64_t w = t * kNestedTile + threadIdx.x;
    const NestedWord x = nested_word(A, seg, unit, w);
    const uint64_t h = w < A.n_words ? hit[uint64_t(unit) * A.n_words + w] & x.p : 0u;
    const bool low = x.p && ((h >> uint32_t(__builtin_ctzll(x.p | (uint64_t(1) << 63)))) & 1u);
    const uint64_t has = wave::ballot(x.p != 0);
    const uint64_t lows = wave::ballot(low);
    if (lane == 0u) {
      s_has[wv] = has ? 1u : 0u;
      s_low[wv] = has ? uint32_t((lows >> uint32_t(__builtin_ctzll(has))) & 1u) : 0u;
    }
    __syncthreads();
    // the hit status of the nearest parent above my word's last one
    uint32_t st = above_hit;
    const uint64_t above = lane == 63u ? 0u : has & ~bits_below(lane + 1u);
    if (above) {
      st = uint32_t((lows >> uint32_t(__builtin_ctzll(above))) & 1u);
    } else {
      for (uint32_t v = kWaves; v-- > wv + 1u;)
        if (s_has[v]) st = s_low[v];
    }
    for (uint32_t v = kWaves; v-- > 0u;)
      if (s_has[v]) above_hit = s_low[v];   // (the next tile's carry, the same in every thread)
    // the children that count: in front of a hit parent, up to the parent before it
    uint64_t m = 0;
    uint32_t start = 0;
    for (uint64_t pp = x.p; pp; pp &= pp - 1u) {
      const uint32_t b = uint32_t(__builtin_ctzll(pp));
      if ((h >> b) & 1u) m |= bits_below(b) & ~bits_below(start);
      start = b + 1u;
    }
    if (st && start < 64u) m |= ~bits_below(start);
    const uint64_t lst = x.c & m;
    uint32_t nl = uint32_t(__builtin_popcountll(lst)), nh = uint32_t(__builtin_popcountll(h));
    uint32_t il = nl, ih = nh;
    wave::inclusive_scan2(il, ih);
    if (lane == 63u) {
      s_nl[wv] = il;
      s_nh[wv] = ih;
    }
    __syncthreads();
    uint32_t tl = 0, th = 0, bl = 0, bh = 0;
    for (uint32_t v = 0; v < kWaves; ++v) {
      if (v == wv) {
        bl = tl;
        bh = th;
      }
      tl += s_nl[v];
      th += s_nh[v];
    }
    uint32_t pos = end_pos - tl + bl + il - nl;
    uint32_t k = end_hit - th + bh + ih - nh;
    const uint32_t word_pos = pos;
    for (uint64_t c = lst; c; c &= c - 1u) docs[pos++] = uint32_t(w * 64u) + uint32_t(__builtin_ctzll(c));
    for (uint64_t pp = h; pp; pp &= pp - 1u) {
      const uint32_t b = uint32_t(__builtin_ctzll(pp));
      pdoc[k] = uint32_t(w * 64u) + b;
      ends[k] = word_pos + uint32_t(__builtin_popcountll(lst & bits_below(b)));
      ++k;
    }
    end_pos -= tl;
    end_hit -= th;
  }
}

// SumMerger / MaxMerger / MinMerger (scorer.hpp:390-423) on the running value
__device__ __forceinline__ float nested_merge(uint32_t merge, float acc, float s) {
  if (merge == kScoreMax) return acc < s ? s : acc;
  if (merge == kScoreMin) return s < acc ? s : acc;
  return acc + s;
}

// Thread i = hit i of a group's `n_hits` (hoff[0 .. n_units], first_unit as k_nested_list's).
// keys[g * cap + j] = make_key(score, parent) for hit j of the group's unit g.  from_zero: the
// value starts from 0, not from the first child's score ({0, none}); scores == null: every hit
// scores `none_boost` ({0, 0}).
__global__ void __launch_bounds__(kThreads)
k_nested_merge(const uint32_t* hoff, uint32_t n_units, uint32_t n_hits, uint32_t first_unit,
               const uint64_t* offsets, const uint32_t* pdoc, const uint32_t* ends, const float* scores,
               uint32_t merge, uint32_t from_zero, float none_boost, uint64_t* keys, uint32_t cap) {
  const unsigned lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  const bool valid = i < n_hits;
  uint32_t g = 0, lo = 0, n = 0;
  if (valid) {
    uint32_t a = 0, b = n_units;   // the last unit whose first hit is <= i
    while (b - a > 1u) {
      const uint32_t mid = (a + b) >> 1;
      if (hoff[mid] <= i) a = mid; else b = mid;
    }
    g = a;
    lo = i == hoff[g] ? uint32_t(offsets[first_unit + g]) : ends[i - 1u];
    n = scores ? ends[i] - lo : 0u;
  }
  float v = 0.f;
  const bool is_long = n > kNestedLongRun;
  if (n && !is_long) {
    uint32_t j = 0;
    if (!from_zero) v = scores[lo + j++];
    for (; j < n; ++j) v = nested_merge(merge, v, scores[lo + j]);
  }
  // the long runs, one after the other, by the whole wavefront: the same values in the same order
  for (uint64_t todo = wave::ballot(is_long); todo; todo &= todo - 1u) {   // (uniform)
    const uint32_t l = uint32_t(__builtin_ctzll(todo));
    const uint32_t rlo = wave::read_lane(lo, l), rn = wave::read_lane(n, l);
    float acc = 0.f;
    for (uint32_t at = 0; at < rn; at += 64u) {
      const uint32_t left = rn - at < 64u ? rn - at : 64u;
      const float s = lane < left ? scores[rlo + at + lane] : 0.f;
      for (uint32_t j = 0; j < left; ++j) {
        const float sj = wave::read_lane_f(s, j);
        acc = (at == 0u && j == 0u && !from_zero) ? sj : nested_merge(merge, acc, sj);
      }
    }
    if (lane == l) v = acc;
  }
  if (valid) keys[uint64_t(g) * cap + (i - hoff[g])] = make_key(scores ? v : none_boost, pdoc[i]);
}

}  // namespace irs_hip
