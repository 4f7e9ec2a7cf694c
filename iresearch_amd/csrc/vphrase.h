// vphrase.h — by_phrase with parts that stand for a set of terms (IRS_HIP_PHRASE_ALT).
//
// Reference: VariadicPrepareCollect (core/search/phrase_filter.cpp:295-432), VariadicPhraseQuery::
// execute (phrase_query.cpp:197-294) -> PhraseIterator<Conjunction of one disjunction per part,
// VariadicPhraseFrequency> (phrase_iterator.hpp:197-364).  Parts P_0..P_n-1 at offsets off_i
// (off_0 = 0); per doc
//   freq(d) = sum over t in P_0 of #{p in pos(t, d) : for every i >= 1 some u in P_i has
//             p + off_i in pos(u, d)}
// (VisitLead adds the counts of the first part's members, VisitFollower is satisfied by one member).
//
// The rows of a unit (DevQuery::n_terms <= kVarRows) are the present members, part after part;
// bit r of the unit's `opens` word is set when row r opens a part.  The block-driven scheme of
// k_phrase (phrase.h) with these changes:
//   - the ITERATION LEAD is the part with the smallest sum of docs_count (a disjunction costs the sum
//     of its members, Conjunction sorts by cost); its lead items are the blocks (and tails) of EVERY
//     one of its members, a wavefront each (k_vphrase_seek writes the records and start blocks);
//   - an item of lead member j owns doc d only if no lead member j' < j holds d: those are decoded
//     first and their hits leave the alive set, so every doc is scored by exactly one item;
//   - every other part's members are decoded for the alive docs (the same "blocks that can hold an
//     alive doc" step as k_phrase), each into its own row; after the part, alive = docs one of its
//     members reached.  The lead's members after j are decoded last, for the surviving docs;
//   - per surviving doc, one lane merges the position lists with one cursor per row (registers,
//     compile-time indexed: the loops over rows are unrolled).
// Alive sets are kept per doc in the lanes (two lead entries each); the bucket bitmap that steers
// the block selection is rebuilt from them after every step.
//
// The lead frame, the alive bitmap rebuilt from the lanes and the walk over a member's blocks are
// lead.h's.  The fixed kernels (k_phrase2 / k_phrase) keep their own text of the walk, two wanted
// blocks at a time: sharing it changed how they run (lead.h).  A batch with any variadic unit runs all
// of its phrase units here.
#pragma once
#include "phrase.h"

namespace irs_hip {

constexpr uint32_t kVarRows = 16;   // IRS_HIP_MAX_PHRASE_ENTRIES

// As k_conj_seek, for the lead items of the variadic kernel: item t of unit `unit` is block / tail
// `item` of the lead part's member in row `row` (ConjItem::item = item | row << 24); seek row: the
// start block in every other row, in row order.  lead_rows[unit] = first | end << 8 of the lead part.
__global__ void __launch_bounds__(kThreads)
k_vphrase_seek(const DevSegment* segs, const DevQuery* queries, const DevTail* tails, uint32_t jt,
               const uint32_t* units, const uint32_t* item_base /*[n_units + 1]*/, uint32_t n_units,
               const uint32_t* lead_rows, uint32_t* seek, ConjItem* recs) {
  const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= item_base[n_units]) return;
  uint32_t lo = 0, hi = n_units;   // the unit whose items hold t: last c with item_base[c] <= t
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (item_base[mid] <= t) lo = mid; else hi = mid;
  }
  const uint32_t unit = units[lo];
  const DevQuery qd = queries[unit];
  const DevSegment& seg = segs[qd.seg];
  const DevTail* tl = tails + uint64_t(unit) * jt;
  const uint32_t lr = lead_rows[unit];
  uint32_t item = t - item_base[lo], row = lr & 0xFFu;
  for (; row + 1u < (lr >> 8); ++row) {   // the member whose items hold t: blocks, then its tail
    const uint32_t k = tl[row].nblk + (tl[row].n ? 1u : 0u);
    if (item < k) break;
    item -= k;
  }
  const DevTail ld = tl[row];
  ConjItem r{};
  r.unit = unit;
  r.item = item | (row << 24);
  if (item < ld.nblk) {
    const uint64_t e = ld.dir_off + item;
    r.base = item ? seg.blk_last[e - 1] : kDocMin;
    r.r_lo = item ? r.base + 1u : kDocMin;
    r.r_hi = seg.blk_last[e];
    r.aoff = seg.blk_aoff[e];
    r.bits = seg.blk_bits[e];
    r.off = seg.blk_off[e];
  } else {
    r.r_lo = ld.first_doc;
    r.r_hi = ld.last_doc;
  }
  recs[t] = r;
  for (uint32_t i = 0; i < qd.n_terms; ++i) {
    if (i == row) continue;
    const uint32_t* last = seg.blk_last + tl[i].dir_off;
    uint32_t a = 0, b = tl[i].nblk;  // lower_bound(last, r_lo)
    while (a < b) {
      const uint32_t mid = (a + b) >> 1;
      if (last[mid] < r.r_lo) a = mid + 1; else b = mid;
    }
    seek[uint64_t(t) * (jt - 1u) + (i < row ? i : i - 1u)] = a;
  }
}

struct VPhraseWave {
  uint32_t docs[kBlock];
  uint32_t pidx[kVarRows][kBlock];    // first position number of the doc in row r's list
  uint32_t tf[kVarRows][kBlock];      // its frequency there (0: the member does not hold the doc)
  alignas(16) uint8_t first[kConjBuckets];   // bucket -> 1 + entry index of its first lead doc
  uint32_t bm[kConjWords + 4];        // alive docs' buckets over [dlo, dhi]
  uint8_t apre[kConjWords + 4];       // bits of bm in the words before word w
  DevPosTerm pt[kVarRows];
  uint32_t off[kVarRows];
};

// MATCH: as for phrase_item (phrase.h) — the surviving docs with a phrase frequency > 0 set their
// bits and count, nothing is scored
template<int LAYOUT, bool MATCH = false>
__device__ __forceinline__ void vphrase_item(const ConjArgs& A, const uint32_t* opens_of,
                                             uint32_t pilot, VPhraseWave* s_wave,
                                             uint32_t* sets32 = nullptr, uint64_t words32 = 0,
                                             unsigned long long* counts = nullptr) {
  const uint32_t tid = threadIdx.x;
  const unsigned lane = tid & 63u;
  const uint32_t wv = wave::uniform(tid >> 6);
  const uint32_t e = lead_item_of(A, pilot, kPhraseWaves);
  if (e == kNoItem) return;
  const ConjItem R = wave::sload<ConjItem>(reinterpret_cast<uint64_t>(A.recs) + uint64_t(e) * sizeof(ConjItem));
  const uint32_t unit = R.unit, item = R.item & kConjItemBlock, j = (R.item >> 24) & 0xFu;
  const DevQuery qd = wave::sload<DevQuery>(reinterpret_cast<uint64_t>(A.queries) + uint64_t(unit) * sizeof(DevQuery));
  const uint32_t m = qd.n_terms;
  if (m == 0 || m > kVarRows || j >= m) return;
  const DevSegment& seg = A.segs[qd.seg];
  const uint64_t tl_at = reinterpret_cast<uint64_t>(A.tails) + uint64_t(unit) * A.jt * sizeof(DevTail);
  auto term_tail = [&](uint32_t i) { return wave::sload<DevTail>(tl_at + i * sizeof(DevTail)); };
  const uint32_t opens = wave::uniform(opens_of[unit]) | 1u;
  const uint32_t n_parts = uint32_t(__builtin_popcount(opens));
  const uint32_t lead_lo = group_lo(opens, j), lead_end = group_end(opens, j, m);
  const uint32_t first_end = group_end(opens, 0u, m);   // rows of P_0, whose positions are counted
  const DevTail ld = term_tail(j);
  const DevQTerm qt = A.qterms[qd.first_term];  // the phrase's scorer rides on every entry
  const uint32_t bs = (MATCH || pilot) ? 0u : A.bstar[unit];
  VPhraseWave& W = s_wave[wv];
  uint32_t* docs = W.docs;
  const uint32_t* seek = A.seek + uint64_t(e) * (A.jt - 1u);
  if (lane < m) {
    const DevTail t = A.tails[uint64_t(unit) * A.jt + lane];
    W.pt[lane] = seg.pterms[t.term];
    W.off[lane] = A.qterms[qd.first_term + lane].pad0;
  }

  // ---- 1. the lead item: entry index 2*lane + h (block) or lane + 64*h (tail)
  uint32_t n = kBlock;
  uint32_t bytes = 0;
  const bool counting = !pilot && A.touched != nullptr;
  uint32_t ld_d[2], ld_e[2];
  bool alive[2];   // the lane's lead entries still in the running (docs of the segment, not masked)
  {
    uint32_t f[2], p[2];
    n = lead_decode_pos<LAYOUT>(seg, ld, R, item, lane, counting, bytes, ld_d, ld_e, f, p);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t idx = ld_e[h];
      docs[idx] = idx < n ? ld_d[h] : 0xFFFFFFFFu;
      alive[h] = idx < n && !(qd.dead && doc_dead(qd.dead, ld_d[h]));
      for (uint32_t i = 0; i < m; ++i) {
        W.pidx[i][idx] = i == j ? p[h] : 0u;
        W.tf[i][idx] = (i == j && alive[h]) ? f[h] : 0u;
      }
    }
    lead_first_clear(W.first, lane);
  }
  wave::sync();
  if (qd.dead && wave::ballot(alive[0] || alive[1]) == 0) {   // (wave-uniform) no lead doc is left
    lead_skipped(A, unit, counting, bytes, lane);
    return;
  }
  const LeadFrame fr = lead_frame(docs, n);
  lead_first_fill(fr, W.first, docs, ld_d, ld_e, n);
  // the alive bitmap from the lanes' alive entries, and its prefix counts: number of alive buckets
  auto rebuild = [&]() {
    const uint32_t left = alive_rebuild(fr, W.bm, W.apre, ld_d, alive, lane);
    wave::sync();
    return left;
  };

  // ---- 2. one row: the blocks of its list that can hold an alive doc (k_phrase step 2), decoded;
  // a posting on a lead doc leaves (P, tf) in the row at the doc's entry
  auto decode_row = [&](uint32_t i) {
    const DevTail tl = term_tail(i);
    auto put = [&](uint32_t doc, uint32_t f, uint32_t p) {
      const uint32_t x = doc - fr.dlo;
      if (f == 0 || x > fr.span) return;
      const uint32_t t = lead_index(W.first, docs, n, x >> fr.s, fr.s, doc);
      if (t == n) return;
      W.pidx[i][t] = p;
      W.tf[i][t] = f;
    };
    follow_list<LAYOUT, true, false>(seg, tl, seek[i < j ? i : i - 1u], fr, W.bm, W.apre, counting, bytes,
                                     lane, put);
  };
  auto quit = [&]() {   // no doc left: what was decoded is counted
    if (counting && lane == 0) atomicAdd(&A.touched[2u * unit], static_cast<unsigned long long>(bytes));
  };
  auto held = [&](uint32_t h, uint32_t lo, uint32_t end) {   // does a row of [lo, end) hold entry h?
    const uint32_t idx = ld_e[h] < n ? ld_e[h] : 0u;
    bool any = false;
    for (uint32_t r = lo; r < end; ++r) any = any || W.tf[r][idx] != 0u;
    return any;
  };
  // a. ownership: the lead members in front of j take the docs they hold
  if (j > lead_lo) {
    if (rebuild() == 0u) return quit();
    for (uint32_t r = lead_lo; r < j; ++r) decode_row(r);
    wave::sync();
#pragma unroll
    for (int h = 0; h < 2; ++h) alive[h] = alive[h] && !held(h, lead_lo, j);
  }
  // b. every other part: alive = docs one of its members holds
  for (uint32_t lo = 0; lo < m;) {
    const uint32_t end = group_end(opens, lo, m);
    if (lo != lead_lo) {
      if (rebuild() == 0u) return quit();
      for (uint32_t r = lo; r < end; ++r) decode_row(r);
      wave::sync();
#pragma unroll
      for (int h = 0; h < 2; ++h) alive[h] = alive[h] && held(h, lo, end);
    }
    lo = end;
  }
  // c. the lead members behind j: their positions on the surviving docs
  if (rebuild() == 0u) return quit();
  for (uint32_t r = j + 1u; r < lead_end; ++r) decode_row(r);
  wave::sync();

  // ---- 3./4. surviving docs, compacted: merge the position lists, score, emit
  const uint64_t below = (1ull << lane) - 1ull;
  const uint64_t m0 = wave::ballot(alive[0]), m1 = wave::ballot(alive[1]);
  const uint32_t c0 = uint32_t(__builtin_popcountll(m0));
  const uint32_t total = c0 + uint32_t(__builtin_popcountll(m1));
  uint8_t* list = W.first;   // (the bucket table has served)
  wave::sync();
  if (alive[0]) list[__builtin_popcountll(m0 & below)] = uint8_t(ld_e[0]);
  if (alive[1]) list[c0 + uint32_t(__builtin_popcountll(m1 & below))] = uint8_t(ld_e[1]);
  wave::sync();
  uint32_t my_hits = 0, my_pos = 0;
  DevSegment ps{};
  ps.pos = seg.pos;
  ps.pblk_off = seg.pblk_off;
  ps.pblk_bits = seg.pblk_bits;
  ps.ptail = seg.ptail;
  ps.pos_base = seg.pos_base;
  const uint32_t need = ((1u << n_parts) - 1u) & ~1u;   // every part but P_0
  for (uint32_t q0 = 0; q0 < total; q0 += 64) {
    bool cand = false;
    float score = 0.f;
    uint32_t doc = 0;
    if (q0 + lane < total) {
      const uint32_t sl = list[q0 + lane];
      uint32_t P[kVarRows], T[kVarRows], K[kVarRows], V[kVarRows];
#pragma unroll
      for (int u = 0; u < int(kVarRows); ++u) {
        const bool on = uint32_t(u) < m;
        P[u] = on ? W.pidx[u][sl] : 0u;
        T[u] = on ? W.tf[u][sl] : 0u;
      }
      uint32_t pf = 0;
      for (uint32_t a = 0; a < first_end; ++a) {   // VisitLead: the members of P_0 add up
        if (MATCH && pf) break;
        const uint32_t ta = W.tf[a][sl], pa = W.pidx[a][sl];
#pragma unroll
        for (int u = 0; u < int(kVarRows); ++u) {
          K[u] = 0u;
          V[u] = ps.pos_base;
        }
        uint32_t head = ps.pos_base;
        for (uint32_t k = 0; k < ta; ++k) {
          head += pos_delta<LAYOUT>(ps, W.pt[a], 0u, pa + k);
          ++my_pos;
          uint32_t hit = 0, open = 0;   // parts with a member at p + off / one that may still have
#pragma unroll
          for (int u = 1; u < int(kVarRows); ++u) {
            if (uint32_t(u) < first_end || uint32_t(u) >= m) continue;
            const uint32_t pb = 1u << (uint32_t(__builtin_popcount(opens & ((2u << u) - 1u))) - 1u);
            if (hit & pb) continue;     // VisitFollower: one member at the position suffices
            const uint32_t target = head + W.off[u];
            // position::seek(target) :1578-1604 (value_ invalid until the first position: K == 0)
            while ((K[u] == 0u || V[u] < target) && K[u] < T[u]) {
              V[u] += pos_delta<LAYOUT>(ps, W.pt[u], 0u, P[u] + K[u]);
              ++K[u];
              ++my_pos;
            }
            if (K[u] != 0u && V[u] == target) hit |= pb;
            else if (K[u] < T[u] || V[u] > target) open |= pb;
          }
          if (hit == need) ++pf;
          else if (((hit | open) & need) != need) break;   // a part exhausted: no later p matches
          if (MATCH && pf) break;
        }
      }
      if constexpr (MATCH) {
        if (pf) {
          doc = docs[sl];
          if (sets32) atomicOr(&sets32[uint64_t(unit) * words32 + (doc >> 5)], 1u << (doc & 31u));
          ++my_hits;
        }
      } else if (pf) {
        doc = docs[sl];
        const uint32_t nv = !seg.pnorm ? norm_value(seg, doc)
                            : (item < ld.nblk ? seg.pnorm[(ld.dir_off + item) * kBlock + sl]
                                              : seg.tail_norms[ld.tail_row + sl]);
        score = score_value(qt, pf, nv);
        const uint32_t bin = score_bin(score, qd.bin_scale);
        if (pilot) atomicAdd(&A.hist[uint64_t(unit) * kBins + bin], 1u);
        else cand = bin >= bs;
        ++my_hits;
      }
    }
    emit_candidates(A, unit, cand, score, doc, lane);
  }
  if constexpr (MATCH) {
    my_hits = wave::reduce_add(my_hits);
    if (lane == 0 && my_hits && counts) atomicAdd(&counts[unit], static_cast<unsigned long long>(my_hits));
    return;
  }
  if (pilot) return;
  my_hits = wave::reduce_add(my_hits);
  if (lane == 0 && my_hits) A.item_hits[e] = my_hits;
  if (A.touched) {
    my_pos = wave::reduce_add(my_pos);
    if (lane == 0) {
      atomicAdd(&A.touched[2u * unit], static_cast<unsigned long long>(bytes));
      if (my_pos) atomicAdd(&A.touched[2u * unit + 1u], static_cast<unsigned long long>(my_pos));
    }
  }
}

// 4 wavefronts x ~18.6 KB of rows: two workgroups per CU (LDS bound)
template<int LAYOUT>
__global__ void __launch_bounds__(kPhraseWaves * 64)
k_vphrase(ConjArgs A, const uint32_t* opens, uint32_t pilot) {
  __shared__ VPhraseWave s_wave[kPhraseWaves];
  vphrase_item<LAYOUT>(A, opens, pilot, s_wave);
}

}  // namespace irs_hip
