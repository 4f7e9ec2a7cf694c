// conj_any.h — irs::And whose children are Ors of by_term (IRS_HIP_GROUP_ALT): a block-driven
// conjunction of disjunctions.
//
// Reference: And::prepare / AndQuery -> make_conjunction over the children's iterators, an Or child
// being its own make_disjunction (boolean_filter.cpp:150-210, boolean_query.cpp:60-145).  Groups
// G_0..G_n-1 (a plain by_term child is a group of one); per doc
//   d matches iff every group has a member holding d (and d is not masked: DevQuery::dead);
//   s_g(d) = sum of the scores of the members of G_g holding d (the inner Or merges with SUM);
//   score(d) = the And's merge (SUM / MAX / MIN) over s_g(d), groups in cost order.
//
// The rows of a unit (DevQuery::n_terms <= kVarRows) are the present members, group after group,
// the groups sorted by the sum of their members' docs_count at create; bit r of the unit's `opens`
// word is set when row r opens a group.  The scheme of k_vphrase (vphrase.h) without positions:
//   - the ITERATION LEAD is the cheapest group; its lead items are the blocks (and tails) of EVERY
//     one of its members, a wavefront each (k_vphrase_seek writes the records and start blocks);
//   - an item of lead member j owns doc d only if no lead member j' < j holds d: those are decoded
//     first and their hits leave the alive set, so every match is scored by exactly one item (a
//     one-member lead group skips this: k_conj's case);
//   - every other group's members are decoded for the alive docs (k_conj's "blocks that can hold an
//     alive doc" step), each into its own frequency row; after the group, alive = docs one of its
//     members reached.  A group that leaves nothing alive ends the item.  The lead's members after
//     j are decoded last, for the surviving docs;
//   - per surviving doc: the norm once, per group the sum of its members' scores in entry order,
//     the And's merge over the groups.
// Block-max pruning is not applied (A.wand is ignored): grouped units run exhaustively.
//
// The lead frame, the alive bitmap rebuilt from the lanes and the walk over a member's blocks are
// lead.h's.
#pragma once
#include "conj.h"
#include "vphrase.h"

namespace irs_hip {

struct AnyWave {
  uint32_t docs[kBlock];
  uint32_t tf[kVarRows][kBlock];      // frequency of the doc in row r's list (0: not held)
  alignas(16) uint8_t first[kConjBuckets];   // bucket -> 1 + entry index of its first lead doc
  uint32_t bm[kConjWords + 4];        // alive docs' buckets over [dlo, dhi]
  uint8_t apre[kConjWords + 4];       // bits of bm in the words before word w
};

template<int LAYOUT>
__device__ __forceinline__ void conj_any_item(const ConjArgs& A, const uint32_t* opens_of,
                                              uint32_t pilot, AnyWave* s_wave) {
  const uint32_t tid = threadIdx.x;
  const unsigned lane = tid & 63u;
  const uint32_t wv = wave::uniform(tid >> 6);
  const uint32_t e = lead_item_of(A, pilot, kConjWaves);
  if (e == kNoItem) return;
  const ConjItem R = wave::sload<ConjItem>(reinterpret_cast<uint64_t>(A.recs) + uint64_t(e) * sizeof(ConjItem));
  const uint32_t unit = R.unit, item = R.item & kConjItemBlock, j = (R.item >> 24) & 0xFu;
  const DevQuery qd = wave::sload<DevQuery>(reinterpret_cast<uint64_t>(A.queries) + uint64_t(unit) * sizeof(DevQuery));
  const uint32_t m = qd.n_terms;
  if (m == 0 || m > kVarRows || j >= m) return;
  const uint32_t mrg = query_merge(qd.op);
  const DevSegment& seg = A.segs[qd.seg];
  const uint64_t tl_at = reinterpret_cast<uint64_t>(A.tails) + uint64_t(unit) * A.jt * sizeof(DevTail);
  const uint64_t qt_at = reinterpret_cast<uint64_t>(A.qterms) + uint64_t(qd.first_term) * sizeof(DevQTerm);
  auto term_tail = [&](uint32_t i) { return wave::sload<DevTail>(tl_at + i * sizeof(DevTail)); };
  auto term_q = [&](uint32_t i) { return wave::sload<DevQTerm>(qt_at + i * sizeof(DevQTerm)); };
  const uint32_t opens = wave::uniform(opens_of[unit]) | 1u;
  const uint32_t lead_lo = group_lo(opens, j), lead_end = group_end(opens, j, m);
  const DevTail ld = term_tail(j);
  const uint32_t bs = pilot ? 0u : A.bstar[unit];
  AnyWave& W = s_wave[wv];
  uint32_t* docs = W.docs;
  const uint32_t* seek = A.seek + uint64_t(e) * (A.jt - 1u);

  // ---- 1. the lead item: entry index 2*lane + h (block) or lane + 64*h (tail)
  uint32_t n = kBlock;
  uint32_t bytes = 0;
  const bool counting = !pilot && A.touched != nullptr;
  uint32_t ld_d[2], ld_e[2];
  bool alive[2];   // the lane's lead entries still in the running (docs of the segment, not masked)
  {
    uint32_t f[2];
    n = lead_decode<LAYOUT>(seg, ld, R, item, lane, counting, bytes, ld_d, ld_e, f);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t idx = ld_e[h];
      docs[idx] = idx < n ? ld_d[h] : 0xFFFFFFFFu;
      alive[h] = idx < n && !(qd.dead && doc_dead(qd.dead, ld_d[h]));
      for (uint32_t i = 0; i < m; ++i) W.tf[i][idx] = (i == j && alive[h]) ? f[h] : 0u;
    }
    lead_first_clear(W.first, lane);
  }
  wave::sync();
  if (n == 0) return;
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

  // ---- 2. one row: the blocks of its list that can hold an alive doc (k_conj step 2), decoded; a
  // posting on a lead doc leaves its frequency in the row at the doc's entry
  auto decode_row = [&](uint32_t i) {
    const DevTail tl = term_tail(i);
    auto put = [&](uint32_t doc, uint32_t f) {
      const uint32_t x = doc - fr.dlo;
      if (f == 0 || x > fr.span) return;
      const uint32_t t = lead_index(W.first, docs, n, x >> fr.s, fr.s, doc);
      if (t == n) return;
      W.tf[i][t] = f;
    };
    follow_list<LAYOUT, false, false>(seg, tl, seek[i < j ? i : i - 1u], fr, W.bm, W.apre, counting, bytes,
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
  // b. every other group, cheapest first: alive = docs one of its members holds
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
  // c. the lead members behind j: their frequencies on the surviving docs
  if (j + 1u < lead_end) {
    if (rebuild() == 0u) return quit();
    for (uint32_t r = j + 1u; r < lead_end; ++r) decode_row(r);
    wave::sync();
  }

  // ---- 3. surviving docs, compacted: scored, into the histogram (pilot) / the candidate list
  const uint64_t below = (1ull << lane) - 1ull;
  const uint64_t m0 = wave::ballot(alive[0]), m1 = wave::ballot(alive[1]);
  const uint32_t c0 = uint32_t(__builtin_popcountll(m0));
  const uint32_t total = c0 + uint32_t(__builtin_popcountll(m1));
  uint8_t* list = W.first;   // (the bucket table has served)
  wave::sync();
  if (alive[0]) list[__builtin_popcountll(m0 & below)] = uint8_t(ld_e[0]);
  if (alive[1]) list[c0 + uint32_t(__builtin_popcountll(m1 & below))] = uint8_t(ld_e[1]);
  wave::sync();
  if (counting && needs_norm(term_q(0).kind)) bytes += total * seg.norm_width;
  for (uint32_t q0 = 0; q0 < total; q0 += 64) {
    bool cand = false;
    float v = 0.f;
    uint32_t doc = 0;
    if (q0 + lane < total) {
      const uint32_t sl = list[q0 + lane];
      doc = docs[sl];
      const uint32_t nv = !seg.pnorm ? norm_value(seg, doc)
                          : (item < ld.nblk ? seg.pnorm[(ld.dir_off + item) * kBlock + sl]
                                            : seg.tail_norms[ld.tail_row + sl]);
      for (uint32_t lo = 0; lo < m;) {
        const uint32_t end = group_end(opens, lo, m);
        float g = 0.f;
        for (uint32_t r = lo; r < end; ++r) {
          const uint32_t f = W.tf[r][sl];
          if (f) g += score_value(term_q(r), f, nv);
        }
        v = merge_scores(mrg, lo == 0u, v, g);
        lo = end;
      }
      const uint32_t bin = score_bin(v, qd.bin_scale);
      if (pilot) atomicAdd(&A.hist[uint64_t(unit) * kBins + bin], 1u);
      else cand = bin >= bs;
    }
    emit_candidates(A, unit, cand, v, doc, lane);
  }
  if (pilot) return;
  if (lane == 0 && total) A.item_hits[e] = total;
  if (counting && lane == 0) atomicAdd(&A.touched[2u * unit], static_cast<unsigned long long>(bytes));
}

// 4 wavefronts x ~9.7 KB of rows (16 frequency rows of 128 docs each): four workgroups per CU, 4
// wavefronts per SIMD (LDS bound); 41 / 43 VGPRs (scalar / simd4), within k_conj's 64-VGPR budget
template<int LAYOUT>
__global__ void __launch_bounds__(kConjWaves * 64) RT_WAVES_PER_SIMD(4)
k_conj_any(ConjArgs A, const uint32_t* opens, uint32_t pilot) {
  __shared__ AnyWave s_wave[kConjWaves];
  conj_any_item<LAYOUT>(A, opens, pilot, s_wave);
}

}  // namespace irs_hip
