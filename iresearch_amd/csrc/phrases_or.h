// phrases_or.h — Or([by_phrase, by_phrase...]): several phrases in one disjunction
// (IRS_HIP_PHRASE_OR; the reference: Or::prepare prepares every child on its own,
// boolean_filter.cpp:150-210; MakeDisjunction -> basic_disjunction for two PhraseIterators,
// small_disjunction for up to five, disjunction.hpp:1411-1467, :208-350, :374-).
//
// The rows of a unit are the words of its PRESENT phrases, phrase after phrase (a phrase with a word
// the segment lacks has no rows: units.h); bit r of the unit's `opens` word = row r opens a phrase
// (bit 0 always).  The same term may stand in several rows ("a b" next to "b a", one phrase twice,
// two phrases led by the same word): every row has its own (P, tf) row in LDS, its own seek column —
// nothing here is keyed by term.
//
// EVERY PHRASE LEADS with its own rarest word: the unit's lead items are the blocks (plus tail or
// single doc) of every phrase's lead row, the row in ConjItem::item as k_vphrase_seek writes it
// (item | row << 24); bit r of lead_mask[unit] = row r leads its phrase (k_phrases_or_seek).  One
// wavefront per lead item of phrase i, on lead.h's frame and walk:
//   1. the lead piece decoded with position numbers; the docs the unit's mask leaves are HELD;
//   2. the other rows of phrase i follow conjunctively, each against the docs every row so far
//      reached (a phrase-local alive set, rebuilt into the bitmap); none left ends the item;
//   3. the docs every row of phrase i reached, compacted, a lane each: the positions of its rows
//      merged with its offsets (FixedPhraseFrequency, phrase_iterator.hpp:75-166) — phrases_item's
//      two-cursor loop for two words, its seek loop otherwise, both bounded by tf.  pf_i == 0: the
//      doc leaves;
//   4. every other present phrase j, j < i first, then j > i, each in entry order: its rows walked
//      against the held docs — the walk narrows the phrase-local alive set, never the held docs —
//      and merged into pf_j.
//      OWNERSHIP (vphrase.h's rule at phrase level): the item keeps d only if no phrase j < i has
//      pf_j(d) > 0.  The phrase with the smallest index that matches d holds d in exactly one block
//      of its lead word, so every matching doc is scored — and counted — by exactly one item;
//   5. score = float32 sum in entry order over the phrases with pf > 0 of s_phrase(tf = pf, norm),
//      from the first one's value: for a kept doc that is phrase i, then the phrases j > i that match.
// A unit with one phrase computes what k_phrase / k_phrase2 compute for it, bit for bit: one
// score_value at tf = pf with the first row's scorer.
// A lead piece may be skipped against a threshold only with a bound on the WHOLE unit's score; none
// is kept per block, so these units are never pruned (irs_hip_batch_set_wand leaves them as they are).
#pragma once
#include "phrase.h"

namespace irs_hip {

// As k_vphrase_seek, for the lead items of k_phrases_or: the lead rows of a unit are the set bits of
// lead_mask[unit] — one row per phrase, not contiguous —, item t of the unit is block / tail `item` of
// the lead row `row` whose items hold t (ConjItem::item = item | row << 24); seek row: the start block
// in every other row, in row order.
__global__ void __launch_bounds__(kThreads)
k_phrases_or_seek(const DevSegment* segs, const DevQuery* queries, const DevTail* tails, uint32_t jt,
                  const uint32_t* units, const uint32_t* item_base /*[n_units + 1]*/, uint32_t n_units,
                  const uint32_t* lead_mask, uint32_t* seek, ConjItem* recs) {
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
  uint32_t left = lead_mask[unit] & ((1u << qd.n_terms) - 1u);
  if (!left) return;   // (a unit with items has a lead row)
  uint32_t item = t - item_base[lo], row = uint32_t(__builtin_ctz(left));
  for (left &= left - 1u; left; left &= left - 1u) {   // the lead row whose items hold t: blocks, then its tail
    const uint32_t k = tl[row].nblk + (tl[row].n ? 1u : 0u);
    if (item < k) break;
    item -= k;
    row = uint32_t(__builtin_ctz(left));
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

template<int MT>
struct PhrasesOrWave {
  uint32_t docs[kBlock];
  uint32_t pidx[MT][kBlock];          // first position number of the doc in row r's list
  uint32_t tf[MT][kBlock];            // its frequency there (0: the row has not reached the doc); a
                                      // merged phrase's frequency replaces its first row's
  alignas(16) uint8_t first[kConjBuckets];   // bucket -> 1 + entry index of its first lead doc (lead.h)
  uint32_t bm[kConjWords + 4];        // the current phrase's alive docs' buckets over [dlo, dhi]
  uint8_t apre[kConjWords + 4];       // bits of bm in the words before word w
  uint8_t list[kBlock];               // the entries a phrase is merged on, compacted
  DevPosTerm pt[MT];                  // the merge stage's per-row records
  uint32_t off[MT];
};

// Phrase frequency of rows [lo, end) of W on lead entry sl: phrases_item's two loops (phrases.h),
// every trip bounded by the rows' tf.  MATCH: ends at the first match.
template<int LAYOUT, int MT, bool MATCH>
__device__ __forceinline__ uint32_t phrases_or_freq(const DevSegment& ps, const PhrasesOrWave<MT>& W,
                                                    uint32_t lo, uint32_t end, uint32_t sl, uint32_t& my_pos) {
  uint32_t pf = 0;
  if (end - lo == 2u) {
    // two words: ONE loop that reads one position per trip, of whichever list is behind; every trip
    // ends the loop or advances a cursor below its tf
    const DevPosTerm pa = W.pt[lo], pb = W.pt[lo + 1u];
    const uint32_t off = W.off[lo + 1u];
    const uint32_t Pa = W.pidx[lo][sl], Pb = W.pidx[lo + 1u][sl];
    const uint32_t Ta = W.tf[lo][sl], Tb = W.tf[lo + 1u][sl];
    uint32_t ka = 0, kb = 0, va = ps.pos_base, vb = ps.pos_base;
    PosCursor ca{0, 0xFFFFFFFFu, 0}, cb{0, 0xFFFFFFFFu, 0};
    for (;;) {
      bool adv_a;
      if (ka == 0u) {
        adv_a = true;                       // lead.next()
      } else if (kb == 0u || vb < va + off) {
        adv_a = false;                      // position::seek(target) :1578-1604
      } else {
        pf += vb == va + off ? 1u : 0u;     // reached the target, or sought too far
        adv_a = true;
        if (MATCH && pf) break;
      }
      if (adv_a ? ka == Ta : kb == Tb) break;   // exhausted: no later position can match
      DevPosTerm pt;
      pt.pos_start = adv_a ? pa.pos_start : pb.pos_start;
      pt.row = adv_a ? pa.row : pb.row;
      pt.nfull = adv_a ? pa.nfull : pb.nfull;
      pt.tail_row = adv_a ? pa.tail_row : pb.tail_row;
      PosCursor cur = adv_a ? ca : cb;
      const uint32_t d = pos_delta_cached<LAYOUT>(ps, pt, cur, adv_a ? Pa + ka : Pb + kb);
      ++my_pos;
      if (adv_a) {
        ca = cur;
        va += d;
        ++ka;
        if (va + off < va) break;           // !pos_limits::valid(term_position)
      } else {
        cb = cur;
        vb += d;
        ++kb;
      }
    }
    return pf;
  }
  // FixedPhraseFrequency::NextPosition (phrase_iterator.hpp:109-151): every position of the first
  // word, the others sought to it + their offsets
  const uint32_t nw = end - lo;
  uint32_t K[MT], V[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    K[i] = 0u;
    V[i] = ps.pos_base;  // pos_limits::invalid() (+ min() before the first delta, one-based)
  }
  const uint32_t T0 = W.tf[lo][sl], P0 = W.pidx[lo][sl];
  uint32_t head = ps.pos_base;
  bool done = false;
  for (uint32_t a = 0; a < T0 && !done; ++a) {
    head += pos_delta<LAYOUT>(ps, W.pt[lo], 0u, P0 + a);  // lead.next()
    ++my_pos;
    bool match = true;
#pragma unroll
    for (int i = 1; i < MT; ++i) {
      if (uint32_t(i) < nw && match && !done) {
        const uint32_t target = head + W.off[lo + i];
        if (target < head) { done = true; break; }  // !pos_limits::valid(term_position)
        const uint32_t Ti = W.tf[lo + i][sl], Pi = W.pidx[lo + i][sl];
        // position::seek(target) :1578-1604 (value_ invalid until the first position: K == 0)
        while ((K[i] == 0u || V[i] < target) && K[i] < Ti) {
          V[i] += pos_delta<LAYOUT>(ps, W.pt[lo + i], 0u, Pi + K[i]);
          ++K[i];
          ++my_pos;
        }
        if (V[i] < target) done = true;           // exhausted: no later position can match
        else if (V[i] != target) match = false;   // sought too far
      }
    }
    if (match && !done) ++pf;
    if (MATCH && pf) break;
  }
  return pf;
}

// MATCH (k_phrases_or_match): the same ownership, so a doc sets its bit and counts once; the merges
// end at the first match and the phrases behind the item's own are not probed
template<int LAYOUT, int MT, bool MATCH = false>
__device__ __forceinline__ void phrases_or_item(const ConjArgs& A, const uint32_t* opens_of, uint32_t pilot,
                                                PhrasesOrWave<MT>* s_wave, uint32_t* sets32 = nullptr,
                                                uint64_t words32 = 0, unsigned long long* counts = nullptr) {
  const uint32_t tid = threadIdx.x;
  const unsigned lane = tid & 63u;
  const uint32_t wv = wave::uniform(tid >> 6);
  const uint32_t e = lead_item_of(A, pilot, kPhraseWaves);
  if (e == kNoItem) return;
  const ConjItem R = wave::sload<ConjItem>(reinterpret_cast<uint64_t>(A.recs) + uint64_t(e) * sizeof(ConjItem));
  const uint32_t unit = R.unit, item = R.item & kConjItemBlock, lead = (R.item >> 24) & 0xFu;
  const DevQuery qd = wave::sload<DevQuery>(reinterpret_cast<uint64_t>(A.queries) + uint64_t(unit) * sizeof(DevQuery));
  const uint32_t m = qd.n_terms;
  if (m == 0 || m > uint32_t(MT) || lead >= m) return;
  const uint32_t opens = (wave::uniform(opens_of[unit]) | 1u) & ((1u << m) - 1u);
  const uint32_t own_lo = group_lo(opens, lead), own_end = group_end(opens, lead, m);
  const DevSegment& seg = A.segs[qd.seg];   // (read field by field)
  const uint64_t tl_at = reinterpret_cast<uint64_t>(A.tails) + uint64_t(unit) * A.jt * sizeof(DevTail);
  auto term_tail = [&](uint32_t i) { return wave::sload<DevTail>(tl_at + i * sizeof(DevTail)); };
  const DevTail ld = term_tail(lead);
  const uint32_t bs = (MATCH || pilot) ? 0u : A.bstar[unit];
  PhrasesOrWave<MT>& W = s_wave[wv];
  uint32_t* docs = W.docs;
  const uint32_t* seek = A.seek + uint64_t(e) * (A.jt - 1u);
  if (lane < m) {   // what the position merges read, a lane per row
    const DevTail t = A.tails[uint64_t(unit) * A.jt + lane];
    W.pt[lane] = seg.pterms[t.term];
    W.off[lane] = A.qterms[qd.first_term + lane].pad0;   // offset in the row's own phrase
  }

  // ---- 1. the lead item: entry index 2*lane + h (block) or lane + 64*h (tail)
  uint32_t n = kBlock;
  uint32_t bytes = 0;   // (wave-uniform) encoded bytes of the doc blocks this wavefront decodes
  const bool counting = !pilot && A.touched != nullptr;   // (irs_hip_batch_profile bit 1)
  uint32_t ld_d[2], ld_e[2];
  bool held[2];   // the lane's lead docs this item may still score (docs of the unit: not deleted, not masked)
  {
    uint32_t f[2], p[2];
    n = lead_decode_pos<LAYOUT>(seg, ld, R, item, lane, counting, bytes, ld_d, ld_e, f, p);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t idx = ld_e[h];
      docs[idx] = idx < n ? ld_d[h] : 0xFFFFFFFFu;
      // a masked doc keeps its place among the lead docs but counts as not reached by the lead
      held[h] = idx < n && !(qd.dead && doc_dead(qd.dead, ld_d[h]));
      for (uint32_t i = 0; i < m; ++i) {
        W.pidx[i][idx] = i == lead ? p[h] : 0u;
        W.tf[i][idx] = (i == lead && held[h]) ? f[h] : 0u;
      }
    }
    lead_first_clear(W.first, lane);
  }
  wave::sync();
  if (qd.dead && wave::ballot(held[0] || held[1]) == 0) {   // (wave-uniform) no lead doc is left
    lead_skipped(A, unit, counting, bytes, lane);
    return;
  }
  const LeadFrame fr = lead_frame(docs, n);
  lead_first_fill(fr, W.first, docs, ld_d, ld_e, n);
  wave::sync();
  uint32_t my_pos = 0;
  // (the fields the position merges read, in registers)
  DevSegment ps{};
  ps.pos = seg.pos;
  ps.pblk_off = seg.pblk_off;
  ps.pblk_bits = seg.pblk_bits;
  ps.ptail = seg.ptail;
  ps.pos_base = seg.pos_base;
  // the lane's two entries (an entry behind the item's postings reads column 0 and is never alive)
  const uint32_t col[2] = {ld_e[0] < n ? ld_e[0] : 0u, ld_e[1] < n ? ld_e[1] : 0u};

  // ---- 2./3. one phrase, rows [lo, end), on the held docs: pf[h] = its frequency on the lane's
  // entries (0: not held, or no match).  `loc` is the phrase's own alive set.
  auto run_phrase = [&](uint32_t lo, uint32_t end, uint32_t (&pf)[2]) {
    bool loc[2] = {held[0], held[1]};
    for (uint32_t i = lo; i < end; ++i) {
      if (i == lead) continue;
      const uint32_t left = alive_rebuild(fr, W.bm, W.apre, ld_d, loc, lane);
      wave::sync();
      if (left == 0u) {   // (wave-uniform) no held doc reached by every row so far
        loc[0] = loc[1] = false;
        break;
      }
      const DevTail tl = term_tail(i);
      // a decoded posting of row i on a lead doc: (P, tf) into the row at the doc's entry
      auto put = [&](uint32_t doc, uint32_t f, uint32_t p) {
        const uint32_t x = doc - fr.dlo;
        if (f == 0 || x > fr.span) return;
        const uint32_t t = lead_index(W.first, docs, n, x >> fr.s, fr.s, doc);
        if (t == n) return;
        W.pidx[i][t] = p;
        W.tf[i][t] = f;
      };
      follow_list<LAYOUT, true, false>(seg, tl, seek[i < lead ? i : i - 1u], fr, W.bm, W.apre, counting, bytes,
                                       lane, put);
      wave::sync();
#pragma unroll
      for (int h = 0; h < 2; ++h) loc[h] = loc[h] && W.tf[i][col[h]] != 0u;
    }
    // the docs every row reached, compacted, a lane each
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t m0 = wave::ballot(loc[0]), m1 = wave::ballot(loc[1]);
    const uint32_t c0 = uint32_t(__builtin_popcountll(m0));
    const uint32_t total = c0 + uint32_t(__builtin_popcountll(m1));
    if (loc[0]) W.list[__builtin_popcountll(m0 & below)] = uint8_t(ld_e[0]);
    if (loc[1]) W.list[c0 + uint32_t(__builtin_popcountll(m1 & below))] = uint8_t(ld_e[1]);
    wave::sync();
    for (uint32_t q0 = 0; q0 < total; q0 += 64) {
      if (q0 + lane < total) {
        const uint32_t sl = W.list[q0 + lane];
        const uint32_t f = phrases_or_freq<LAYOUT, MT, MATCH>(ps, W, lo, end, sl, my_pos);
        W.tf[lo][sl] = f;   // (this lane's column: the phrase's frequency, read back by the entry's lane)
      }
    }
    wave::sync();
#pragma unroll
    for (int h = 0; h < 2; ++h) pf[h] = loc[h] ? W.tf[lo][col[h]] : 0u;
    wave::sync();   // (the list and the bitmap are free for the next phrase)
  };
  auto finish = [&](uint32_t my_hits) {   // what the item leaves behind
    if constexpr (MATCH) {
      my_hits = wave::reduce_add(my_hits);
      if (lane == 0 && my_hits && counts) atomicAdd(&counts[unit], static_cast<unsigned long long>(my_hits));
    } else {
      if (pilot) return;
      my_hits = wave::reduce_add(my_hits);
      if (lane == 0 && my_hits) A.item_hits[e] = my_hits;
      if (A.touched) {   // (only when the batch counts: irs_hip_batch_profile bit 1)
        my_pos = wave::reduce_add(my_pos);
        if (lane == 0) {
          atomicAdd(&A.touched[2u * unit], static_cast<unsigned long long>(bytes));
          if (my_pos) atomicAdd(&A.touched[2u * unit + 1u], static_cast<unsigned long long>(my_pos));
        }
      }
    }
  };

  // The phrases in the order the item wants them — its own, then those in front of it, then those
  // behind — through ONE copy of the phrase step (`at`: the next one's first row; wave-uniform).
  uint32_t pf[2];
  float score[2] = {0.f, 0.f};
  uint32_t nv[2] = {0u, 0u};
  const uint32_t last = MATCH ? own_lo : m;   // (a match-only item does not probe the phrases behind its own)
  for (uint32_t lo = own_lo, at = 0u;;) {
    const uint32_t end = group_end(opens, lo, m);
    run_phrase(lo, end, pf);
    if (lo == own_lo) {
      // ---- 3. its own phrase: the docs it does not match leave
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        held[h] = held[h] && pf[h] != 0u;
        if constexpr (!MATCH) {
          if (held[h]) {
            // (a posting of the lead item: its norm from the posting-order copy of the column)
            nv[h] = !seg.pnorm ? norm_value(seg, ld_d[h])
                    : (item < ld.nblk ? seg.pnorm[(ld.dir_off + item) * kBlock + ld_e[h]]
                                      : seg.tail_norms[ld.tail_row + ld_e[h]]);
            score[h] = score_value(A.qterms[qd.first_term + lo], pf[h], nv[h]);
          }
        }
      }
    } else if (lo < own_lo) {
      // ---- 4. a phrase in front of it owns the docs it matches
#pragma unroll
      for (int h = 0; h < 2; ++h) held[h] = held[h] && pf[h] == 0u;
    } else {
      // ---- 4./5. a phrase behind it adds its score where it matches
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (held[h] && pf[h] != 0u) score[h] += score_value(A.qterms[qd.first_term + lo], pf[h], nv[h]);
    }
    if (wave::ballot(held[0] || held[1]) == 0) return finish(0u);
    if (lo != own_lo) at = end;
    if (at == own_lo) at = own_end;   // (its own phrase is done)
    if (at >= last) break;
    lo = at;
  }
  uint32_t my_hits = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if constexpr (MATCH) {
      if (held[h]) {
        if (sets32) atomicOr(&sets32[uint64_t(unit) * words32 + (ld_d[h] >> 5)], 1u << (ld_d[h] & 31u));
        ++my_hits;
      }
    } else {
      bool cand = false;
      if (held[h]) {
        const uint32_t bin = score_bin(score[h], qd.bin_scale);
        if (pilot) atomicAdd(&A.hist[uint64_t(unit) * kBins + bin], 1u);
        else cand = bin >= bs;   // below the pilot's threshold bin: cannot be among the top k
        ++my_hits;
      }
      emit_candidates(A, unit, cand, score[h], ld_d[h], lane);
    }
  }
  finish(my_hits);
}

// MT in {4, 8}: the words of all phrases <= 8 (IRS_HIP_MAX_PHRASE_TERMS)
template<int LAYOUT, int MT>
__global__ void __launch_bounds__(kPhraseWaves * 64)
k_phrases_or(ConjArgs A, const uint32_t* opens, uint32_t pilot) {
  __shared__ PhrasesOrWave<MT> s_wave[kPhraseWaves];
  phrases_or_item<LAYOUT, MT>(A, opens, pilot, s_wave);
}
// Unscored execution (irs_hip_batch_match_sets, match.h): the docs on which some phrase matches
template<int LAYOUT, int MT>
__global__ void __launch_bounds__(kPhraseWaves * 64)
k_phrases_or_match(ConjArgs A, const uint32_t* opens, uint32_t* sets32, uint64_t words32,
                   unsigned long long* counts) {
  __shared__ PhrasesOrWave<MT> s_wave[kPhraseWaves];
  phrases_or_item<LAYOUT, MT, true>(A, opens, 0u, s_wave, sets32, words32, counts);
}

}  // namespace irs_hip
