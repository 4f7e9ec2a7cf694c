// phrases.h — And([by_phrase, by_phrase..., by_term...]): several phrases in one conjunction, plus
// required terms (IRS_HIP_PHRASE_NEXT; the reference: And::prepare -> make_conjunction over
// {PhraseIterator..., term iterators}, boolean_filter.cpp:150-210, boolean_query.cpp:60-145,
// conjunction.hpp:436-490).
//
// The rows of a unit are its entries: the words of phrase 1, of phrase 2, ..., then the required
// terms.  n_phrase[unit] = the first required row (= all word rows); bit r of the unit's `opens` word
// = row r opens a phrase (bit 0 always).  The same term may stand in two rows ("a b" next to "b a",
// one phrase twice): every row has its own (P, tf) row in LDS, its own seek column, its own cursor —
// nothing here is keyed by term.
//
// The block-driven scheme of k_phrase_and (phrase.h), written on lead.h's frame and walk:
//   1. the lead is the rarest of ALL rows (build_phrase_work), its item decoded with position numbers;
//   2. every other row follows in row order: (P, tf) at the lead doc's rank where the lead and every
//      earlier row hold the doc, which marks the doc alive for the next row; an empty alive bitmap
//      ends the item;
//   3. the docs every row reached, compacted, a lane each: phrase after phrase in entry order the
//      positions of its rows are merged with its offsets (FixedPhraseFrequency,
//      phrase_iterator.hpp:75-166) — phrase_item's two-cursor loop for a phrase of two words, its
//      nested seek loop otherwise — until a phrase has frequency 0: no match.  ONE phrase's cursors
//      live at a time; a phrase's frequency replaces the tf of its first row in LDS (the lane owns
//      the doc's column), which is where step 4 finds it;
//   4. score = float32 sum over the And's children — a phrase at tf = its frequency with the scorer
//      its first word carries, a term at its own tf — in cost order as Conjunction sorts them
//      (conjunction.hpp:450-453): a phrase costs its rarest word's docs_count, a term its own, ties
//      in entry order; the sum starts from the first child's value.
// A unit with one phrase is what k_phrase_and computes for it, bit for bit: the same score_value per
// child, added in the same order (one phrase and no term: its value alone, as k_phrase / k_phrase2).
// Every loop of step 3 is bounded by the rows' tf, as in phrase_item.
#pragma once
#include "phrase.h"

namespace irs_hip {

constexpr int kPhraseSeveral = 3;   // (launch_phrase's REQ: next to kPhraseReq / kPhraseOpt)

template<int MT>
struct PhrasesWave : PhraseWave<MT> {
  uint32_t cost[MT];    // docs_count of the row's term
  uint32_t order[MT];   // the And's children by cost: the r-th cheapest one's first row
};

// MATCH (k_phrases_and_match): steps 1-3 only, a phrase's merge ends at its first match; a doc on
// which every phrase has one sets its bit in the unit's row of `sets32` and counts for the unit
template<int LAYOUT, int MT, bool MATCH = false>
__device__ __forceinline__ void phrases_item(const ConjArgs& A, const uint32_t* n_phrase,
                                             const uint32_t* opens_of, uint32_t pilot,
                                             PhrasesWave<MT>* s_wave, uint32_t* sets32 = nullptr,
                                             uint64_t words32 = 0, unsigned long long* counts = nullptr) {
  const uint32_t tid = threadIdx.x;
  const unsigned lane = tid & 63u;
  const uint32_t wv = wave::uniform(tid >> 6);
  const uint32_t e = lead_item_of(A, pilot, kPhraseWaves);
  if (e == kNoItem) return;
  const ConjItem R = wave::sload<ConjItem>(reinterpret_cast<uint64_t>(A.recs) + uint64_t(e) * sizeof(ConjItem));
  const uint32_t unit = R.unit, item = R.item & kConjItemBlock;
  const DevQuery qd = wave::sload<DevQuery>(reinterpret_cast<uint64_t>(A.queries) + uint64_t(unit) * sizeof(DevQuery));
  const uint32_t m = qd.n_terms;
  if (m == 0 || m > uint32_t(MT)) return;
  // rows [0, mp) are words, rows [mp, m) required terms
  const uint32_t mp = wave::uniform(n_phrase[unit]);
  if (mp == 0u || mp > m) return;
  const uint32_t opens = (wave::uniform(opens_of[unit]) | 1u) & ((1u << mp) - 1u);
  const DevSegment& seg = A.segs[qd.seg];   // (read field by field)
  const uint64_t tl_at = reinterpret_cast<uint64_t>(A.tails) + uint64_t(unit) * A.jt * sizeof(DevTail);
  auto term_tail = [&](uint32_t i) { return wave::sload<DevTail>(tl_at + i * sizeof(DevTail)); };
  const uint32_t lead = wave::uniform(A.lead_of[unit]);
  if (lead >= m) return;
  const DevTail ld = term_tail(lead);
  const uint32_t bs = (MATCH || pilot) ? 0u : A.bstar[unit];
  PhrasesWave<MT>& W = s_wave[wv];
  uint32_t* docs = W.docs;
  const uint32_t* seek = A.seek + uint64_t(e) * (A.jt - 1u);
  if (lane < m) {   // what the position merges and the cost order read, a lane per row
    const DevTail t = A.tails[uint64_t(unit) * A.jt + lane];
    W.pt[lane] = seg.pterms[t.term];
    W.off[lane] = lane < mp ? A.qterms[qd.first_term + lane].pad0 : 0u;   // offset in the row's own phrase
    W.cost[lane] = t.nblk * kBlock + t.n;
  }

  // ---- 1. the lead item: entry index 2*lane + h (block) or lane + 64*h (tail)
  uint32_t n = kBlock;
  uint32_t bytes = 0;   // (wave-uniform) encoded bytes of the doc blocks this wavefront decodes
  const bool counting = !pilot && A.touched != nullptr;   // (irs_hip_batch_profile bit 1)
  uint32_t ld_d[2], ld_e[2];
  bool live[2];   // the lane's lead docs that are docs of the unit at all (not deleted, not masked)
  {
    uint32_t f[2], p[2];
    n = lead_decode_pos<LAYOUT>(seg, ld, R, item, lane, counting, bytes, ld_d, ld_e, f, p);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t idx = ld_e[h];
      docs[idx] = idx < n ? ld_d[h] : 0xFFFFFFFFu;
      // a masked doc keeps its place among the lead docs but counts as not reached by the lead
      live[h] = idx < n && !(qd.dead && doc_dead(qd.dead, ld_d[h]));
      for (uint32_t i = 0; i < m; ++i) {
        W.pidx[i][idx] = i == lead ? p[h] : 0u;
        W.tf[i][idx] = (i == lead && live[h]) ? f[h] : 0u;
      }
    }
    if (lane < (kConjWords + 4u) / 2u) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        W.bm[k][2u * lane] = 0u;
        W.bm[k][2u * lane + 1u] = 0u;
      }
    }
    lead_first_clear(W.first, lane);
  }
  wave::sync();
  if (qd.dead && wave::ballot(live[0] || live[1]) == 0) {   // (wave-uniform) no lead doc is left
    lead_skipped(A, unit, counting, bytes, lane);
    return;
  }
  const LeadFrame fr = lead_frame(docs, n);
  const bool masked = qd.dead != nullptr;   // (wave-uniform)
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (ld_e[h] < n) {
      const uint32_t bk = fr.bucket(ld_d[h]);
      atomicOr(&W.bm[0][bk >> 5], 1u << (bk & 31u));
      // (the first follower may only reach the LIVE lead docs)
      if (masked && live[h]) atomicOr(&W.bm[2][bk >> 5], 1u << (bk & 31u));
    }
  }
  lead_first_fill(fr, W.first, docs, ld_d, ld_e, n);
  // The And's children in the order their scores are summed: row r opens a child when it opens a
  // phrase or is a required term; a phrase costs its rarest word.  The lane of a child's first row
  // ranks it among the others (cost, then entry order).
  const uint32_t heads = opens | (((1u << m) - 1u) & ~((1u << mp) - 1u));
  const uint32_t n_children = uint32_t(__builtin_popcount(heads));
  if (!MATCH && lane < m && ((heads >> lane) & 1u)) {
    auto child_cost = [&](uint32_t lo) {
      const uint32_t end = lo < mp ? group_end(opens, lo, mp) : lo + 1u;
      uint32_t c = W.cost[lo];
      for (uint32_t r = lo + 1u; r < end; ++r) c = W.cost[r] < c ? W.cost[r] : c;
      return c;
    };
    const uint32_t mine = child_cost(lane);
    uint32_t rank = 0;
    for (uint32_t r = 0; r < m; ++r) {
      if (r == lane || !((heads >> r) & 1u)) continue;
      const uint32_t c = child_cost(r);
      rank += (c < mine || (c == mine && r < lane)) ? 1u : 0u;
    }
    W.order[rank] = lane;
  }
  wave::sync();
  bitmap_prefix(W.bm[0], W.lpre, lane);
  wave::sync();

  // ---- 2. every other row, in row order
  uint32_t step = 0;   // followers done so far
  for (uint32_t i = 0; i < m; ++i) {
    if (i == lead) continue;
    const DevTail tl = term_tail(i);
    // alive = docs every row so far reached: the lead bitmap, then what the previous follower
    // marked; `mark` collects what this one reaches
    const uint32_t mk = 1u + (step & 1u);
    const uint32_t* alive = step == 0u ? (masked ? W.bm[2] : W.bm[0]) : W.bm[3u - mk];
    uint32_t* mark = W.bm[mk];
    const uint8_t* apre = W.lpre;
    if (step > 0u || masked) {
      if (step > 0u && lane < kConjWords / 2u) {
        mark[2u * lane] = 0u;
        mark[2u * lane + 1u] = 0u;
      }
      apre = W.apre;
      const uint32_t left = bitmap_prefix(alive, W.apre, lane);
      wave::sync();
      if (left == 0u) {   // no doc reached by every row so far: done
        if (counting && lane == 0) atomicAdd(&A.touched[2u * unit], static_cast<unsigned long long>(bytes));
        return;
      }
    }
    ++step;
    const bool more_rows = step + 1u < m;   // (the last follower marks nothing: nobody reads it)
    // a decoded posting of row i: is its doc one of the lead docs still alive?
    auto put = [&](uint32_t doc, uint32_t f, uint32_t p) {
      const uint32_t x = doc - fr.dlo;
      if (f == 0 || x > fr.span) return;
      const uint32_t bk = x >> fr.s;
      const uint32_t t = lead_index(W.first, docs, n, bk, fr.s, doc);
      if (t == n) return;
      // every earlier row — and the lead, whose masked docs count as not reached — holds THIS doc
      if (W.tf[lead][t] == 0u) return;
      for (uint32_t j = 0; j < i; ++j)
        if (j != lead && W.tf[j][t] == 0u) return;
      W.pidx[i][t] = p;
      W.tf[i][t] = f;
      if (more_rows) atomicOr(&mark[bk >> 5], 1u << (bk & 31u));   // (alive for the next row)
    };
    follow_list<LAYOUT, true, false>(seg, tl, seek[i < lead ? i : i - 1u], fr, alive, apre, counting, bytes,
                                     lane, put);
    wave::sync();
  }

  // ---- 3./4. lead docs every row reached, compacted: merge phrase after phrase, score, emit
  bool h01[2];
  uint64_t m01[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t sl = lane + 64u * uint32_t(h);
    bool all = sl < n;
    for (uint32_t i = 0; i < m; ++i) all = all && W.tf[i][sl < n ? sl : 0u] != 0u;
    h01[h] = all;
    m01[h] = wave::ballot(all);
  }
  const uint64_t below = (1ull << lane) - 1ull;
  const uint32_t c0 = uint32_t(__builtin_popcountll(m01[0]));
  const uint32_t total = c0 + uint32_t(__builtin_popcountll(m01[1]));
  uint8_t* list = W.first;   // (the bucket table has served: room for the 128 entry indices)
  if (h01[0]) list[__builtin_popcountll(m01[0] & below)] = uint8_t(lane);
  if (h01[1]) list[c0 + uint32_t(__builtin_popcountll(m01[1] & below))] = uint8_t(lane + 64u);
  wave::sync();
  uint32_t my_hits = 0, my_pos = 0;
  // (the fields the position merges read, in registers)
  DevSegment ps{};
  ps.pos = seg.pos;
  ps.pblk_off = seg.pblk_off;
  ps.pblk_bits = seg.pblk_bits;
  ps.ptail = seg.ptail;
  ps.pos_base = seg.pos_base;
  for (uint32_t q0 = 0; q0 < total; q0 += 64) {
    bool cand = false;
    float score = 0.f;
    uint32_t doc = 0;
    if (q0 + lane < total) {
      const uint32_t sl = list[q0 + lane];
      bool ok = true;   // every phrase so far has a match on the doc
      for (uint32_t lo = 0; lo < mp;) {   // (wave-uniform) phrase [lo, end)
        const uint32_t end = group_end(opens, lo, mp);
        if (ok) {
          uint32_t pf = 0;
          if (end - lo == 2u) {
            // two words: ONE loop that reads one position per trip, of whichever list is behind
            // (phrase_item); every trip ends the loop or advances a cursor below its tf
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
          } else {
            // FixedPhraseFrequency::NextPosition (phrase_iterator.hpp:109-151): every position of
            // the first word, the others sought to it + their offsets
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
          }
          if constexpr (!MATCH) W.tf[lo][sl] = pf;   // (this lane's column: the phrase's tf for step 4)
          ok = pf != 0u;
        }
        lo = end;
      }
      if constexpr (MATCH) {
        if (ok) {
          doc = docs[sl];
          if (sets32) atomicOr(&sets32[uint64_t(unit) * words32 + (doc >> 5)], 1u << (doc & 31u));
          ++my_hits;
        }
      } else if (ok) {
        doc = docs[sl];
        // (a posting of the lead item: its norm from the posting-order copy of the column)
        const uint32_t nv = !seg.pnorm ? norm_value(seg, doc)
                            : (item < ld.nblk ? seg.pnorm[(ld.dir_off + item) * kBlock + sl]
                                              : seg.tail_norms[ld.tail_row + sl]);
        // the children in cost order (each one's scorer read where it is used), from the first's value
        for (uint32_t r = 0; r < n_children; ++r) {
          const uint32_t row = W.order[r];
          const float v = score_value(A.qterms[qd.first_term + row], W.tf[row][sl], nv);
          score = r == 0u ? v : score + v;
        }
        const uint32_t bin = score_bin(score, qd.bin_scale);
        if (pilot) atomicAdd(&A.hist[uint64_t(unit) * kBins + bin], 1u);
        else cand = bin >= bs;   // below the pilot's threshold bin: cannot be among the top k
        ++my_hits;
      }
    }
    if constexpr (!MATCH) emit_candidates(A, unit, cand, score, doc, lane);
  }
  if constexpr (MATCH) {
    my_hits = wave::reduce_add(my_hits);
    if (lane == 0 && my_hits && counts) atomicAdd(&counts[unit], static_cast<unsigned long long>(my_hits));
    return;
  }
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

// MT in {4, 8}: words + required terms <= 8 (IRS_HIP_MAX_PHRASE_TERMS)
template<int LAYOUT, int MT>
__global__ void __launch_bounds__(kPhraseWaves * 64)
k_phrases_and(ConjArgs A, const uint32_t* n_phrase, const uint32_t* opens, uint32_t pilot) {
  __shared__ PhrasesWave<MT> s_wave[kPhraseWaves];
  phrases_item<LAYOUT, MT>(A, n_phrase, opens, pilot, s_wave);
}
// Unscored execution (irs_hip_batch_match_sets, match.h): the docs on which every phrase matches
// and every required term stands
template<int LAYOUT, int MT>
__global__ void __launch_bounds__(kPhraseWaves * 64)
k_phrases_and_match(ConjArgs A, const uint32_t* n_phrase, const uint32_t* opens, uint32_t* sets32,
                    uint64_t words32, unsigned long long* counts) {
  __shared__ PhrasesWave<MT> s_wave[kPhraseWaves];
  phrases_item<LAYOUT, MT, true>(A, n_phrase, opens, 0u, s_wave, sets32, words32, counts);
}

}  // namespace irs_hip
