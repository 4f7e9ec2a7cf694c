// phrase.h — positions (`.pos`) and by_phrase with fixed offsets.
//
// Reference: the position attribute of a posting list, formats_10.cpp:1457-1682
// (position_impl::prepare / read_block / read_tail_block, position::next / seek / skip),
// its writer :894-933 and EndTerm :713-760; the phrase iterator
// core/search/phrase_iterator.hpp:75-166 (FixedPhraseFrequency) and :540-626
// (PhraseIterator: conjunction of the terms, then the phrase frequency as tf).
//
// The reference walks the `.pos` stream sequentially behind every doc iterator
// ("pend_pos" positions behind).  Here the stream is RANDOM ACCESS: position number P of
// a term (0-based over the whole list) sits in pos block P / 128 at slot P % 128, a pos
// block directory built at open says where each block starts and how wide it is, and
// one packed value is extracted by itself (both layouts).  P of a doc's first position
// is the exclusive prefix sum of the frequencies in front of it: per 128-doc block that
// sum is precomputed at open (DevSegment::blk_pos), inside the block one wavefront scan
// gives the rest.  So the conjunction of the phrase's terms is formed from the doc blocks
// alone (k_phrase below), with (P, tf) riding along, and only docs holding ALL phrase terms
// ever touch the position stream.  What k_phrase shares with the other block-driven kernels — the
// lead item's records and the doc-block decoders — is in lead.h, which also describes the lead frame
// and the follower walk; phrase_item keeps its own text of those two (see there for why).
#pragma once
#include "lead.h"
#include "score.h"

namespace irs_hip {

constexpr uint32_t kPhraseMaxTerms = 8;    // IRS_HIP_MAX_PHRASE_TERMS

// Value j (0..127) of one packed block payload of `bits` (1..32) bits per value:
// packed::at for the scalar layout (bit_packing.hpp), the same for simdcomp's 4-lane one.
template<int LAYOUT>
__device__ __forceinline__ uint32_t packed_at(const uint8_t* payload, uint32_t bits, uint32_t j) {
  const uint32_t mask = bits >= 32 ? 0xFFFFFFFFu : ((1u << bits) - 1u);
  if (LAYOUT == kSimd4) {
    // value j = 4r + l: SSE lane l, bit r*bits of that lane's stream; word k of it = u32 4k + l
    const uint32_t l = j & 3u, bit = (j >> 2) * bits, k = bit >> 5;
    const uint8_t* p = payload + 4u * (4u * k + l);
    const uint64_t w0 = wave::load_u32(p), w1 = wave::load_u32(p + 16);
    return uint32_t(((w1 << 32) | w0) >> (bit & 31u)) & mask;
  }
  const uint32_t bit = j * bits;
  return uint32_t(wave::load_u64(payload + 4u * (bit >> 5)) >> (bit & 31u)) & mask;
}

// Position delta number `idx` of a term (what position::next adds to value_, :1624-1626).
template<int LAYOUT>
__device__ __forceinline__ uint32_t pos_delta(const DevSegment& seg, const DevPosTerm& pt,
                                              uint32_t term, uint32_t idx) {
  const uint32_t b = idx >> 7;
  if (b < pt.nfull) {
    const uint64_t e = pt.row + b;
    const uint8_t* blk = seg.pos + pt.pos_start + seg.pblk_off[e];
    const uint32_t bits = seg.pblk_bits[e];
    if (bits == 0) {  // ALL_EQUAL (bitpack.hpp:159)
      uint32_t len;
      return vint_from(wave::load_u64(blk + 1), &len);
    }
    return packed_at<LAYOUT>(blk + 1, bits, idx & 127u);
  }
  return seg.ptail[pt.tail_row + (idx - (pt.nfull << 7))];  // read_tail_block :1515
}

// A position list read front to back: the block a delta lives in (its payload address and bit
// width: two dependent directory reads) is looked up once per 128 positions, not per position.
struct PosCursor {
  uint64_t payload;   // address of the current block's packed payload / of its all-equal value
  uint32_t blk;       // index of the current block (0xFFFFFFFF: none yet)
  uint32_t bits;      // its bit width (0: all-equal)
};
template<int LAYOUT>
__device__ __forceinline__ uint32_t pos_delta_cached(const DevSegment& seg, const DevPosTerm& pt,
                                                     PosCursor& c, uint32_t idx) {
  const uint32_t b = idx >> 7;
  if (b >= pt.nfull) return seg.ptail[pt.tail_row + (idx - (pt.nfull << 7))];  // read_tail_block :1515
  if (b != c.blk) {
    const uint64_t e = pt.row + b;
    c.blk = b;
    c.bits = seg.pblk_bits[e];
    c.payload = reinterpret_cast<uint64_t>(seg.pos + pt.pos_start + seg.pblk_off[e] + 1);
  }
  const uint8_t* pl = reinterpret_cast<const uint8_t*>(c.payload);
  if (c.bits == 0) {  // ALL_EQUAL (bitpack.hpp:159)
    uint32_t len;
    return vint_from(wave::load_u64(pl), &len);
  }
  return packed_at<LAYOUT>(pl, c.bits, idx & 127u);
}

// ------------------------------------------------------------ open time --

// Sum of the frequencies of every full doc block (-> exclusive scan -> blk_pos).
// Work split by directory row, as k_pack_payloads.
template<int LAYOUT>
__global__ void __launch_bounds__(kThreads)
k_freq_sums(DevSegment seg, uint64_t rows, uint32_t* sums) {
  const unsigned lane = threadIdx.x & 63u;
  IRS_FOR_ROWS(e, rows) {
    const uint32_t bits = seg.blk_bits[e];
    uint32_t d0, d1, f0, f1;
    decode_block<LAYOUT, true>(row_block(seg, e), bits & 0xFFu, bits >> 8,
                               0u, lane, d0, d1, f0, f1);
    const uint32_t s = wave::reduce_add(f0 + f1);
    if (lane == 0) sums[e] = s;
  }
}

// term_meta::freq (what sizes the position buffers and the pos block directory) must be
// what the `.doc` stream really holds: the frequencies of the term's full blocks (blk_pos
// differences) plus those of its decoded tail.  One thread per term.
__global__ void __launch_bounds__(kThreads)
k_check_freq_totals(DevSegment seg, const DevPosTerm* pterms, uint32_t* status) {
  const uint32_t term = blockIdx.x * kThreads + threadIdx.x;
  if (term >= seg.num_terms) return;
  const DevTerm t = seg.terms[term];
  if (t.docs_count == 0) return;
  uint32_t sum = seg.blk_pos[t.dir_off + t.nblk] - seg.blk_pos[t.dir_off];
  const uint32_t n = t.docs_count == 1 ? 1u : t.tail_n;
  for (uint32_t i = 0; i < n; ++i) sum += seg.tail_freqs[t.tail_row + i];
  if (sum != pterms[term].total) atomicOr(status, kStatusCorrupt);
}

// One workgroup per term lists the term's pos blocks (header byte -> size,
// bitpack::skip_block32) and decodes the vint tail (read_tail_block :1515-1537).  The headers
// form a chain of dependent one-byte reads; the stream is staged through LDS 8 KB at a time
// and the chain of a window is followed by pointer doubling (chain_orbit, kernels.h), all
// threads write the directory rows.  The 10 M-doc segment's longest term has 540 k pos blocks.
__global__ void __launch_bounds__(kChainThreads)
k_pos_directory(DevSegment seg, DevPosTerm* pterms, uint32_t* pblk_off, uint8_t* pblk_bits,
                uint32_t* ptail, const uint64_t* pos_end, uint32_t* status) {
  __shared__ __attribute__((aligned(16))) uint8_t win[kChainWindow + 64];
  __shared__ ChainTables s_chain;
  __shared__ uint32_t s_hdr[kChainCap];   // (offset in the window << 8) | bits
  __shared__ uint64_t s_cur;
  __shared__ uint32_t s_bad;
  const uint32_t tid = threadIdx.x;
  const uint32_t term = blockIdx.x;
  if (term >= seg.num_terms) return;
  const DevPosTerm pt = pterms[term];
  if (pt.total == 0) return;
  const uint64_t staged = seg.pos_len + kPadBytes;  // the device copy ends with zero padding
  uint64_t cur = pt.pos_start, win_lo = 0;
  uint32_t b = 0, bad = 0, lim = 0;
  // window [win_lo, win_lo + lim) of the stream, starting at the 16-byte line holding `at`
  auto refill = [&](uint64_t at) {
    win_lo = at & ~uint64_t(15);
    uint64_t bytes = staged - win_lo;
    if (bytes > kChainWindow) bytes = kChainWindow;
    bytes &= ~uint64_t(15);
    for (uint32_t o = tid * 16u; o < bytes; o += kChainThreads * 16u)
      *reinterpret_cast<ChainLine*>(win + o) =
        *reinterpret_cast<const ChainLine*>(seg.pos + win_lo + o);
    lim = uint32_t(bytes);
    __syncthreads();
  };
  while (b < pt.nfull && !bad) {
    if (cur + 8 > seg.pos_len) { bad = 1; break; }
    refill(cur);
    const uint32_t left = pt.nfull - b;
    uint32_t next;
    const uint32_t n = chain_orbit(win, s_chain, uint32_t(cur - win_lo), lim, seg.pos_len - win_lo,
                                   left < kChainCap ? left : kChainCap, s_hdr, &next, &bad,
                                   block_link{win});
    // a window from `cur` holds at least one whole block of a valid stream (<= 513 bytes)
    if (n == 0) bad = 1;
    // (offsets are kept in 32 bits: a term's positions beyond 4 GB are refused)
    if (n && win_lo + (s_hdr[n - 1] >> 8) - pt.pos_start > 0xFFFFFFFFull) bad = 1;
    for (uint32_t i = tid; i < n && !bad; i += kChainThreads) {
      const uint32_t rec = s_hdr[i];
      pblk_off[pt.row + b + i] = uint32_t(win_lo + (rec >> 8) - pt.pos_start);
      pblk_bits[pt.row + b + i] = uint8_t(rec);
    }
    b += n;
    cur = win_lo + next;
    __syncthreads();  // the window and the list are rewritten next
  }
  // where the writer says the tail starts (EndTerm :719-722; reader :2270-2278)
  if (!bad && pt.total > kBlock && pos_end[term] != cur - pt.pos_start) bad = 1;
  if (!bad && pt.tail_n) {
    if (cur + 1 > seg.pos_len) {
      bad = 1;
    } else {
      refill(cur);  // at most 127 vints of <= 5 bytes
      if (tid == 0) {
        uint64_t c = cur;
        uint32_t tb = 0;
        for (uint32_t i = 0; i < pt.tail_n; ++i) {
          if (c + 1 > seg.pos_len) { tb = 1; break; }
          uint32_t len;
          ptail[pt.tail_row + i] = vint_bytes(win + (c - win_lo), &len);
          c += len;
        }
        if (c > seg.pos_len) tb = 1;
        s_cur = c;
        s_bad = tb;
      }
      __syncthreads();
      cur = s_cur;
      bad = s_bad;
    }
  }
  if (tid == 0) {
    pterms[term].bytes = uint32_t(cur - pt.pos_start);
    if (bad) atomicOr(status, kStatusCorrupt);
  }
}

// Bit-exact test surface: every position of every doc of one term, doc after doc
// (what draining the position attribute behind doc_iterator::next yields).
// grid.x = nblk + 1 wave-sized items, kWaves per workgroup (as k_decode_term).
template<int LAYOUT>
__global__ void __launch_bounds__(kThreads)
k_decode_positions(DevSegment seg, uint32_t term, uint32_t* out) {
  const unsigned lane = threadIdx.x & 63u;
  const DevTerm t = seg.terms[term];
  const DevPosTerm pt = seg.pterms[term];
  const uint32_t item = blockIdx.x * kWaves + (threadIdx.x >> 6);
  uint32_t doc[2], tf[2] = {0u, 0u}, pidx[2] = {0u, 0u};
  if (item < t.nblk && t.docs_count > 1) {
    const uint64_t e = t.dir_off + item;
    const uint32_t bits = seg.blk_bits[e];
    decode_block<LAYOUT, true>(seg.doc + t.doc_start + seg.blk_off[e], bits & 0xFFu, bits >> 8,
                               0u, lane, doc[0], doc[1], tf[0], tf[1]);
    const uint32_t incl = wave::inclusive_scan(tf[0] + tf[1]);
    pidx[0] = seg.blk_pos[e] - seg.blk_pos[t.dir_off] + incl - tf[0] - tf[1];
    pidx[1] = pidx[0] + tf[0];
  } else if (item == t.nblk) {
    const uint32_t n = t.docs_count == 1 ? 1u : t.tail_n;
    const uint32_t base = seg.blk_pos[t.dir_off + t.nblk] - seg.blk_pos[t.dir_off];
    tail_pidx(seg, t.tail_row, n, base, lane, doc, tf, pidx);
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    uint32_t v = seg.pos_base;  // pos_limits::invalid() (+ pos_limits::min() in the one-based formats)
    for (uint32_t k = 0; k < tf[h]; ++k) {
      v += pos_delta<LAYOUT>(seg, pt, term, pidx[h] + k);
      out[pidx[h] + k] = v;
    }
  }
}

// ------------------------------------------------------------ query time --

constexpr uint32_t kPhraseWaves = 4;  // wavefronts (= lead blocks) per workgroup

// #{i < n : sorted[i] <= x}, knowing that it lies in [a, b]
__device__ __forceinline__ uint32_t count_le(const uint32_t* sorted, uint32_t a, uint32_t b,
                                             uint32_t x) {
  while (a < b) {
    const uint32_t mid = (a + b) >> 1;
    if (sorted[mid] <= x) a = mid + 1; else b = mid;
  }
  return a;
}


// by_phrase, block driven.  The conjunction PhraseIterator::next runs first
// (phrase_iterator.hpp:590-596) is bounded by its rarest member — the reason Conjunction
// sorts its iterators by cost (conjunction.hpp:450-453) and lets the cheapest LEAD while
// the others seek().  Here ONE WAVEFRONT owns one 128-posting block (or the vint tail)
// of the lead term (its record and the other terms' start blocks come from k_conj_seek):
//   1. it decodes the lead block: 128 ascending docs into LDS and into a bitmap over the
//      block's doc range (the lead frame, lead.h), (P, tf) of each into the lead's row;
//   2. for every other term it finds the blocks that can hold one of the docs every term
//      so far reached — what seek() does through the skip list (skip_list.hpp:208-249) — and
//      decodes them (the walk of follow_list, lead.h, here with position numbers AND two blocks in
//      flight); each decoded posting looks its doc up among the lead docs: a hit leaves (P, tf) in
//      the term's row at the doc's rank and marks the doc alive for the next term;
//   3. docs that every term reached are the conjunction's matches: compacted, one lane each
//      merges the terms' position lists (FixedPhraseFrequency::NextPosition,
//      phrase_iterator.hpp:109-151): phrase frequency = #{p in first term : p + off_i in
//      term i for all i};
//   4. matches are scored with tf = phrase frequency; those at or above the unit's threshold
//      bin (pilot pass: histogrammed instead) are appended to its candidates, one reservation
//      per wavefront.
// Wavefronts are independent (no workgroup barrier).  MT = compile-time bound of the phrase
// length (cursor state stays in registers).
// MATCH (match.h, unscored execution): steps 1-3 only — a doc with phrase frequency > 0 sets its bit
// in the unit's row of `sets32` (zeroed by the caller; matches are sparse: a global atomic) and
// counts for the unit; the position merge stops at the first match; no threshold, norm, score or
// candidate.  The scored instantiations compile to what they were without the parameter.
// REQ (k_phrase_and below): rows [n_phrase[unit], m) of the unit are REQUIRED TERMS — the by_term
// children of the irs::And that holds the phrase (IRS_HIP_PHRASE_REQUIRED) — see there.
// REQ == kPhraseOpt (k_phrase_or below): those rows are OPTIONAL TERMS — the by_term children of the
// irs::Or that holds the phrase (IRS_HIP_PHRASE_OPTIONAL): they never lead, drop no doc, and add
// their score where they hold a doc the phrase matches — see there.
constexpr int kPhraseReq = 1, kPhraseOpt = 2;   // (REQ: `true` is kPhraseReq)
template<int MT>
struct PhraseWave {
  uint32_t docs[kBlock];
  uint32_t pidx[MT][kBlock];          // first position number of the doc in term i's list
  uint32_t tf[MT][kBlock];            // its frequency there (0: the term has not reached the doc)
  alignas(16) uint8_t first[kConjBuckets];   // bucket -> 1 + entry index of its first lead doc (lead.h)
  uint32_t bm[3][kConjWords + 4];     // bitmaps over [dlo, dhi]: lead docs, alive / marked
  uint8_t lpre[kConjWords + 4];       // lead-bitmap bits in the words before word w
  uint8_t apre[kConjWords + 4];       // the same for the alive bitmap of the current term
  DevPosTerm pt[MT];                  // the merge stage's per-term records
  uint32_t term[MT];
  uint32_t off[MT];
};

template<int LAYOUT, int MT, bool MATCH = false, int REQ = 0>
__device__ __forceinline__ void phrase_item(const ConjArgs& A, uint32_t pilot /*1: histogram the
                                            scores of the sampled lead items, no candidates*/,
                                            PhraseWave<MT>* s_wave, uint32_t* sets32 = nullptr,
                                            uint64_t words32 = 0, unsigned long long* counts = nullptr,
                                            const uint32_t* n_phrase = nullptr /*REQ: [unit] phrase rows*/,
                                            uint32_t* taken = nullptr /*kPhraseOpt: [unit][words32] bit =
                                            doc id, zeroed per run: the docs the phrase matched*/) {
  constexpr bool OPT = REQ == kPhraseOpt;
  const uint32_t tid = threadIdx.x;
  const unsigned lane = tid & 63u;
  const uint32_t wv = wave::uniform(tid >> 6);
  uint32_t e = blockIdx.x * kPhraseWaves + wv;
  if (pilot) {
    if (e >= A.n_pilot) return;
    const PhraseWg w = A.wgs[e];
    e = wave::uniform(A.unit_items[w.unit] + w.first_item);
  } else if (e >= A.n_items) {
    return;
  }
  const ConjItem R = wave::sload<ConjItem>(reinterpret_cast<uint64_t>(A.recs) + uint64_t(e) * sizeof(ConjItem));
  const uint32_t unit = R.unit, item = R.item;
  const DevQuery qd = wave::sload<DevQuery>(reinterpret_cast<uint64_t>(A.queries) + uint64_t(unit) * sizeof(DevQuery));
  uint32_t m_all = qd.n_terms;
  if (m_all == 0 || m_all > uint32_t(MT)) return;
  // rows [0, mp) are the phrase's words (the lists step 3 merges), rows [mp, m) required terms
  uint32_t mp = m_all;
  if constexpr (REQ) {
    mp = wave::uniform(n_phrase[unit]);
    if (mp == 0u || mp > m_all) return;
    // (optional rows decide no match: the match-only form leaves them out altogether)
    if constexpr (OPT && MATCH) m_all = mp;
  }
  const uint32_t m = m_all;
  const DevSegment& seg = A.segs[qd.seg];   // (read field by field)
  const uint64_t tl_at = reinterpret_cast<uint64_t>(A.tails) + uint64_t(unit) * A.jt * sizeof(DevTail);
  auto term_tail = [&](uint32_t i) { return wave::sload<DevTail>(tl_at + i * sizeof(DevTail)); };
  const uint32_t lead = A.lead_of[unit];   // the term with the fewest postings leads
  const DevTail ld = term_tail(lead);
  const DevQTerm qt = A.qterms[qd.first_term];  // the phrase's scorer rides on its first term
  const uint32_t bs = (MATCH || pilot) ? 0u : A.bstar[unit];
  PhraseWave<MT>& W = s_wave[wv];
  uint32_t* docs = W.docs;
  const uint32_t* seek = A.seek + uint64_t(e) * (A.jt - 1u);
  if (lane < m) {   // what the position merges read, a lane per term
    const DevTail t = A.tails[uint64_t(unit) * A.jt + lane];
    W.pt[lane] = seg.pterms[t.term];
    W.term[lane] = t.term;
    if (!REQ || lane < mp) W.off[lane] = A.qterms[qd.first_term + lane].pad0;  // desired offset in the phrase
  }
  // REQ: the order the And's children are summed in — Conjunction sorts them by cost
  // (conjunction.hpp:450-453): the phrase costs its rarest word's docs_count (the front of its
  // approx_ conjunction, phrase_iterator.hpp:545-560), a term its own; ties in entry order.
  // W.off[mp + r] (no offset lives there) = the r-th cheapest required row, phrase_at = required
  // rows summed in front of the phrase.
  uint32_t phrase_at = 0;
  if constexpr (REQ == kPhraseReq) {
    uint32_t cost = 0xFFFFFFFFu;
    if (lane < m) {
      const DevTail t = A.tails[uint64_t(unit) * A.jt + lane];
      cost = t.nblk * kBlock + t.n;
    }
    uint32_t pcost = 0xFFFFFFFFu;
    for (uint32_t j = 0; j < mp; ++j) {
      const uint32_t cj = wave::read_lane(cost, j);
      pcost = cj < pcost ? cj : pcost;
    }
    uint32_t rank = 0;
    for (uint32_t j = mp; j < m; ++j) {
      const uint32_t cj = wave::read_lane(cost, j);
      rank += (cj < cost || (cj == cost && j < lane)) ? 1u : 0u;
      phrase_at += cj < pcost ? 1u : 0u;
    }
    if (lane >= mp && lane < m) W.off[mp + rank] = lane;
  }

  // ---- 1. the lead block: entry index 2*lane + h (block) or lane + 64*h (tail)
  uint32_t n = kBlock;
  uint32_t bytes = 0;   // (wave-uniform) encoded bytes of the doc blocks this wavefront decodes
  const bool counting = !pilot && A.touched != nullptr;   // (irs_hip_batch_profile bit 1)
  uint32_t ld_d[2], ld_e[2];
  bool live[2];   // the lane's lead docs that are docs of the segment at all (not deleted)
  {
    uint32_t f[2], p[2], estep;
    if (item < ld.nblk) {
      const uint64_t eb = ld.dir_off + item;
      if (counting) bytes += block_bytes(R.bits);
      uint32_t before;
      if (pk_both(R.bits & 0xFFu, R.bits >> 8)) {
        decode_packed_pos<LAYOUT>(seg.pk + (uint64_t(R.aoff) << 4), R.bits & 0xFFu, R.bits >> 8,
                                  R.base, lane, ld_d[0], ld_d[1], f[0], f[1], before);
      } else {
        decode_block_pos<LAYOUT>(seg.doc + ld.doc_start + R.off, R.bits & 0xFFu, R.bits >> 8,
                                 R.base, lane, ld_d[0], ld_d[1], f[0], f[1], before);
      }
      p[0] = seg.blk_pos[eb] - seg.blk_pos[ld.dir_off] + before;
      p[1] = p[0] + f[0];
      ld_e[0] = 2u * lane;
      estep = 1u;
    } else {
      n = ld.n;
      // positions in front of the tail = all frequencies of the full blocks (0 for a
      // list without blocks, whose dir_off has no rows of its own)
      const uint32_t base = seg.blk_pos[ld.dir_off + ld.nblk] - seg.blk_pos[ld.dir_off];
      tail_pidx(seg, ld.tail_row, n, base, lane, ld_d, f, p);
      ld_e[0] = lane;
      estep = 64u;
    }
    ld_e[1] = ld_e[0] + estep;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t idx = ld_e[h];
      docs[idx] = idx < n ? ld_d[h] : 0xFFFFFFFFu;
      // a deleted doc (SegmentReaderImpl::mask) keeps its place among the lead docs but counts as
      // not reached by the lead: it can never be a match
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
  const uint32_t dlo = wave::uniform(docs[0]), dhi = wave::uniform(docs[n - 1]);
  // bucket of a doc: (doc - dlo) >> s, below kConjBuckets (s = 0: one doc per bucket)
  const uint32_t span = dhi - dlo;
  const uint32_t s = span < kConjBuckets ? 0u
                     : 32u - uint32_t(__builtin_clz(span)) - (5u + uint32_t(__builtin_ctz(kConjWords)));
  const bool masked = qd.dead != nullptr;   // (wave-uniform)
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (ld_e[h] < n) {
      const uint32_t bk = (ld_d[h] - dlo) >> s;
      atomicOr(&W.bm[0][bk >> 5], 1u << (bk & 31u));
      // (conj.h: the first other term may only reach the LIVE lead docs)
      if (masked && live[h]) atomicOr(&W.bm[2][bk >> 5], 1u << (bk & 31u));
      // the bucket's first lead doc (entries are in doc order: its predecessor lies in another)
      if (ld_e[h] == 0u || ((docs[ld_e[h] - 1u] - dlo) >> s) != bk) W.first[bk] = uint8_t(ld_e[h] + 1u);
    }
  }
  wave::sync();
  // bits in the words before word w (lane: words 2*lane, 2*lane+1; [kConjWords] = all)
  auto prefix = [&](const uint32_t* bmap, uint8_t* pre) {
    uint32_t p0 = 0, p1 = 0;
    if (lane < kConjWords / 2u) {
      p0 = uint32_t(__builtin_popcount(bmap[2u * lane]));
      p1 = uint32_t(__builtin_popcount(bmap[2u * lane + 1u]));
    }
    const uint32_t incl = wave::inclusive_scan(p0 + p1);
    if (lane < kConjWords / 2u) {
      pre[2u * lane] = uint8_t(incl - p0 - p1);
      pre[2u * lane + 1u] = uint8_t(incl - p1);
    }
    if (lane == kConjWords / 2u - 1u) pre[kConjWords] = uint8_t(incl);
    wave::sync();
    return wave::read_lane(incl, 63);
  };
  prefix(W.bm[0], W.lpre);

  // ---- 2. the other terms
  uint32_t step = 0;   // terms done so far (the lead aside)
  for (uint32_t i = 0; i < m; ++i) {
    if (i == lead) continue;
    const DevTail tl = term_tail(i);
    // alive = docs every term so far reached: the lead bitmap, then what the previous term
    // marked; `mark` collects what this term reaches
    // (kPhraseOpt) an optional row reads what the LAST WORD left alive, marks nothing and leaves
    // `step` where it is: the next optional row reads the same bitmap
    const bool opt_row = OPT && i >= mp;
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
      if (prefix(alive, W.apre) == 0u) {   // no doc reached by every term so far: done
        if (!pilot && A.touched && lane == 0)
          atomicAdd(&A.touched[2u * unit], static_cast<unsigned long long>(bytes));
        return;
      }
    }
    if (!opt_row) ++step;
    const bool more_terms = MT > 2 && !opt_row && step + 1u < m;   // (the last term marks nothing: nobody reads it)
    const uint32_t n_before = (OPT && i > mp) ? mp : i;   // (an optional row: every WORD holds the doc)
    auto alive_below = [&](uint32_t x) {
      return uint32_t(apre[x >> 5]) + uint32_t(__builtin_popcount(alive[x >> 5] & ((1u << (x & 31u)) - 1u)));
    };
    // a decoded posting of term i: is its doc one of the lead docs still alive?
    auto put = [&](uint32_t doc, uint32_t f, uint32_t p) {
      const uint32_t x = doc - dlo;
      if (f == 0 || x > span) return;
      const uint32_t bk = x >> s;
      const uint32_t t = lead_index(W.first, docs, n, bk, s, doc);
      if (t == n) return;
      // every earlier term — and the lead, whose deleted docs count as not reached — holds THIS doc
      if (W.tf[lead][t] == 0u) return;
      for (uint32_t j = 0; j < n_before; ++j)
        if (j != lead && W.tf[j][t] == 0u) return;
      W.pidx[i][t] = p;
      W.tf[i][t] = f;
      if (more_terms) atomicOr(&mark[bk >> 5], 1u << (bk & 31u));   // (alive for the next term)
    };
    if (tl.nblk) {
      // (integer addresses: loads through the global address space, see raw_load_packed_g)
      const uint64_t last_at = reinterpret_cast<uint64_t>(seg.blk_last + tl.dir_off);
      const uint64_t dir_at = reinterpret_cast<uint64_t>(seg.blk_dir + tl.dir_off);
      const uint64_t pos_at = reinterpret_cast<uint64_t>(seg.blk_pos + tl.dir_off);
      const uint64_t pk_at = reinterpret_cast<uint64_t>(seg.pk);
      const uint32_t pos0 = seg.blk_pos[tl.dir_off];
      const uint32_t b_first = seek[i < lead ? i : i - 1u];
      for (uint32_t b0 = b_first; b0 < tl.nblk; b0 += 64) {
        const uint32_t bl = b0 + lane;
        const bool valid = bl < tl.nblk;
        // the block's last doc, its directory record (which also holds the preceding block's
        // last doc) and its first position number in ONE round trip (conj.h)
        const uint32_t lst = valid ? wave::gload_u32(last_at, bl * 4u) : 0xFFFFFFFFu;
        BlkDir d{};
        uint32_t pos_l = 0;
        if (valid) {
          uint32_t w[4];
          wave::gload_u32x4(dir_at, bl * uint32_t(sizeof(BlkDir)), w);
          d = BlkDir{w[0], w[1], w[2], w[3]};
          pos_l = wave::gload_u32(pos_at, bl * 4u);
        }
        const uint32_t prv = bl ? d.prev_last : 0u;   // the block holds docs in (prv, lst]
        const bool reach = valid && prv < dhi && lst >= dlo;
        bool want = false;
        if (reach) {
          const uint32_t x0 = prv + 1u > dlo ? prv + 1u - dlo : 0u;
          const uint32_t x1 = (lst < dhi ? lst : dhi) - dlo;
          want = alive_below((x1 >> s) + 1u) > alive_below(x0 >> s);
        }
        uint64_t mask = wave::ballot(want);
        const bool more = wave::ballot(valid && prv >= dhi) == 0;  // no block started behind dhi yet
        while (mask) {
          const uint32_t k = uint32_t(__builtin_ctzll(mask));
          mask &= mask - 1;
          const uint32_t bits = wave::read_lane(d.bits, k);
          if (counting) bytes += block_bytes(bits);
          const uint32_t base = wave::read_lane(d.prev_last, k);
          uint32_t d0, d1, f0, f1, before;
          const uint32_t dbits = bits & 0xFFu, fbits = bits >> 8;
          // two wanted blocks at a time where both live in the packed image: their payload
          // loads are in flight together
          if (mask && pk_both(dbits, fbits)) {
            const uint32_t k2 = uint32_t(__builtin_ctzll(mask));
            const uint32_t bits2 = wave::read_lane(d.bits, k2);
            if (pk_both(bits2 & 0xFFu, bits2 >> 8)) {
              mask &= mask - 1;
              if (counting) bytes += block_bytes(bits2);
              const uint64_t pl1 = pk_at + (uint64_t(wave::read_lane(d.aoff, k)) << 4);
              const uint64_t pl2 = pk_at + (uint64_t(wave::read_lane(d.aoff, k2)) << 4);
              uint64_t da1, db1, fa1, fb1, da2, db2, fa2, fb2;
              raw_load_packed_g<LAYOUT>(pl1, dbits, lane, da1, db1);
              raw_load_packed_g<LAYOUT>(pl1 + 16u * dbits, fbits, lane, fa1, fb1);
              raw_load_packed_g<LAYOUT>(pl2, bits2 & 0xFFu, lane, da2, db2);
              raw_load_packed_g<LAYOUT>(pl2 + 16u * (bits2 & 0xFFu), bits2 >> 8, lane, fa2, fb2);
              uint32_t x0, x1;
              extract_fast<LAYOUT>(da1, db1, dbits, lane, x0, x1);
              extract_fast<LAYOUT>(fa1, fb1, fbits, lane, f0, f1);
              uint32_t dsum = x0 + x1, fsum = f0 + f1;
              wave::inclusive_scan2(dsum, fsum);
              uint32_t p0 = wave::read_lane(pos_l, k) - pos0 + (fsum - f0 - f1);
              put(base + dsum - x1, f0, p0);
              put(base + dsum, f1, p0 + f0);
              extract_fast<LAYOUT>(da2, db2, bits2 & 0xFFu, lane, x0, x1);
              extract_fast<LAYOUT>(fa2, fb2, bits2 >> 8, lane, f0, f1);
              dsum = x0 + x1;
              fsum = f0 + f1;
              wave::inclusive_scan2(dsum, fsum);
              const uint32_t base2 = wave::read_lane(d.prev_last, k2);
              p0 = wave::read_lane(pos_l, k2) - pos0 + (fsum - f0 - f1);
              put(base2 + dsum - x1, f0, p0);
              put(base2 + dsum, f1, p0 + f0);
              continue;
            }
          }
          if (pk_both(dbits, fbits)) {
            // both parts 1..31-bit packed: the 16-byte aligned copy in the packed image,
            // one funnel shift + one bit-field extract per value (as k_score's hot loop)
            decode_packed_pos<LAYOUT>(seg.pk + (uint64_t(wave::read_lane(d.aoff, k)) << 4), dbits,
                                      fbits, base, lane, d0, d1, f0, f1, before);
          } else {
            decode_block_pos<LAYOUT>(seg.doc + tl.doc_start + wave::read_lane(d.off, k), dbits,
                                     fbits, base, lane, d0, d1, f0, f1, before);
          }
          const uint32_t p0 = wave::read_lane(pos_l, k) - pos0 + before;
          put(d0, f0, p0);
          put(d1, f1, p0 + f0);
        }
        if (!more) break;
      }
    }
    if (tl.n && tl.first_doc <= dhi && tl.last_doc >= dlo) {  // vint tail / single doc
      const uint32_t base = seg.blk_pos[tl.dir_off + tl.nblk] - seg.blk_pos[tl.dir_off];
      uint32_t d[2], f[2], p[2];
      tail_pidx(seg, tl.tail_row, tl.n, base, lane, d, f, p);
      put(d[0], f[0], p[0]);
      put(d[1], f[1], p[1]);
    }
    wave::sync();
  }

  // ---- 3./4. lead docs every term reached, compacted: merge the position lists, score, emit
  bool h01[2];
  uint64_t m01[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t sl = lane + 64u * uint32_t(h);
    bool all = sl < n;
    for (uint32_t i = 0; i < (OPT ? mp : m); ++i) all = all && W.tf[i][sl < n ? sl : 0u] != 0u;
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
  // (the fields the position merges read, in registers: through the reference every
  // pos_delta of the serial merge loops would load them again)
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
      uint32_t P[MT], T[MT], K[MT], V[MT];
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const bool on = uint32_t(i) < mp;
        P[i] = on ? W.pidx[i][sl] : 0u;
        T[i] = on ? W.tf[i][sl] : 0u;
        K[i] = 0u;
        V[i] = ps.pos_base;  // pos_limits::invalid() (+ min() before the first delta, one-based)
      }
      // Walking every position of the first term counts the same matches as the
      // reference's lead.seek(sought - offset), which only skips positions that cannot match.
      uint32_t pf = 0, head = ps.pos_base;
      bool done = false;
      if (REQ ? mp == 2u : (MT == 2 && m == 2u)) {
        // Two terms: ONE loop that reads one position per trip, of whichever list is behind
        // (the term's records selected per lane).  The nested form below costs a wavefront the
        // SUM over lead positions of the LONGEST seek among its 64 docs; this one the longest
        // tf_a + tf_b — what very frequent phrases (thousands of matching docs per block of
        // the lead) are bound by: 43 -> 36 ms per 1000 such queries.  (Keeping two deltas of
        // either list in flight was tried and is slower: the loop is bound by the instructions
        // of a random-access position read, not by its latency.)
        const DevPosTerm pa = W.pt[0], pb = W.pt[1];
        const uint32_t off = W.off[1];
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
          if (adv_a ? ka == T[0] : kb == T[1]) break;   // exhausted: no later position can match
          DevPosTerm pt;
          pt.pos_start = adv_a ? pa.pos_start : pb.pos_start;
          pt.row = adv_a ? pa.row : pb.row;
          pt.nfull = adv_a ? pa.nfull : pb.nfull;
          pt.tail_row = adv_a ? pa.tail_row : pb.tail_row;
          PosCursor cur = adv_a ? ca : cb;
          const uint32_t d = pos_delta_cached<LAYOUT>(ps, pt, cur, adv_a ? P[0] + ka : P[1] + kb);
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
        done = true;
      }
      for (uint32_t a = 0; a < T[0] && !done; ++a) {
        head += pos_delta<LAYOUT>(ps, W.pt[0], W.term[0], P[0] + a);  // lead.next()
        ++my_pos;
        bool match = true;
#pragma unroll
        for (int i = 1; i < MT; ++i) {
          if (uint32_t(i) < mp && match && !done) {
            const uint32_t target = head + W.off[i];
            if (target < head) { done = true; break; }  // !pos_limits::valid(term_position)
            // position::seek(target) :1578-1604
            // (value_ is invalid until the first position is read: K[i] == 0)
            while ((K[i] == 0u || V[i] < target) && K[i] < T[i]) {
              V[i] += pos_delta<LAYOUT>(ps, W.pt[i], W.term[i], P[i] + K[i]);
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
      if constexpr (MATCH) {
        if (pf) {
          doc = docs[sl];
          if (sets32) atomicOr(&sets32[uint64_t(unit) * words32 + (doc >> 5)], 1u << (doc & 31u));
          ++my_hits;
        }
      } else if (pf) {
        doc = docs[sl];
        // (a posting of the lead block: its norm from the posting-order copy of the column)
        const uint32_t nv = !seg.pnorm ? norm_value(seg, doc)
                            : (item < ld.nblk ? seg.pnorm[(ld.dir_off + item) * kBlock + sl]
                                              : seg.tail_norms[ld.tail_row + sl]);
        score = score_value(qt, pf, nv);
        if constexpr (OPT) {
          // + the score of every optional term that holds the doc, in entry order; the doc is
          // taken: the term pass will not see it (a global atomic: matches are sparse)
          if (mp < m) {
            for (uint32_t row = mp; row < m; ++row) {
              const uint32_t tfr = W.tf[row][sl];
              if (tfr) score += score_value(A.qterms[qd.first_term + row], tfr, nv);
            }
            if (taken) atomicOr(&taken[uint64_t(unit) * words32 + (doc >> 5)], 1u << (doc & 31u));
          }
        } else if constexpr (REQ) {
          // + every required term's own score at its frequency in the doc, in cost order (each
          // row's scorer read where it is used: up to 6 of them would not stay in registers)
          const uint32_t nreq = m - mp;
          float sum = phrase_at == 0u ? score : 0.f;
          for (uint32_t r = 0; r < nreq; ++r) {
            const uint32_t row = W.off[mp + r];
            const float v = score_value(A.qterms[qd.first_term + row], W.tf[row][sl], nv);
            sum = (r == 0u && phrase_at != 0u) ? v : sum + v;
            if (r + 1u == phrase_at) sum += score;
          }
          score = sum;
        }
        const uint32_t bin = score_bin(score, qd.bin_scale);
        if (pilot) atomicAdd(&A.hist[uint64_t(unit) * kBins + bin], 1u);
        else cand = bin >= bs;   // below the pilot's threshold bin: cannot be among the top k
        ++my_hits;
      }
    }
    // one reservation per wavefront for all its candidates of this pass
    const uint64_t cm = wave::ballot(cand);
    if (cm) {
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(&A.cand_count[unit], uint32_t(__builtin_popcountll(cm)));
      base = wave::read_lane(base, 0);
      const uint32_t slot = base + uint32_t(__builtin_popcountll(cm & below));
      if (cand && slot < A.cand_cap) A.cands[uint64_t(unit) * A.cand_cap + slot] = make_key(score, doc);
    }
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

template<int LAYOUT, int MT>
__global__ void __launch_bounds__(kPhraseWaves * 64)
k_phrase(ConjArgs A, uint32_t pilot) {
  __shared__ PhraseWave<MT> s_wave[kPhraseWaves];
  phrase_item<LAYOUT, MT>(A, pilot, s_wave);
}
// Two-word phrases (the usual case, BASELINE config 5) at the hardware's 8 wavefronts per SIMD: the
// kernel is a chain of dependent loads, resident wavefronts count for more than the 4 registers
// over 64 it would like (12 bytes of scratch): 7.34 -> 6.44 ms per 1000 phrases.  Longer phrases
// keep their registers (their LDS rows limit the occupancy anyway).
template<int LAYOUT>
__global__ void __launch_bounds__(kPhraseWaves * 64) RT_WAVES_PER_SIMD(8)
k_phrase2(ConjArgs A, uint32_t pilot) {
  __shared__ PhraseWave<2> s_wave[kPhraseWaves];
  phrase_item<LAYOUT, 2>(A, pilot, s_wave);
}


// And([by_phrase, by_term...]) — a phrase plus required terms (IRS_HIP_PHRASE_REQUIRED; the
// reference: And::prepare -> make_conjunction over {PhraseIterator, term iterators},
// boolean_filter.cpp:150-210, boolean_query.cpp:60-145, conjunction.hpp:436-490).  phrase_item with
// rows [n_phrase[unit], m) as required terms:
//   lead  the rarest of ALL rows; when a required term leads, every phrase word gets its (P, tf)
//         from step 2's `put`; the doc's norm still comes from the lead's posting-order copy;
//   2.    a required row is intersected like a phrase word (its P is stored and never read: the
//         LDS row of an MT-wide wavefront is there anyway);
//   3.    "reached by every row" runs over all rows, the position merge over the phrase rows only
//         (two words: the single loop); phrase frequency 0 = no match whatever the terms hold;
//   4.    score = phrase scorer at tf = phrase frequency + every required term's scorer at its own
//         tf, float32, children in cost order — into the bin, the pilot histogram and the key.
// A plain phrase of such a batch has no required rows: its score is the phrase's alone, bit for bit
// what k_phrase gives.  MT in {4, 8}: phrase words + required terms <= 8.
template<int LAYOUT, int MT>
__global__ void __launch_bounds__(kPhraseWaves * 64)
k_phrase_and(ConjArgs A, const uint32_t* n_phrase, uint32_t pilot) {
  __shared__ PhraseWave<MT> s_wave[kPhraseWaves];
  phrase_item<LAYOUT, MT, false, true>(A, pilot, s_wave, nullptr, 0, nullptr, n_phrase);
}


// Or([by_phrase, by_term...]) — a phrase or optional terms (IRS_HIP_PHRASE_OPTIONAL; the reference:
// Or::prepare, boolean_filter.cpp:150-210 -> MakeDisjunction over {PhraseIterator, term iterators},
// disjunction.hpp:1411-1467).  This is the PHRASE PASS of such a unit: every doc the phrase matches,
// scored in full.  phrase_item with rows [n_phrase[unit], m) as optional terms:
//   lead  the rarest WORD (build_phrase_work); an optional row never leads;
//   2.    an optional row is probed like a word — against the docs every WORD reached — but marks
//         nothing alive and drops nothing;
//   3.    "reached by every row" and the position merge run over the words only;
//   4.    score = phrase scorer at tf = phrase frequency + the scorer of every optional row that
//         holds the doc at its own tf, float32, entry order — into the bin, the pilot histogram and
//         the key; the doc's bit is set in the unit's row of `taken` (zeroed per run).  k_not_words
//         turns the rows into the doc sets the TERM PASS (a plain disjunction of the optional terms
//         on the work-item path, a batch of its own behind this one) is restricted to: the two
//         passes emit disjoint docs.
// A plain phrase of such a batch has no optional rows: bit for bit what k_phrase gives.
template<int LAYOUT, int MT>
__global__ void __launch_bounds__(kPhraseWaves * 64)
k_phrase_or(ConjArgs A, const uint32_t* n_phrase, uint32_t* taken, uint64_t words32, uint32_t pilot) {
  __shared__ PhraseWave<MT> s_wave[kPhraseWaves];
  phrase_item<LAYOUT, MT, false, kPhraseOpt>(A, pilot, s_wave, nullptr, words32, nullptr, n_phrase, taken);
}

// taken -> not taken, in place: the rows of `taken` as doc sets (bit set = the doc may match)
__global__ void __launch_bounds__(kThreads)
k_not_words(uint32_t* words, uint64_t n) {
  const uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i < n) words[i] = ~words[i];
}

// The union of the two passes of a batch with optional terms, a thread per hit: both lists of a unit
// are sorted as make_key sorts (score descending, doc ascending) and hold disjoint docs, so a hit's
// place in the union is its own index plus the hits of the other list in front of it (a binary
// search).  out[unit] = the first min(k, ca + cb) of the union; total = both passes' totals.
__global__ void __launch_bounds__(kThreads)
k_union_topk(const DevQuery* queries, uint32_t k_max, const Hit* a, const uint32_t* ca,
             const unsigned long long* ta, const Hit* b, const uint32_t* cb, const unsigned long long* tb,
             Hit* out, uint32_t* out_count, unsigned long long* out_total) {
  const uint32_t unit = blockIdx.x;
  const uint32_t k = queries[unit].k;
  const uint32_t na = ca[unit] < k_max ? ca[unit] : k_max, nb = cb[unit] < k_max ? cb[unit] : k_max;
  const Hit* la = a + uint64_t(unit) * k_max;
  const Hit* lb = b + uint64_t(unit) * k_max;
  Hit* o = out + uint64_t(unit) * k_max;
  const uint32_t keep = (na + nb < k ? na + nb : k) < k_max ? (na + nb < k ? na + nb : k) : k_max;
  for (uint32_t i = threadIdx.x; i < na + nb; i += kThreads) {
    const bool from_a = i < na;
    const uint32_t at = from_a ? i : i - na;
    const Hit h = from_a ? la[at] : lb[at];
    const uint64_t key = make_key(h.score, h.doc);
    const Hit* other = from_a ? lb : la;
    uint32_t lo = 0, hi = from_a ? nb : na;   // hits of the other list in front of this one
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (make_key(other[mid].score, other[mid].doc) > key) lo = mid + 1; else hi = mid;
    }
    if (at + lo < keep) o[at + lo] = h;
  }
  if (threadIdx.x == 0) {
    out_count[unit] = keep;
    out_total[unit] = ta[unit] + tb[unit];
  }
}

}  // namespace irs_hip
