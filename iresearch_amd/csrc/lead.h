// lead.h — what the block-driven kernels share: k_conj (conj.h), k_conj_any (conj_any.h), k_vphrase*
// (vphrase.h) and, for the records and the doc-block decoders only, k_phrase* (phrase.h, match.h):
// phrase_item keeps its own text of the frame and the walk, instruction for instruction — through
// the shared walk k_phrase2 ran 0.5 - 1.6 % slower at unchanged registers, LDS and occupancy
// (profiles/lead_walk_ab.txt).
//
// ONE WAVEFRONT owns one lead item — a 128-posting block, or the decoded vint tail, of the unit's
// cheapest list (ConjItem, written by k_conj_seek / k_vphrase_seek) — and walks every other list (a
// FOLLOWER) for the docs of that item which are still alive.  Two things are the same in all of them:
//
// THE LEAD FRAME.  The item's docs, ascending, lie in a wavefront's `docs[n]` in LDS.  Their range
// [dlo, dhi] is cut into kConjBuckets buckets of 2^s docs (s = 0 when the range is that small;
// LeadFrame).  Per bucket: the entry index of its FIRST lead doc (`first`, 0 = none) — "is this
// decoded posting's doc a lead doc, and which" is one byte read, a walk over the bucket's lead docs
// (1.1 on average) and a compare (lead_index), where a search of the sorted docs walks seven
// dependent reads (round 6: the search ran for ~every decoded block of a sparse lead, a third of
// k_conj's instructions).  And one BIT per bucket in doc-range bitmaps of kConjWords words, with the
// bits in front of every word counted once per bitmap (bitmap_prefix): "does this block of the
// follower hold a doc still alive" is two prefix-count reads for a directory record (alive_below).
// k_conj (and phrase_item) keep a lead bitmap and two that alternate (what the current follower
// reaches is alive for the next); conj_any_item and vphrase_item keep the alive docs in the lanes and
// rebuild one bitmap from them (alive_rebuild).
//
// THE FOLLOWER WALK (follow_list): from a start block on, 64 directory records per round, a lane
// each; a block is wanted when some alive bucket touches its doc range (previous last, last]; the
// wanted blocks are decoded and every posting handed to the kernel's `put`; the walk ends with the
// round in which a block starts at or behind dhi; then the list's decoded tail.  It is the one place
// that decides which blocks of a follower can hold a doc that is still alive.  What a posting MEANS
// (which row it lands in, whether earlier followers must have reached the doc, whether it marks the
// doc alive for the next) is the `put` of each kernel.
//
// The functions below take the LDS arrays they work on (the four wavefront records differ) and, but
// for the two between the phases of alive_rebuild, hold no wave::sync(): every kernel places its own
// between what its lanes write and what they read across lanes.
#pragma once
#include "score.h"

namespace irs_hip {

constexpr uint32_t kConjWords = 32;   // 32-bit words of a wavefront's doc-range bitmaps: 1024 buckets
constexpr uint32_t kConjBuckets = 32u * kConjWords;

// One entry of a pilot list: a sampled lead item of a unit.
struct PhraseWg {
  uint32_t unit;        // (segment, query) execution unit
  uint32_t first_item;  // index of the lead item
};

// A wavefront's bucket table: the entry index (< n) of lead doc `doc` of bucket bk, or n: not a
// lead doc
__device__ __forceinline__ uint32_t lead_index(const uint8_t* first, const uint32_t* docs, uint32_t n,
                                               uint32_t bk, uint32_t s, uint32_t doc) {
  uint32_t t = first[bk];
  if (!t) return n;
  --t;
  if (s) {   // (wave-uniform) a bucket may hold several lead docs, in entry order
    while (docs[t] < doc && t + 1u < n) ++t;
  }
  return docs[t] == doc ? t : n;
}
struct alignas(16) ConjQuad {   // 16 bytes cleared at once
  uint32_t x, y, z, w;
};

// One lead item (a 128-posting block of the conjunction's rarest term, or its decoded vint
// tail), everything its wavefront needs to start decoding — written by the pre-pass so that
// the wavefront's first load is this record (one scalar load) instead of a chain of dependent
// ones (unit -> query -> term record -> directory words).
// A lead block whose docs spread over many blocks of the other terms (a rare lead against frequent
// terms: the reference's AndHighLow) is cut into 2^lg lead items of 128 >> lg consecutive postings:
// one wavefront would decode up to 128 blocks per other term one after the other, a chain of
// dependent loads with nobody to overlap it.
constexpr uint32_t kConjItemBlock = 0xFFFFFFu;   // ConjItem::item: block index (nblk <= 2^24)
constexpr uint32_t kConjSplitMax = 4;            //   | piece << 24 | lg << 28: 16 pieces at most
struct alignas(32) ConjItem {
  uint32_t unit;
  uint32_t item;    // block index in the lead's list; == its nblk: the vint tail (+ piece, lg above)
  uint32_t base;    // doc the block's first delta is relative to (formats_10.cpp:636)
  uint32_t r_lo;    // the item's docs lie in [r_lo, r_hi] (from the directory)
  uint32_t r_hi;
  uint32_t aoff;    // block in the packed-payload image, 16-byte units
  uint32_t bits;    // header bytes: dbits | fbits << 8
  uint32_t off;     // block in `.doc`, relative to the term's doc_start
};
static_assert(sizeof(ConjItem) == 32, "one s_load_dwordx8 per lead item");

// Pre-pass, one thread per lead item of every conjunction: the item's record, and where the
// other terms start for it — the binary search of a term's block directory for the first
// block reaching the lead item's first doc, SkipReader::Seek (skip_list.hpp:208-249), done
// once per (lead item, term) by ONE THREAD (inside k_conj a wavefront would walk the same
// dependent chain 64 lanes wide).  seek[(item_base + item) * (jt - 1) + slot of term i among the non-lead terms].
__global__ void __launch_bounds__(kThreads)
k_conj_seek(const DevSegment* segs, const DevQuery* queries, const DevTail* tails, uint32_t jt,
            const uint32_t* conj_units, const uint32_t* item_base /*[n_conj + 1]*/,
            uint32_t n_conj, const uint32_t* lead_of /*[unit] slot of the lead term; null: 0*/,
            const uint32_t* split_lg /*[n_conj] log2 of the pieces per lead block; null: 0*/,
            uint32_t* seek, ConjItem* recs) {
  const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= item_base[n_conj]) return;
  uint32_t lo = 0, hi = n_conj;   // the unit whose items hold t: last c with item_base[c] <= t
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (item_base[mid] <= t) lo = mid; else hi = mid;
  }
  const uint32_t lg = split_lg ? split_lg[lo] : 0u;
  const uint32_t unit = conj_units[lo], item = (t - item_base[lo]) >> lg;
  const uint32_t piece = (t - item_base[lo]) & ((1u << lg) - 1u);
  const DevQuery qd = queries[unit];
  const DevSegment& seg = segs[qd.seg];
  const DevTail* tl = tails + uint64_t(unit) * jt;
  const uint32_t lead = lead_of ? lead_of[unit] : 0u;
  const DevTail ld = tl[lead];
  ConjItem r{};
  r.unit = unit;
  r.item = item | (piece << 24) | (lg << 28);
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
  for (uint32_t i = 0; i < qd.n_terms; ++i) {   // row: the other terms in slot order
    if (i == lead) continue;
    const uint32_t* last = seg.blk_last + tl[i].dir_off;
    uint32_t a = 0, b = tl[i].nblk;  // lower_bound(last, r_lo)
    while (a < b) {
      const uint32_t mid = (a + b) >> 1;
      if (last[mid] < r.r_lo) a = mid + 1; else b = mid;
    }
    seek[uint64_t(t) * (jt - 1u) + (i < lead ? i : i - 1u)] = a;
  }
}

struct ConjArgs {
  const DevSegment* segs;
  const DevQuery* queries;
  const DevQTerm* qterms;
  const PhraseWg* wgs;          // pilot pass: {unit, lead item} per wavefront (the sampled items)
  uint32_t n_pilot;             // entries of the pilot list
  uint32_t n_items;             // full pass: lead items of all conjunctions (= records)
  const DevTail* tails;         // [unit][jt] (k_plan)
  const uint32_t* bstar;        // threshold bin per unit (0 = none)
  const uint32_t* seek;         // k_conj_seek
  const ConjItem* recs;         // k_conj_seek
  const uint32_t* unit_items;   // [nq] first record of the unit's lead items (conj units)
  const uint32_t* lead_of;      // [nq] by_phrase: slot of the unit's lead (rarest) term
  uint64_t* cands;
  uint32_t* cand_count;
  unsigned long long* hits;
  uint32_t* item_hits;          // [n_items] matches of every lead item (full pass; zeroed per run):
                                // a store instead of an atomic on the unit's counter — one hot
                                // address per unit kept every wavefront resident until its atomic
                                // had come back (1.6 of 6.4 ms per 1000 AND-2 queries);
                                // k_conj_hits adds them up
  unsigned long long* touched;  // [unit][2]: `.doc` + norm bytes actually decoded / read (full
                                // pass; per unit: one hot address would serialise the atomics);
                                // null unless the batch counts (irs_hip_batch_profile bit 1)
  uint32_t* hist;               // [unit][kBins], pilot pass only
  uint32_t jt;
  uint32_t cand_cap;
  uint32_t pilot_stride;        // pilot pass: lead items {phase, phase + P, ...}
  uint32_t wand;                // prune lead blocks by block-max bounds
  uint32_t* pruned;             // [unit] set when a lead block was skipped (k_select's underflow check)
  // doc sets (irs_hip_batch_doc_set_stats), counted like `touched` (null unless the batch counts):
  // lead pieces of the units whose mask comes from a doc set (`restricted`: [unit] bytes), and how
  // many of them held no doc the mask leaves
  unsigned long long* leads;    // [2]
  const uint8_t* restricted;
};

// A lead piece of a masked unit, decoded, none of whose docs the mask leaves (one wave-uniform
// ballot of the lanes' `live`) ends there — nothing of it can match: no other term is sought or
// decoded, no position read; its hit count, candidate slots and pilot contribution stay zero.  What
// an exhausted `alive` bitmap tells a few steps later (and all a unit masked by deletions or
// exclusions alone ever sees of this: the same results); a doc set empties whole doc ranges.
// lead_skipped: what such a piece leaves behind in a counting run.  Its atomics sit on the path
// that ends the wavefront, nowhere else: a write to memory in front of the kernels' other loads
// would turn their scalar loads into vector loads (the compiler could no longer take the tables for
// unwritten) — which is why the pieces themselves are counted by k_count_leads, not here.
__device__ __forceinline__ void lead_skipped(const ConjArgs& A, uint32_t unit, bool counting, uint32_t bytes,
                                             unsigned lane) {
  if (counting && lane == 0) {
    atomicAdd(&A.touched[2u * unit], static_cast<unsigned long long>(bytes));
    if (A.leads && A.restricted[unit]) atomicAdd(&A.leads[1], 1ull);
  }
}
// A counting run of a batch with doc sets: the lead pieces (records) of its restricted units
__global__ void __launch_bounds__(kThreads)
k_count_leads(const ConjItem* recs, uint32_t n, const uint8_t* restricted, unsigned long long* leads) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  const bool on = i < n && restricted[recs[i].unit];
  const uint32_t c = uint32_t(__builtin_popcountll(wave::ballot(on)));
  if ((threadIdx.x & 63u) == 0 && c) atomicAdd(&leads[0], static_cast<unsigned long long>(c));
}

// ------------------------------------------------------------ doc blocks --

// Doc block `e` of a term, from the packed image when both parts live there (one funnel
// shift + one bit-field extract per value), else from `.doc` (any framing).
template<int LAYOUT>
__device__ __forceinline__ void decode_dir_block(const DevSegment& seg, uint64_t doc_start,
                                                 uint32_t bits, uint32_t off, uint32_t aoff,
                                                 uint32_t base, unsigned lane, uint32_t& d0,
                                                 uint32_t& d1, uint32_t& f0, uint32_t& f1) {
  const uint32_t dbits = bits & 0xFFu, fbits = bits >> 8;
  if (pk_both(dbits, fbits)) {
    const uint64_t pl = reinterpret_cast<uint64_t>(seg.pk) + (uint64_t(aoff) << 4);
    uint64_t da, db, fa, fb;
    raw_load_packed_g<LAYOUT>(pl, dbits, lane, da, db);
    raw_load_packed_g<LAYOUT>(pl + 16u * dbits, fbits, lane, fa, fb);
    uint32_t x0, x1;
    extract_fast<LAYOUT>(da, db, dbits, lane, x0, x1);
    extract_fast<LAYOUT>(fa, fb, fbits, lane, f0, f1);
    d1 = base + wave::inclusive_scan(x0 + x1);
    d0 = d1 - x1;
  } else {
    decode_block<LAYOUT, true>(seg.doc + doc_start + off, dbits, fbits, base, lane, d0, d1, f0, f1);
  }
}

// decode_block (decode.h) for a field with positions: absolute docs d0/d1 and frequencies
// f0/f1 of postings 2*lane, 2*lane+1, and `before` = sum of the frequencies of the block's
// postings in front of 2*lane (where this lane's positions start inside the block).  The two
// prefix sums run as one interleaved chain.
template<int LAYOUT>
__device__ __forceinline__ void decode_block_pos(const uint8_t* blk, uint32_t dbits,
                                                 uint32_t fbits, uint32_t base, unsigned lane,
                                                 uint32_t& d0, uint32_t& d1, uint32_t& f0,
                                                 uint32_t& f1, uint32_t& before) {
  uint32_t x0, x1;
  const uint32_t size = read_block_pair<LAYOUT>(blk, dbits, lane, x0, x1);
  read_block_pair<LAYOUT>(blk + size, fbits, lane, f0, f1);
  uint32_t dsum = x0 + x1, fsum = f0 + f1;
  wave::inclusive_scan2(dsum, fsum);
  d1 = base + dsum;
  d0 = d1 - x1;
  before = fsum - f0 - f1;
}

// The same from the packed-payload image (both parts 1..31-bit packed, pk_both()):
// 16-byte aligned payloads, one funnel shift + one bit-field extract per value, as k_score's
// hot loop reads them.
template<int LAYOUT>
__device__ __forceinline__ void decode_packed_pos(const uint8_t* pl, uint32_t dbits,
                                                  uint32_t fbits, uint32_t base, unsigned lane,
                                                  uint32_t& d0, uint32_t& d1, uint32_t& f0,
                                                  uint32_t& f1, uint32_t& before) {
  uint64_t da, db, fa, fb;
  const uint64_t at = reinterpret_cast<uint64_t>(pl);
  raw_load_packed_g<LAYOUT>(at, dbits, lane, da, db);
  raw_load_packed_g<LAYOUT>(at + 16u * dbits, fbits, lane, fa, fb);
  uint32_t x0, x1;
  extract_fast<LAYOUT>(da, db, dbits, lane, x0, x1);
  extract_fast<LAYOUT>(fa, fb, fbits, lane, f0, f1);
  uint32_t dsum = x0 + x1, fsum = f0 + f1;
  wave::inclusive_scan2(dsum, fsum);
  d1 = base + dsum;
  d0 = d1 - x1;
  before = fsum - f0 - f1;
}

// decode_dir_block with `before`
template<int LAYOUT>
__device__ __forceinline__ void decode_dir_block_pos(const DevSegment& seg, uint64_t doc_start,
                                                     uint32_t bits, uint32_t off, uint32_t aoff,
                                                     uint32_t base, unsigned lane, uint32_t& d0,
                                                     uint32_t& d1, uint32_t& f0, uint32_t& f1,
                                                     uint32_t& before) {
  const uint32_t dbits = bits & 0xFFu, fbits = bits >> 8;
  if (pk_both(dbits, fbits)) {
    decode_packed_pos<LAYOUT>(seg.pk + (uint64_t(aoff) << 4), dbits, fbits, base, lane, d0, d1, f0, f1,
                              before);
  } else {
    decode_block_pos<LAYOUT>(seg.doc + doc_start + off, dbits, fbits, base, lane, d0, d1, f0, f1, before);
  }
}

// (P, tf) of the tail postings this lane owns: entries `lane` and `lane + 64` of the
// decoded tail (or the single doc).  base = positions in front of the tail.
__device__ __forceinline__ void tail_pidx(const DevSegment& seg, uint32_t row, uint32_t n,
                                          uint32_t base, unsigned lane, uint32_t (&doc)[2],
                                          uint32_t (&tf)[2], uint32_t (&pidx)[2]) {
  tf[0] = lane < n ? seg.tail_freqs[row + lane] : 0u;
  tf[1] = lane + 64u < n ? seg.tail_freqs[row + lane + 64u] : 0u;
  doc[0] = lane < n ? seg.tail_docs[row + lane] : 0u;
  doc[1] = lane + 64u < n ? seg.tail_docs[row + lane + 64u] : 0u;
  const uint32_t ia = wave::inclusive_scan(tf[0]);
  const uint32_t ta = wave::bcast(ia, 63);
  const uint32_t ib = wave::inclusive_scan(tf[1]);
  pidx[0] = base + ia - tf[0];
  pidx[1] = base + ta + ib - tf[1];
}

// Encoded bytes of a doc block: header bytes + payloads (all-equal: ~1 byte of vint) — what a
// counting run (ConjArgs::touched) adds per decoded block
__device__ __forceinline__ uint32_t block_bytes(uint32_t bits) {
  const uint32_t db = bits & 0xFFu, fb = bits >> 8;
  return 2u + (db ? 16u * db : 1u) + (fb ? 16u * fb : 1u);
}

// ------------------------------------------------------------ the lead item --

// The record index of this wavefront's lead item, or kNoItem.  Pilot pass: the sampled items'
// records, through the pilot list.
constexpr uint32_t kNoItem = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t lead_item_of(const ConjArgs& A, uint32_t pilot, uint32_t waves_per_wg) {
  const uint32_t e = blockIdx.x * waves_per_wg + wave::uniform(threadIdx.x >> 6);
  if (pilot) {
    if (e >= A.n_pilot) return kNoItem;
    const PhraseWg w = A.wgs[e];
    return wave::uniform(A.unit_items[w.unit] + w.first_item);
  }
  return e < A.n_items ? e : kNoItem;
}

// The lead item decoded: block `item` of list `ld` through its record, or the list's tail.  The
// lane's two docs d[h] and frequencies f[h] are entries e[h] of the item: 2*lane + h of a block,
// lane + 64*h of a tail.  Returns the item's postings; a counting run adds the block's bytes.
template<int LAYOUT>
__device__ __forceinline__ uint32_t lead_decode(const DevSegment& seg, const DevTail& ld, const ConjItem& R,
                                                uint32_t item, unsigned lane, bool counting, uint32_t& bytes,
                                                uint32_t (&d)[2], uint32_t (&e)[2], uint32_t (&f)[2]) {
  if (item < ld.nblk) {
    decode_dir_block<LAYOUT>(seg, ld.doc_start, R.bits, R.off, R.aoff, R.base, lane, d[0], d[1], f[0], f[1]);
    if (counting) bytes += block_bytes(R.bits);
    e[0] = 2u * lane;
    e[1] = e[0] + 1u;
    return kBlock;
  }
  const uint32_t n = ld.n;
  d[0] = lane < n ? seg.tail_docs[ld.tail_row + lane] : 0u;
  d[1] = lane + 64u < n ? seg.tail_docs[ld.tail_row + lane + 64u] : 0u;
  f[0] = lane < n ? seg.tail_freqs[ld.tail_row + lane] : 0u;
  f[1] = lane + 64u < n ? seg.tail_freqs[ld.tail_row + lane + 64u] : 0u;
  e[0] = lane;
  e[1] = e[0] + 64u;
  return n;
}
// ... of a field with positions: p[h] = the number of the doc's first position in the list
template<int LAYOUT>
__device__ __forceinline__ uint32_t lead_decode_pos(const DevSegment& seg, const DevTail& ld, const ConjItem& R,
                                                    uint32_t item, unsigned lane, bool counting, uint32_t& bytes,
                                                    uint32_t (&d)[2], uint32_t (&e)[2], uint32_t (&f)[2],
                                                    uint32_t (&p)[2]) {
  if (item < ld.nblk) {
    if (counting) bytes += block_bytes(R.bits);
    uint32_t before;
    decode_dir_block_pos<LAYOUT>(seg, ld.doc_start, R.bits, R.off, R.aoff, R.base, lane, d[0], d[1], f[0],
                                 f[1], before);
    p[0] = seg.blk_pos[ld.dir_off + item] - seg.blk_pos[ld.dir_off] + before;
    p[1] = p[0] + f[0];
    e[0] = 2u * lane;
    e[1] = e[0] + 1u;
    return kBlock;
  }
  // positions in front of the tail = all frequencies of the full blocks (0 for a
  // list without blocks, whose dir_off has no rows of its own)
  const uint32_t base = seg.blk_pos[ld.dir_off + ld.nblk] - seg.blk_pos[ld.dir_off];
  tail_pidx(seg, ld.tail_row, ld.n, base, lane, d, f, p);
  e[0] = lane;
  e[1] = e[0] + 64u;
  return ld.n;
}

// `first` cleared, every lane its 16 bytes
__device__ __forceinline__ void lead_first_clear(uint8_t* first, unsigned lane) {
  static_assert(kConjBuckets == 64u * 16u, "one 16-byte store per lane clears `first`");
  reinterpret_cast<ConjQuad*>(first)[lane] = ConjQuad{0u, 0u, 0u, 0u};
}

// The doc range of a lead item's n docs and its buckets: bucket of a doc = (doc - dlo) >> s, below
// kConjBuckets (s = 0: one doc per bucket)
struct LeadFrame {
  uint32_t dlo, dhi;
  uint32_t span;   // dhi - dlo
  uint32_t s;
  __device__ __forceinline__ uint32_t bucket(uint32_t doc) const { return (doc - dlo) >> s; }
};
__device__ __forceinline__ LeadFrame lead_frame(const uint32_t* docs, uint32_t n) {
  LeadFrame fr;
  fr.dlo = wave::uniform(docs[0]);
  fr.dhi = wave::uniform(docs[n - 1]);
  fr.span = fr.dhi - fr.dlo;
  fr.s = fr.span < kConjBuckets ? 0u
         : 32u - uint32_t(__builtin_clz(fr.span)) - (5u + uint32_t(__builtin_ctz(kConjWords)));
  return fr;
}

// `first` of the buckets whose first lead doc is one of this lane's (entries are in doc order: such
// a doc's predecessor lies in another bucket)
__device__ __forceinline__ void lead_first_fill(const LeadFrame& fr, uint8_t* first, const uint32_t* docs,
                                                const uint32_t (&ld_d)[2], const uint32_t (&ld_e)[2],
                                                uint32_t n) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (ld_e[h] < n) {
      const uint32_t bk = fr.bucket(ld_d[h]);
      if (ld_e[h] == 0u || fr.bucket(docs[ld_e[h] - 1u]) != bk) first[bk] = uint8_t(ld_e[h] + 1u);
    }
  }
}

// pre[w] = bits of bmap in the words before word w (lane: words 2*lane, 2*lane+1), pre[kConjWords]
// = all of them, which is also what every lane gets back
__device__ __forceinline__ uint32_t bitmap_prefix(const uint32_t* bmap, uint8_t* pre, unsigned lane) {
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
  return wave::read_lane(incl, 63);
}

// bits of bmap in the buckets below x, 0 <= x <= kConjBuckets (the bitmaps have slack words)
__device__ __forceinline__ uint32_t alive_below(const uint32_t* bmap, const uint8_t* pre, uint32_t x) {
  return uint32_t(pre[x >> 5]) + uint32_t(__builtin_popcount(bmap[x >> 5] & ((1u << (x & 31u)) - 1u)));
}

// The alive bitmap `bm` (kConjWords + 4 words) from the lanes' alive entries, and its prefix counts:
// returns the number of alive buckets.  Cleared, marked and counted by different lanes, hence the
// two syncs; the caller's follows, as for bitmap_prefix.
__device__ __forceinline__ uint32_t alive_rebuild(const LeadFrame& fr, uint32_t* bm, uint8_t* apre,
                                                  const uint32_t (&ld_d)[2], const bool (&alive)[2],
                                                  unsigned lane) {
  if (lane < (kConjWords + 4u) / 2u) {
    bm[2u * lane] = 0u;
    bm[2u * lane + 1u] = 0u;
  }
  wave::sync();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (alive[h]) {
      const uint32_t bk = fr.bucket(ld_d[h]);
      atomicOr(&bm[bk >> 5], 1u << (bk & 31u));
    }
  }
  wave::sync();
  return bitmap_prefix(bm, apre, lane);
}

// Rows of a grouped unit (conj_any.h groups, vphrase.h parts): bit r of `opens` is set when row r
// opens a group (bit 0 always); rows [group_lo(r), group_end(r)) form the group of row r of m
__device__ __forceinline__ uint32_t group_lo(uint32_t opens, uint32_t r) {
  return 31u - uint32_t(__builtin_clz(opens & ((2u << r) - 1u)));
}
__device__ __forceinline__ uint32_t group_end(uint32_t opens, uint32_t r, uint32_t m) {
  const uint32_t above = opens & ~((2u << r) - 1u) & ((1u << m) - 1u);
  return above ? uint32_t(__builtin_ctz(above)) : m;
}

// ------------------------------------------------------------ a follower --

// One follower list `tl` against the lead frame: its full blocks from b_first on (the seek table's
// start block, or further on), then its decoded tail.  alive / apre: the bitmap of the docs still
// alive and its prefix counts.  Every posting of a wanted block goes to put(doc, f) — POS:
// put(doc, f, p), p = the number of the doc's first position in the list, which costs the walk the
// block's blk_pos beside its directory record.  PAIR (not with POS): two wanted blocks at a time
// where both live in the packed image.  `bytes` grows by the decoded blocks' encoded size in a counting run.
template<int LAYOUT, bool POS, bool PAIR, typename Put>
__device__ __forceinline__ void follow_list(const DevSegment& seg, const DevTail& tl, uint32_t b_first,
                                            const LeadFrame& fr, const uint32_t* alive, const uint8_t* apre,
                                            bool counting, uint32_t& bytes, unsigned lane, Put&& put) {
  // (the fixed phrase kernels, which would be POS with PAIR, keep a walk of their own: phrase.h)
  static_assert(!(POS && PAIR), "two blocks in flight: without position numbers only");
  const uint32_t dlo = fr.dlo, dhi = fr.dhi, s = fr.s;
  if (tl.nblk) {
    // (integer addresses: loads through the global address space, see raw_load_packed_g)
    const uint64_t last_at = reinterpret_cast<uint64_t>(seg.blk_last + tl.dir_off);
    const uint64_t dir_at = reinterpret_cast<uint64_t>(seg.blk_dir + tl.dir_off);
    const uint64_t pos_at = POS ? reinterpret_cast<uint64_t>(seg.blk_pos + tl.dir_off) : 0u;
    const uint64_t pk_at = reinterpret_cast<uint64_t>(seg.pk);
    const uint32_t pos0 = POS ? seg.blk_pos[tl.dir_off] : 0u;
    // a wanted block of the packed image, its payload words loaded: the lane's two postings
    auto put_packed = [&](uint64_t da, uint64_t db, uint64_t fa, uint64_t fb, uint32_t bits, uint32_t base) {
      if constexpr (!POS) {
        uint32_t x0, x1, f0, f1;
        extract_fast<LAYOUT>(da, db, bits & 0xFFu, lane, x0, x1);
        extract_fast<LAYOUT>(fa, fb, bits >> 8, lane, f0, f1);
        const uint32_t d1 = base + wave::inclusive_scan(x0 + x1);
        put(d1 - x1, f0);
        put(d1, f1);
      }
    };
    for (uint32_t b0 = b_first; b0 < tl.nblk; b0 += 64) {
      const uint32_t bl = b0 + lane;
      const bool valid = bl < tl.nblk;
      // the block's last doc, its directory record (which also holds the preceding block's last
      // doc) and, POS, its first position number in ONE round trip: the kernels are chains of
      // dependent loads — fetching the record only for the blocks that turn out to be wanted made
      // them one longer
      const uint32_t lst = valid ? wave::gload_u32(last_at, bl * 4u) : 0xFFFFFFFFu;
      BlkDir d{};
      uint32_t pos_l = 0;
      if (valid) {
        uint32_t w[4];
        wave::gload_u32x4(dir_at, bl * uint32_t(sizeof(BlkDir)), w);
        d = BlkDir{w[0], w[1], w[2], w[3]};
        if constexpr (POS) pos_l = wave::gload_u32(pos_at, bl * 4u);
      }
      // the block holds docs in (prv, lst], prv = the preceding block's lst
      const uint32_t prv = bl ? d.prev_last : 0u;
      const bool reach = valid && prv < dhi && lst >= dlo;
      // some doc still alive lies in a bucket touching (prv, lst]
      bool want = false;
      if (reach) {
        const uint32_t x0 = prv + 1u > dlo ? prv + 1u - dlo : 0u;
        const uint32_t x1 = (lst < dhi ? lst : dhi) - dlo;
        want = alive_below(alive, apre, (x1 >> s) + 1u) > alive_below(alive, apre, x0 >> s);
      }
      uint64_t mask = wave::ballot(want);
      const bool more = wave::ballot(valid && prv >= dhi) == 0;  // no block started behind dhi yet
      while (mask) {
        const uint32_t k = uint32_t(__builtin_ctzll(mask));
        mask &= mask - 1;
        const uint32_t kbits = wave::read_lane(d.bits, k);
        if (counting) bytes += block_bytes(kbits);
        // two wanted blocks at a time where both live in the packed image: their payload
        // loads are in flight together (one round trip for the pair)
        if (PAIR && mask && pk_both(kbits & 0xFFu, kbits >> 8)) {
          const uint32_t k2 = uint32_t(__builtin_ctzll(mask));
          const uint32_t kbits2 = wave::read_lane(d.bits, k2);
          if (pk_both(kbits2 & 0xFFu, kbits2 >> 8)) {
            mask &= mask - 1;
            if (counting) bytes += block_bytes(kbits2);
            const uint64_t pl1 = pk_at + (uint64_t(wave::read_lane(d.aoff, k)) << 4);
            const uint64_t pl2 = pk_at + (uint64_t(wave::read_lane(d.aoff, k2)) << 4);
            uint64_t da1, db1, fa1, fb1, da2, db2, fa2, fb2;
            raw_load_packed_g<LAYOUT>(pl1, kbits & 0xFFu, lane, da1, db1);
            raw_load_packed_g<LAYOUT>(pl1 + 16u * (kbits & 0xFFu), kbits >> 8, lane, fa1, fb1);
            raw_load_packed_g<LAYOUT>(pl2, kbits2 & 0xFFu, lane, da2, db2);
            raw_load_packed_g<LAYOUT>(pl2 + 16u * (kbits2 & 0xFFu), kbits2 >> 8, lane, fa2, fb2);
            put_packed(da1, db1, fa1, fb1, kbits, wave::read_lane(d.prev_last, k));
            put_packed(da2, db2, fa2, fb2, kbits2, wave::read_lane(d.prev_last, k2));
            continue;
          }
        }
        uint32_t d0, d1, f0, f1;
        if constexpr (POS) {
          // (the branch is taken here, not inside decode_dir_block_pos: a lane broadcast cannot sink
          // into a branch, and only one of `aoff` / `off` is needed)
          const uint32_t base = wave::read_lane(d.prev_last, k);
          const uint32_t dbits = kbits & 0xFFu, fbits = kbits >> 8;
          uint32_t before;
          if (pk_both(dbits, fbits)) {
            decode_packed_pos<LAYOUT>(seg.pk + (uint64_t(wave::read_lane(d.aoff, k)) << 4), dbits, fbits,
                                      base, lane, d0, d1, f0, f1, before);
          } else {
            decode_block_pos<LAYOUT>(seg.doc + tl.doc_start + wave::read_lane(d.off, k), dbits, fbits,
                                     base, lane, d0, d1, f0, f1, before);
          }
          const uint32_t p0 = wave::read_lane(pos_l, k) - pos0 + before;
          put(d0, f0, p0);
          put(d1, f1, p0 + f0);
        } else {
          decode_dir_block<LAYOUT>(seg, tl.doc_start, kbits, wave::read_lane(d.off, k),
                                   wave::read_lane(d.aoff, k), wave::read_lane(d.prev_last, k),
                                   lane, d0, d1, f0, f1);
          put(d0, f0);
          put(d1, f1);
        }
      }
      if (!more) break;
    }
  }
  if (tl.n && tl.first_doc <= dhi && tl.last_doc >= dlo) {  // vint tail / single doc
    if constexpr (POS) {
      const uint32_t base = seg.blk_pos[tl.dir_off + tl.nblk] - seg.blk_pos[tl.dir_off];
      uint32_t d[2], f[2], p[2];
      tail_pidx(seg, tl.tail_row, tl.n, base, lane, d, f, p);
      put(d[0], f[0], p[0]);
      put(d[1], f[1], p[1]);
    } else {
      const uint32_t t0 = lane < tl.n ? seg.tail_docs[tl.tail_row + lane] : 0u;
      const uint32_t t1 = lane + 64u < tl.n ? seg.tail_docs[tl.tail_row + lane + 64u] : 0u;
      const uint32_t g0 = lane < tl.n ? seg.tail_freqs[tl.tail_row + lane] : 0u;
      const uint32_t g1 = lane + 64u < tl.n ? seg.tail_freqs[tl.tail_row + lane + 64u] : 0u;
      put(t0, g0);
      put(t1, g1);
    }
  }
}

// ------------------------------------------------------------ candidates --

// One pass of a wavefront's matches into the unit's candidate list: one reservation per wavefront
// for all its candidates of the pass (lanes with `cand`), key = make_key(score, doc)
__device__ __forceinline__ void emit_candidates(const ConjArgs& A, uint32_t unit, bool cand, float score,
                                                uint32_t doc, unsigned lane) {
  const uint64_t cm = wave::ballot(cand);
  if (cm) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&A.cand_count[unit], uint32_t(__builtin_popcountll(cm)));
    base = wave::read_lane(base, 0);
    const uint32_t slot = base + uint32_t(__builtin_popcountll(cm & ((1ull << lane) - 1ull)));
    if (cand && slot < A.cand_cap) A.cands[uint64_t(unit) * A.cand_cap + slot] = make_key(score, doc);
  }
}

}  // namespace irs_hip
