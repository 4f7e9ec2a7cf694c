// score_docs.h — doc_iterator::seek(target) + score for docs the CALLER names
// (irs_hip_batch_score_docs): for every doc of a unit's list, does the unit's filter match it, and
// with what score (formats_10.cpp:2304-2365; conjunction.hpp:207-223: a conjunction seeks its other
// children to the lead's doc).  What a GPU-backed query needs to sit under a host conjunction, and
// what scores the candidates of another retriever.
//
//   k_score_docs  one wavefront per CHUNK: at most 128 consecutive docs of one unit's list
//                 (score_docs_shape.h).  The caller's docs are a lead item that needs no decoding:
//                 the lead frame, the bucket table, the alive bitmap and the follower walk are
//                 lead.h's, EVERY row of the unit is a follower.
//
// Per chunk:
//   1. the docs to LDS (entries lane, lane + 64); one ballot verifies that they ascend strictly —
//      a chunk that does not is reported unmatched as a whole; a doc of 0 or above the segment's
//      num_docs stays in the frame (ascending docs: such docs sit at its ends) but is never alive:
//      no mask word, no norm and no output but its own zero is indexed by it.  Alive = in range
//      and not masked (DevQuery::dead: deleted docs, excluded terms, the doc set); the alive
//      bitmap holds every alive doc for every row
//   2. lane r searches row r's block directory for the first block that reaches the chunk's first
//      doc (k_conj_seek's search, side by side)
//   3. row after row, follow_list from that block on: a posting on a lead doc sets bit r of the
//      entry's PRESENCE word and leaves score_value(row, tf, norm(doc)) in the entry's slot of row
//      r — a list holds a doc once and the rows run one after the other: plain LDS stores
//   4. a lane's two entries are evaluated from the presence word and the rows' scores, by
//      query_run(op): the flat count against query_need with the unit's merge; a conjunction's
//      groups (a flat one: every row a group); the clauses whose need-mask the word covers; the
//      tree's scoring mask.  float32 sums in row order — entry order for disjunctions, cost order
//      for conjunctions, which is the order the unit's run sums in; clause and tree units sum
//      64-bit fixed point there and float32 here, a difference far inside 1e-5
//   5. scores and matched bytes out, entries lane and lane + 64: coalesced
// Nothing is pruned: no threshold, no block-max bounds, no k.
#pragma once
#include "conj.h"
#include "lead.h"
#include "score_docs_shape.h"
#include "tree.h"

namespace irs_hip {

constexpr uint32_t kSdWaves = 4;   // wavefronts (= chunks) per workgroup
static_assert(kScoreDocsChunk == kBlock, "a chunk is a lead item: a lane's two docs");

// One unit as k_score_docs reads it (plan_score_docs.h builds them from the batch's query records)
struct SdUnit {
  const uint32_t* dead;   // DevQuery::dead
  uint32_t seg;
  uint32_t first;         // its rows: SdArgs::rows[first .. first + n_rows)
  int32_t op;             // DevQuery::op
  uint32_t n_rows;        // 0: the unit matches nothing
  uint32_t opens;         // kRunConj: bit r set = row r opens a group (a flat And: every row)
  uint32_t nodes;         // kRunTree: its first record in SdArgs::nodes (query_need(op) of them)
};
static_assert(sizeof(SdUnit) == 32, "SdUnit: 32 bytes");

struct SdArgs {
  const DevSegment* segs;
  const SdUnit* units;
  const DevQTerm* rows;
  const TreeNode* nodes;
  const ScoreDocsChunk* chunks;   // the host form's records; null: the device form (offsets)
  const uint64_t* offsets;        // [n_units + 1], the device form
  const uint32_t* docs;
  float* scores;
  uint8_t* matched;               // null: not asked for
  uint32_t n_units;
  uint32_t n_chunks;              // records (host form) / slots (device form): wavefronts with work
  uint32_t n_docs;
};

struct SdWave {
  uint32_t docs[kBlock];
  float score[kMaxTerms][kBlock];     // row r's score of the entry (where bit r of pres is set)
  uint32_t norm[kBlock];              // norm_value of the entry's doc
  alignas(16) uint8_t first[kConjBuckets];   // bucket -> 1 + entry index of its first lead doc
  uint32_t bm[kConjWords + 4];        // alive docs' buckets over [dlo, dhi]
  uint8_t apre[kConjWords + 4];       // bits of bm in the words before word w
  uint16_t pres[kBlock];              // bit r: row r holds the entry's doc
  uint32_t info[kMaxTerms];           // DevQTerm::pad0 of row r: clause need-mask / tree leaf
  TreeNode nodes[kTreeMaxNodes];
};
static_assert(sizeof(SdWave) * kSdWaves <= 48u * 1024u, "three workgroups share a CU's 160 KB of LDS");

// tree_shape.h tree_eval on the wavefront's copy of the node table
__device__ __forceinline__ uint32_t sd_tree_mask(const TreeNode* node, uint32_t n_nodes, uint32_t present) {
  uint32_t sat = 0;
  for (uint32_t i = 0; i < n_nodes; ++i) {   // (uniform)
    const TreeNode nd = node[i];
    const uint32_t cnt = uint32_t(__builtin_popcount(present & nd.pos_leaves)) +
                         uint32_t(__builtin_popcount(sat & nd.pos_nodes));
    const bool ok = cnt >= nd.min_match && !(present & nd.neg_leaves) && !(sat & nd.neg_nodes);
    sat |= (ok ? 1u : 0u) << i;
  }
  if (n_nodes == 0 || !((sat >> (n_nodes - 1u)) & 1u)) return 0u;
  uint32_t active = 1u << (n_nodes - 1u), score = 0;
  for (uint32_t i = n_nodes; i-- > 0u;) {
    if (!((active >> i) & 1u)) continue;
    score |= present & node[i].pos_leaves;
    active |= sat & node[i].pos_nodes;
  }
  return score;
}

// Step 4 for one entry: `p` = its presence word (0 for a doc that is not alive)
__device__ __forceinline__ bool sd_evaluate(const SdUnit& U, const SdWave& W, uint32_t e, uint32_t p, float* out) {
  const uint32_t m = U.n_rows, run = query_run(U.op), mrg = query_merge(U.op), need = query_need(U.op);
  float v = 0.f;
  bool hit = false;
  if (p == 0u) {
  } else if (run == kRunTiles || run == kRunCount) {
    const uint32_t c = uint32_t(__builtin_popcount(p));
    hit = run == kRunTiles || c >= need;
    if (hit) {
      bool first = true;
      for (uint32_t r = 0; r < m; ++r) {
        if (!((p >> r) & 1u)) continue;
        v = merge_scores(mrg, first, v, W.score[r][e]);
        first = false;
      }
      if (query_min_both(U.op) && c < 2u) v = 0.f;
    }
  } else if (run == kRunConj) {
    const uint32_t opens = U.opens | 1u;
    hit = true;
    for (uint32_t lo = 0; lo < m && hit;) {
      const uint32_t end = group_end(opens, lo, m);
      float g = 0.f;
      bool any = false;
      for (uint32_t r = lo; r < end; ++r) {
        if (!((p >> r) & 1u)) continue;
        g += W.score[r][e];
        any = true;
      }
      hit = any;
      v = merge_scores(mrg, lo == 0u, v, g);
      lo = end;
    }
    if (!hit) v = 0.f;
  } else if (run == kRunClause) {
    uint32_t covered = 0;
    for (uint32_t r = 0; r < m; ++r) {   // (the row that is its mask's lowest bit opens the clause)
      const uint32_t mk = W.info[r] & 0xFFFFu;
      if (mk && (mk & (0u - mk)) == (1u << r) && (p & mk) == mk) ++covered;
    }
    hit = covered >= need;
    for (uint32_t r = 0; r < m && hit; ++r) {
      const uint32_t mk = W.info[r] & 0xFFFFu;
      if (((p >> r) & 1u) && (p & mk) == mk) v += W.score[r][e];
    }
  } else if (run == kRunTree) {
    uint32_t present = 0;
    for (uint32_t r = 0; r < m; ++r)
      if ((p >> r) & 1u) present |= 1u << (W.info[r] & 15u);
    const uint32_t sm = sd_tree_mask(W.nodes, need, present);
    hit = sm != 0u;
    for (uint32_t r = 0; r < m && hit; ++r) {
      const uint32_t in = W.info[r];
      if (((p >> r) & 1u) && !(in & kTreeNegated) && ((sm >> (in & 15u)) & 1u)) v += W.score[r][e];
    }
  }
  *out = v;
  return hit;
}

template<int LAYOUT>
__device__ __forceinline__ void score_docs_chunk(const SdArgs& A, SdWave* s_wave) {
  const unsigned lane = threadIdx.x & 63u;
  const uint32_t wv = wave::uniform(threadIdx.x >> 6);
  const uint32_t w = blockIdx.x * kSdWaves + wv;
  if (w >= A.n_chunks) return;
  uint32_t unit, first, n;
  if (A.chunks) {
    const ScoreDocsChunk c = wave::sload<ScoreDocsChunk>(reinterpret_cast<uint64_t>(A.chunks) + uint64_t(w) * sizeof(ScoreDocsChunk));
    unit = c.unit;
    first = c.first;
    n = c.n;
  } else {
    // the last unit whose first slot is <= w (score_docs_shape.h); the caller's offsets are not
    // verified: whatever they hold, only docs[0, n_docs) is read and only their outputs written
    if (A.n_units == 0u) return;   // (offsets[lo + 1] below: there is a unit)
    uint32_t lo = 0, hi = A.n_units;
    while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;
      if (score_docs_slot(A.offsets[mid], mid) <= w) lo = mid; else hi = mid;
    }
    const uint64_t a = wave::uniform64(A.offsets[lo]), b = wave::uniform64(A.offsets[lo + 1u]);
    if (a > b || b > A.n_docs) return;
    const uint64_t s0 = score_docs_slot(a, lo);
    if (s0 > w) return;
    const uint64_t at = a + (uint64_t(w) - s0) * kScoreDocsChunk;
    if (at >= b) return;   // a slot none of the unit's chunks takes
    unit = lo;
    first = uint32_t(at);
    n = b - at < kScoreDocsChunk ? uint32_t(b - at) : kScoreDocsChunk;
  }
  if (unit >= A.n_units || n == 0u || n > kScoreDocsChunk) return;
  const SdUnit U = wave::sload<SdUnit>(reinterpret_cast<uint64_t>(A.units) + uint64_t(unit) * sizeof(SdUnit));
  const DevSegment& seg = A.segs[U.seg];
  const uint32_t m = U.n_rows;
  SdWave& W = s_wave[wv];
  uint32_t* docs = W.docs;

  // ---- 1. the chunk's docs: entries lane and lane + 64
  uint32_t ld_d[2], ld_e[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    ld_e[h] = lane + 64u * uint32_t(h);
    ld_d[h] = ld_e[h] < n ? A.docs[first + ld_e[h]] : 0xFFFFFFFFu;
    docs[ld_e[h]] = ld_d[h];
    W.pres[ld_e[h]] = 0;
  }
  lead_first_clear(W.first, lane);
  wave::sync();
  bool bad = false;
  bool alive[2];
  const uint32_t num_docs = seg.num_docs;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t e = ld_e[h], d = ld_d[h];
    if (e < n && e > 0u && docs[e - 1u] >= d) bad = true;
    const bool in_range = e < n && d >= kDocMin && d <= num_docs;
    alive[h] = in_range && !(U.dead && doc_dead(U.dead, d));
    // (a doc outside the norm column is in no posting list: its value is never used)
    const bool has_norm = in_range && seg.norms && d >= seg.norm_min_doc && uint64_t(d - seg.norm_min_doc) < seg.norm_count;
    W.norm[e] = has_norm ? norm_value(seg, d) : 1u;
  }
  const bool ordered = wave::ballot(bad) == 0;
  const bool any_alive = wave::ballot(alive[0] || alive[1]) != 0;
  auto store = [&](int h, float v, bool hit) {
    if (ld_e[h] < n) {
      A.scores[first + ld_e[h]] = v;
      if (A.matched) A.matched[first + ld_e[h]] = hit ? 1 : 0;
    }
  };
  if (!ordered || !any_alive || m == 0u || m > kMaxTerms) {   // (wave-uniform) nothing of the chunk can match
    store(0, 0.f, false);
    store(1, 0.f, false);
    return;
  }
  const LeadFrame fr = lead_frame(docs, n);
  lead_first_fill(fr, W.first, docs, ld_d, ld_e, n);
  alive_rebuild(fr, W.bm, W.apre, ld_d, alive, lane);

  // ---- 2. every row's first block that reaches the chunk's first doc; the unit's tables
  const uint64_t rows_at = reinterpret_cast<uint64_t>(A.rows) + uint64_t(U.first) * sizeof(DevQTerm);
  uint32_t start = 0;
  if (lane < m) {
    const DevQTerm qt = A.rows[U.first + lane];
    W.info[lane] = qt.pad0;
    if (qt.term != kNoTerm) {
      const DevTerm t = seg.terms[qt.term];
      const uint32_t* last = seg.blk_last + t.dir_off;
      uint32_t a = 0, b = t.nblk;   // lower_bound(last, dlo)
      while (a < b) {
        const uint32_t mid = (a + b) >> 1;
        if (last[mid] < fr.dlo) a = mid + 1; else b = mid;
      }
      start = a;
    }
  }
  if (query_run(U.op) == kRunTree) {
    const uint32_t n_nodes = query_need(U.op) < kTreeMaxNodes ? query_need(U.op) : kTreeMaxNodes;
    if (lane < 4u * n_nodes)
      reinterpret_cast<uint32_t*>(W.nodes)[lane] = reinterpret_cast<const uint32_t*>(A.nodes + U.nodes)[lane];
  }
  wave::sync();

  // ---- 3. the rows, one after the other
  uint32_t bytes = 0;
  for (uint32_t r = 0; r < m; ++r) {   // (uniform)
    const DevQTerm qt = wave::sload<DevQTerm>(rows_at + r * sizeof(DevQTerm));
    if (qt.term == kNoTerm) continue;
    const DevTerm t = wave::sload<DevTerm>(reinterpret_cast<uint64_t>(seg.terms) + uint64_t(qt.term) * sizeof(DevTerm));
    DevTail tl;   // (what k_plan writes per (unit, term slot))
    tl.n = t.docs_count == 1u ? 1u : t.tail_n;
    tl.first_doc = tl.n ? seg.tail_docs[t.tail_row] : 0u;
    tl.last_doc = tl.n ? t.last_doc : 0u;
    tl.nblk = t.nblk;
    tl.doc_start = t.doc_start;
    tl.dir_off = t.dir_off;
    tl.term = qt.term;
    tl.tail_row = t.tail_row;
    const uint16_t bit = uint16_t(1u << r);
    float* row = W.score[r];
    auto put = [&](uint32_t doc, uint32_t f) {
      const uint32_t x = doc - fr.dlo;
      if (f == 0u || x > fr.span) return;
      const uint32_t i = lead_index(W.first, docs, n, x >> fr.s, fr.s, doc);
      if (i == n) return;
      W.pres[i] = uint16_t(W.pres[i] | bit);
      row[i] = score_value(qt, f, W.norm[i]);
    };
    follow_list<LAYOUT, false, true>(seg, tl, wave::read_lane(start, r), fr, W.bm, W.apre, false, bytes, lane, put);
    wave::sync();
  }

  // ---- 4., 5. a lane's two entries
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t e = ld_e[h] < n ? ld_e[h] : 0u;
    float v = 0.f;
    const bool hit = sd_evaluate(U, W, e, alive[h] ? uint32_t(W.pres[e]) : 0u, &v);
    store(h, v, hit);
  }
}

// 4 wavefronts x ~10.8 KB (16 score rows of 128 docs each): three workgroups per CU, 3 wavefronts
// per SIMD (LDS bound), as k_conj_any
template<int LAYOUT>
__global__ void __launch_bounds__(kSdWaves * 64)
k_score_docs(SdArgs A) {
  __shared__ SdWave s_wave[kSdWaves];
  score_docs_chunk<LAYOUT>(A, s_wave);
}

}  // namespace irs_hip
