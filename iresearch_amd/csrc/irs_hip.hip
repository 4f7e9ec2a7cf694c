// irs_hip.hip — host side of the C ABI declared in include/irs_hip.h:
// staging into HBM, kernel orchestration on a HIP stream, result hand-back.
// Nothing here touches oracle/; there is no CPU execution path.
#include "irs_hip.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <tuple>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "gpu_rt.h"
#include "kernels.h"
#include "phrase.h"
#include "vphrase.h"
#include "phrases.h"
#include "phrases_or.h"
#include "score.h"
#include "conj.h"
#include "conj_any.h"
#include "join.h"
#include "wide.h"
#include "clauses.h"
#include "clause_shape.h"
#include "tree.h"
#include "excl.h"
#include "match.h"
#include "score_docs.h"
#include "nested.h"

using namespace irs_hip;

#include "pool.h"
#include "stream_cache.h"
#include "segment.h"
#include "batch.h"
#include "plan_tiles.h"
#include "plan_blocks.h"
#include "plan_any.h"
#include "plan_wide.h"
#include "plan_clauses.h"
#include "plan_tree.h"
#include "plan_join.h"
#include "plan_match.h"
#include "plan_score_docs.h"
#include "plan_nested.h"
#include "units.h"

namespace {

// `all`, in order: the units of `joining` (a subsequence) to join.units, the others to `rest`
void deal(irs_hip_batch* b, const std::vector<uint32_t>& all, const std::vector<uint32_t>& joining,
          std::vector<uint32_t>& rest) {
  size_t at = 0;
  for (uint32_t u : all) {
    const bool joins = at < joining.size() && joining[at] == u;
    (joins ? b->join.units : rest).push_back(u);
    at += joins;
  }
}

// Doc-tile units to joined streams (join.units) or work items (tiles.units); conjunctions to joined
// streams or block-driven work (blocks.units).
void deal_units(irs_hip_batch* b) {
  // doc-tile units: plain disjunctions run as joined posting streams (join.h), the others as
  // work items (score.h)
  const bool allow = join_allowed(b);
  b->tiles.units.clear();
  b->join.units.clear();
  b->tiles.any_and = false;
  {
    std::vector<uint32_t> can;
    for (uint32_t u : b->all_tile_units)
      if (allow && unit_joinable(b, u)) can.push_back(u);
    const int forced = join_or_forced(b);
    if (forced == 0 || (forced < 0 && !join_or_pays(b, can))) can.clear();
    deal(b, b->all_tile_units, can, b->tiles.units);
    for (uint32_t u : b->tiles.units) b->tiles.any_and = b->tiles.any_and || unit_counts_matches(b->queries[u]);
  }
  if (!b->phrase) {   // (a phrase batch's blocks.units are its phrases, fixed at create)
    // a conjunction whose rarest term is far rarer than the rest is cheaper block driven
    // (conj.h decodes only the blocks the lead term's docs fall into): join_and_saving
    b->blocks.units.clear();
    const int forced = join_and_forced(b);
    std::vector<uint32_t> joining;
    int64_t saved = 0;
    for (uint32_t u : b->all_conj_units) {
      const int64_t s = (allow && forced != 0 && unit_joinable(b, u))
                            ? (forced == 1 ? 1 : join_and_saving(b, b->queries[u])) : 0;
      if (s > 0) {
        joining.push_back(u);
        saved += s;
      }
    }
    // (a batch that joins plain disjunctions anyway has paid for k_join and the pilot: one more
    // k_join_score launch is all a joined conjunction adds)
    if (forced != 1 && saved < (b->join.units.empty() ? kJoinAndLaunchCost : kJoinAndLaunchCost / 10))
      joining.clear();
    deal(b, b->all_conj_units, joining, b->blocks.units);
  }
}

// The geometry of the deal: the tile, every unit's tiles and slices of the plan tables, k_score's
// queue order, the pilot stride, the workgroup sizes.  first_words: the plan table's words;
// item_bound: an upper bound of the work items.  false: the batch is too large.
bool size_units(irs_hip_batch* b, uint64_t* first_words, uint64_t* item_bound) {
  // 32-bit accumulators halve the LDS per doc: twice the tile at the same residency
  // the largest tile that still lets two workgroups share a CU's 160 KB of LDS
  // (AND / min-match batches also keep a match counter byte per doc)
  // (chosen anew on every deal: set_path / set_wand re-deal the units, and `any_and` with them)
  if (b->tiles.asked) b->tiles.docs = b->tiles.asked;
  else if (!b->phrase) b->tiles.docs = b->acc32 ? (b->tiles.any_and ? 8192 : 12288) : 6144;
  // per unit: tiles of its segment, its slice of the plan table and of the per-tile tables;
  // upper bound of its work items: every block once + one more per tile border it may
  // straddle + the decoded tail
  uint64_t tiles = 0;
  *first_words = 0;
  *item_bound = kItemSlack;
  b->n_tiles = 0xFFFFFFFFu;
  b->tiles.n_max = 0;
  b->join.n_max = 0;
  b->wide.n_max = 0;
  b->wide.n_min = 0xFFFFFFFFu;
  b->clause.n_max = 0;
  b->clause.n_min = 0xFFFFFFFFu;
  b->tree.n_max = 0;
  b->tree.n_min = 0xFFFFFFFFu;
  std::vector<uint8_t> is_join(b->nq, 0);
  for (uint32_t u : b->join.units) is_join[u] = 1;
  for (uint32_t u = 0; u < b->nq; ++u) {
    DevQuery& dq = b->queries[u];
    if (unit_is_wide(dq)) {   // (tiles of its own: nothing of the other units' geometry counts it)
      size_wide_unit(b, dq);
      continue;
    }
    if (unit_is_clause(dq)) {   // (likewise)
      size_clause_unit(b, dq);
      continue;
    }
    if (unit_is_tree(dq)) {   // (likewise)
      size_tree_unit(b, dq);
      continue;
    }
    // (conjunctions are block driven unless they run as joined streams)
    const bool tiled = !b->phrase && (query_run(dq.op) != kRunConj || is_join[u]);
    const uint32_t tile_docs = is_join[u] ? kJoinTile : b->tiles.docs;   // (streams are cut at kJoinTile)
    dq.n_tiles = tiled ? (b->segs[dq.seg]->dev.num_docs + tile_docs - 1) / tile_docs : 0u;
    if (b->phrase) dq.n_tiles = 1;
    if (tiled) b->n_tiles = std::min(b->n_tiles, dq.n_tiles);
    if (is_join[u]) {   // no plan table, no work items (k_plan / k_items_* skip the unit)
      dq.first_off = kNoPlan;
      dq.tile_base = 0;
      b->join.n_max = std::max(b->join.n_max, dq.n_tiles);
      continue;
    }
    dq.first_off = *first_words;
    *first_words += uint64_t(dq.n_tiles + 1) * b->jt;
    if (tiles + dq.n_tiles > 0xFFFFFF00ull) return false;
    dq.tile_base = uint32_t(tiles);
    tiles += dq.n_tiles;
    b->tiles.n_max = std::max(b->tiles.n_max, dq.n_tiles);
    if (tiled) {
      for (uint32_t j = 0; j < dq.n_terms; ++j)
        *item_bound += uint64_t(b->segs[dq.seg]->terms[b->qterms[dq.first_term + j].term].nblk) +
                      dq.n_tiles + 1;
    }
  }
  if (*item_bound > 0xFFFFFF00ull) return false;
  b->tiles.n_total = uint32_t(tiles);
  if (b->n_tiles == 0xFFFFFFFFu) b->n_tiles = 0;
  {  // k_score's queue order over the tiled units: heaviest first within every chunk round
    std::vector<std::pair<uint64_t, uint32_t>> work;
    for (uint32_t u : b->tiles.units) {
      const DevQuery& dq = b->queries[u];
      uint64_t w = 0;
      for (uint32_t j = 0; j < dq.n_terms; ++j)
        w += b->segs[dq.seg]->terms[b->qterms[dq.first_term + j].term].docs_count;
      work.push_back({w, u});
    }
    // ... segment by segment: the workgroups resident at one time should keep reading the same
    // doc range (shared in L2), so units of one segment stay together
    std::stable_sort(work.begin(), work.end(), [&](const auto& x, const auto& y) {
      const uint32_t sx = b->queries[x.second].seg, sy = b->queries[y.second].seg;
      return sx != sy ? sx < sy : x.first > y.first;
    });
    for (uint32_t i = 0; i < work.size(); ++i) b->queries[i].run_unit = work[i].second;
  }
  b->stride_eff = (b->tiles.units.empty() && b->join.units.empty())
                      ? b->stride
                      : std::max<uint32_t>(1, std::min<uint32_t>(b->stride, b->n_tiles / 2));
  // k_pilot / k_score stage TILE norm bytes per tile, NormStage<TILE>::kPieces x 8 per thread
  {
    const uint32_t pieces = (b->tiles.docs + 4095u) / 4096u;
    uint32_t need = b->phrase ? 0u : (b->tiles.docs + 8u * pieces - 1u) / (8u * pieces);
    b->tiles.threads = b->knobs.wg_threads;
    while (b->tiles.threads < need) b->tiles.threads *= 2;
    b->tiles.nw_log2 = 0;
    while ((64u << b->tiles.nw_log2) < b->tiles.threads) ++b->tiles.nw_log2;
  }
  b->join.threads = b->knobs.join_threads;
  b->join.nw_log2 = 0;
  while ((64u << b->join.nw_log2) < b->join.threads) ++b->join.nw_log2;
  if (b->cand_cap == 0) b->cand_cap = default_cand_cap(b);
  return true;
}

// The buffers of the deal, its streams and groups, and its tables staged for the next run
bool alloc_scratch(irs_hip_batch* b, uint64_t first_words, uint64_t item_bound) {
  const uint64_t rows = uint64_t(b->nq) * b->jt;
  // what every run starts from zero lives in ONE block (one fill per run instead of six: each is
  // a dispatch of its own in front of the first kernel): status, thresholds, candidate and hit
  // counters, the touched / pruned tallies
  {
    const uint64_t nq = b->nq;
    auto up = [](uint64_t v) { return (v + 255u) & ~uint64_t(255); };
    const uint64_t o_status = 0, o_bstar = 256, o_count = o_bstar + up(nq * 4),
                   o_hits = o_count + up(nq * 4), o_touched = o_hits + up(nq * 8),
                   o_pruned = o_touched + up(nq * 16), total = o_pruned + up(nq * 4);
    if (!b->d_zeroed.alloc(total)) return false;
    uint8_t* z = b->d_zeroed.as<uint8_t>();
    b->d_status.view(z + o_status, 4);
    b->d_bstar.view(z + o_bstar, nq * 4);
    b->d_cand_count.view(z + o_count, nq * 4);
    b->d_hits.view(z + o_hits, nq * 8);
    b->d_touched.view(z + o_touched, nq * 16);
    b->d_pruned.view(z + o_pruned, nq * 4);
  }
  if (!b->d_first.alloc(std::max<uint64_t>(first_words, 1) * sizeof(uint32_t)) ||
      !b->d_tails.alloc(rows * sizeof(DevTail)) ||
      !b->d_cands.alloc(uint64_t(b->nq) * b->cand_cap * sizeof(uint64_t)) ||
      !b->d_out.alloc(uint64_t(b->nq) * b->k_max * sizeof(Hit)) ||
      !b->d_out_count.alloc(b->nq * sizeof(uint32_t)) || !b->tiles.d_work.alloc(16))
    return false;
  if (streams_on(b) && !build_streams(b)) return false;
  if (!alloc_wide(b) || !alloc_clauses(b) || !alloc_tree(b) || !build_groups(b)) return false;
  if (!b->tiles.units.empty()) {
    if (!b->tiles.d_units.alloc(b->tiles.units.size() * 4) ||
        !b->up.copy(b->tiles.d_units.p, b->tiles.units.data(), b->tiles.units.size() * 4))
      return false;
  }
  if (!b->phrase && !b->tiles.units.empty()) {
    const uint64_t tiles = b->tiles.n_total;
    const uint64_t parts = (tiles + 1 + kScanChunk - 1) / kScanChunk;
    if (!b->tiles.d_off.alloc((tiles + 1) * sizeof(uint32_t)) ||
        !b->tiles.d_scan_parts.alloc((parts + 1) * sizeof(uint64_t)) ||
        !b->tiles.d_items.alloc(item_bound * sizeof(ItemG)) ||
        !b->tiles.d_args.alloc(sizeof(ScoreArgs)) ||
        !b->tiles.d_ub.alloc((tiles + 1) * sizeof(float)) ||
        (b->excl.sets_on() && !b->excl.d_tile_live.alloc(tiles + 1)))
      return false;
  }
  // (the unit records last: dealing the units and building the streams filled fields in)
  return b->up.copy(b->d_queries.p, b->queries.data(), b->queries.size() * sizeof(DevQuery));
}

// The distinct doc masks of the batch, from what create recorded per unit (its present excluded
// terms) and the doc sets in force: one per (segment, doc-set row, terms), every unit that has one
// pointing at it, the others at their segment's deleted docs.  The words are one pool block.  At
// create, and whenever irs_hip_batch_set_doc_sets changes the rows (the batch is quiet then: the
// tables are replaced).
int build_masks(irs_hip_batch* b) {
  ExclWork& x = b->excl;
  // (tables staged for an upload that never went out: their buffers may change below)
  b->up.pending.erase(std::remove_if(b->up.pending.begin(), b->up.pending.end(), [&](const Stager::Piece& p) {
    return p.dst == x.d_masks.p || p.dst == x.d_terms.p || p.dst == x.d_restricted.p;
  }), b->up.pending.end());
  x.masks.clear();
  x.terms.clear();
  x.restricted.assign(b->nq, 0);
  x.set_bytes = 0;
  std::map<std::tuple<uint32_t, uint32_t, std::vector<uint32_t>>, uint32_t> mask_ids;
  std::vector<uint32_t> mask_of(b->nq, 0);   // [unit] mask + 1, 0: none
  std::vector<uint32_t> terms;
  for (uint32_t q = 0; q < b->nq; ++q) {
    const uint32_t s = q / b->nq_user;
    const irs_hip_segment* seg = b->segs[s];
    b->queries[q].dead = seg->dev.dead;
    const uint32_t row = x.sets_on() ? x.row_of[q] : IRS_HIP_NO_DOC_SET;
    if (row != IRS_HIP_NO_DOC_SET) x.set_bytes += (uint64_t(seg->dev.num_docs) + 7u) / 8u;
    terms.assign(x.unit_terms.begin() + x.unit_first[q], x.unit_terms.begin() + x.unit_first[q + 1]);
    if (!x.unit_live[q] || (terms.empty() && row == IRS_HIP_NO_DOC_SET)) continue;
    auto ins = mask_ids.emplace(std::make_tuple(s, row, terms), uint32_t(x.masks.size()));
    if (ins.second) {
      ExclMask m{};
      m.seg = s;
      m.first = uint32_t(x.terms.size());
      m.n = uint32_t(terms.size());
      m.words = dead_words(seg->dev.num_docs);
      m.dead = seg->dev.dead;
      m.num_docs = seg->dev.num_docs;
      if (row != IRS_HIP_NO_DOC_SET) {
        m.set = x.sets + uint64_t(row) * x.set_words;
        m.set_words = x.set_words;
      }
      x.masks.push_back(m);
      x.terms.insert(x.terms.end(), terms.begin(), terms.end());
    }
    mask_of[q] = ins.first->second + 1u;
    x.restricted[q] = row != IRS_HIP_NO_DOC_SET;
  }
  if (x.sets_on() && (!x.d_restricted.alloc(b->nq) || !b->up.copy(x.d_restricted.p, x.restricted.data(), b->nq)))
    return IRS_HIP_ENOMEM;
  if (!x.on()) return IRS_HIP_OK;
  uint64_t words = 0, most = 0;
  for (const ExclMask& m : x.masks) {
    words += m.words;
    most = std::max(most, m.words);
  }
  if (!x.d_words.alloc(words * 4) || !x.d_masks.alloc(x.masks.size() * sizeof(ExclMask)) ||
      !x.d_terms.alloc(std::max<size_t>(x.terms.size(), 1) * 4))
    return IRS_HIP_ENOMEM;
  words = 0;
  for (ExclMask& m : x.masks) {
    m.out = x.d_words.as<uint32_t>() + words;
    words += m.words;
  }
  for (uint32_t q = 0; q < b->nq; ++q)
    if (mask_of[q]) b->queries[q].dead = x.masks[mask_of[q] - 1u].out;
  x.slices = uint32_t((most + b->knobs.excl_slice - 1) / b->knobs.excl_slice);
  if (uint64_t(x.slices) * x.masks.size() > 0x7FFFFFFFull) return IRS_HIP_EUNSUPPORTED;
  if (!b->up.copy(x.d_masks.p, x.masks.data(), x.masks.size() * sizeof(ExclMask)) ||
      !b->up.copy(x.d_terms.p, x.terms.data(), x.terms.size() * 4))
    return IRS_HIP_ENOMEM;
  return IRS_HIP_OK;
}

// The doc masks of the units with excluded terms (excl.h): every distinct mask in one launch — in the
// plan stage of every run, and ahead of a batch's match sets (plan_match.h)
bool launch_excl_masks(irs_hip_batch* b, rt::stream_t st) {
  const size_t smem = size_t(b->knobs.excl_slice) * 4;
  const uint32_t grid = b->excl.slices * uint32_t(b->excl.masks.size());
  return with_layout(b->seg->dev.layout, [&](auto L) {
    if (!big_smem(k_excl_mask<decltype(L)::value>, smem)) return false;
    RT_LAUNCH((k_excl_mask<decltype(L)::value>), grid, kThreads, smem, st, b->d_segs.as<DevSegment>(),
              b->excl.d_masks.as<ExclMask>(), b->excl.d_terms.as<uint32_t>(), b->excl.slices,
              b->knobs.excl_slice);
    return rt::last_error_ok();
  });
}

bool ensure_scratch(irs_hip_batch* b) {
  if (b->scratch_ready) return true;
  HostTrace trace("ensure_scratch (units dealt, streams, work lists)");
  b->join.args_valid[0] = b->join.args_valid[1] = b->tiles.args_valid = false;
  b->min_dirty = b->has_min;   // (a unit's bin_scale may change below: build_groups)
  if (b->phrase) b->tiles.docs = 0x40000000u;  // k_phrase is block driven: one "tile" = the segment
  deal_units(b);
  if (!b->phrase && build_conj_work(b) != IRS_HIP_OK) return false;
  uint64_t first_words = 0, item_bound = 0;
  if (!size_units(b, &first_words, &item_bound) || !alloc_scratch(b, first_words, item_bound))
    return false;
  b->scratch_ready = true;
  return true;
}

}  // namespace

// Runs one entry point's body; exceptions (std::bad_alloc out of a std::vector, anything
// else) become status codes: the ABI promises that nothing is thrown across it.
template<typename F>
int guarded(F&& f) noexcept {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return IRS_HIP_ENOMEM;
  } catch (...) {
    return IRS_HIP_EHIP;
  }
}

// ---- the host half of a run, off the caller's thread -------------------------------------------
// One worker thread per device (started with the first run).  A caller that serves batches in a
// loop prepares and creates batch i + 1 while the worker deals the units of batch i, builds its
// streams and work lists and queues its uploads and kernels; the GPU meanwhile executes batch
// i - 1.  At one GPU the kernels hide all of it; with 8 ranks a rank's kernels take as long as this
// host work (index-search runs its queries on --threads workers for the same reason:
// index-search.cpp:673-722).  IRS_HIP_ASYNC_RUN=0 runs everything on the caller's thread.
namespace worker {
// A job = the host half of a run, or the recovery of a batch whose threshold spans ranks: both
// issue collectives on the batch's communicator, and RCCL pairs collectives by issue ORDER — so
// everything of a device that may issue one goes through this one FIFO (a re-run of
// batch i on the caller's thread raced the worker's run of batch i + 1 on the same communicator).
struct Job {
  irs_hip_batch* b;
  std::function<int()> fn;
};
struct Queue {
  std::mutex m;
  std::condition_variable cv;
  std::deque<Job> jobs;
  std::thread th;
  bool started = false, stop = false;
  int device = 0;
  ~Queue() {
    {
      std::lock_guard<std::mutex> lock(m);
      stop = true;
    }
    cv.notify_all();
    if (th.joinable()) th.join();
  }
};
static Queue& of(int device) {
  static Queue queues[pool::kMaxDevices];
  return queues[device >= 0 && device < pool::kMaxDevices ? device : 0];
}
static void loop(Queue* q) {
  rt::set_device(q->device);
  for (;;) {
    Job job;
    {
      std::unique_lock<std::mutex> lock(q->m);
      q->cv.wait(lock, [&] { return q->stop || !q->jobs.empty(); });
      if (q->jobs.empty()) return;   // (stop)
      job = q->jobs.front();
      q->jobs.pop_front();
    }
    const int rc = guarded([&] {
      if (!rt::set_device(job.b->seg->device)) return int(IRS_HIP_EHIP);
      return job.fn();
    });
    {
      std::lock_guard<std::mutex> lock(job.b->sync.m);
      job.b->sync.async_rc = rc;
      job.b->sync.async_pending = false;
    }
    job.b->sync.cv.notify_all();
  }
}
static bool enabled() {
  static const bool on = [] {
    const char* e = std::getenv("IRS_HIP_ASYNC_RUN");
    return !e || std::atoi(e) != 0;
  }();
  return on;
}
// Queues `fn` for the batch on its device's worker; false: the worker cannot take it (no thread,
// no memory) — nothing is pending, the caller runs `fn` itself.
static bool submit(irs_hip_batch* b, std::function<int()> fn) {
  Queue& q = of(b->seg->device);
  try {
    std::lock_guard<std::mutex> lock(q.m);
    if (!q.started) {
      q.device = b->seg->device;
      q.th = std::thread(loop, &q);
      q.started = true;
    }
    {
      std::lock_guard<std::mutex> block(b->sync.m);
      b->sync.async_pending = true;
      b->sync.async_rc = IRS_HIP_OK;
    }
    try {
      q.jobs.push_back(Job{b, std::move(fn)});
    } catch (...) {
      std::lock_guard<std::mutex> block(b->sync.m);
      b->sync.async_pending = false;   // (nothing was queued: nobody would ever clear it)
      throw;
    }
    q.cv.notify_one();
    return true;
  } catch (...) {
    return false;
  }
}
static bool wanted(const irs_hip_batch* b) { return b->sync.async_pref < 0 ? enabled() : b->sync.async_pref != 0; }
}  // namespace worker

// Before anything else touches a batch: its run, if one was handed to the worker, is queued.
// Returns what that run returned (once).
static int settle(irs_hip_batch* b) {
  if (!b) return IRS_HIP_OK;
  std::unique_lock<std::mutex> lock(b->sync.m);
  b->sync.cv.wait(lock, [&] { return !b->sync.async_pending; });
  const int rc = b->sync.async_rc;
  b->sync.async_rc = IRS_HIP_OK;
  return rc;
}
// an entry point's body behind the batch's pending run
template<typename F>
static int settled(irs_hip_batch* b, F&& f) noexcept {
  return guarded([&] {
    if (const int rc = settle(b)) return rc;
    return f();
  });
}

extern "C" {

uint32_t irs_hip_abi_version(void) { return IRS_HIP_ABI_VERSION; }

const char* irs_hip_strerror(int status) {
  switch (status) {
    case IRS_HIP_OK: return "ok";
    case IRS_HIP_EINVAL: return "invalid argument";
    case IRS_HIP_ECORRUPT: return "corrupt postings data";
    case IRS_HIP_ENOMEM: return "out of memory";
    case IRS_HIP_EHIP: return "HIP runtime error or no gfx950 device";
    case IRS_HIP_EOVERFLOW: return "candidate buffer overflow";
    case IRS_HIP_EUNSUPPORTED: return "unsupported";
    case IRS_HIP_EPEER: return "another rank could not re-execute its batch";
    default: return "unknown status";
  }
}

void irs_hip_segment_close(irs_hip_segment* seg) {
  if (!seg) return;
  rt::set_device(seg->device);
  scache::drop_unpinned(seg->device, seg->uid);   // (its decoded streams: back to the pool)
  pool::tl_free_now = true;   // (its buffers are freed, not pooled)
  delete seg;
  pool::tl_free_now = false;
}

uint64_t irs_hip_segment_device_bytes(const irs_hip_segment* seg) {
  return seg ? seg->device_bytes : 0;
}
uint64_t irs_hip_segment_live_docs(const irs_hip_segment* seg) { return seg ? seg->live_docs : 0; }

// ----------------------------------------------------------------- batch --

// What create leaves on the device: the segments' records and the units' rows (d_queries goes out
// from ensure_scratch, once the units' tile geometry is in)
static int upload_create_tables(irs_hip_batch* b) {
  if (b->jt == 0) b->jt = 1;
  if (b->qterms.empty()) b->qterms.push_back(DevQTerm{});
  std::vector<DevSegment> dsegs;
  for (irs_hip_segment* sg : b->segs) {
    // (another thread's batch may be adding the lazily built tables to `dev` right now)
    std::lock_guard<std::mutex> lock(sg->wand_mutex);
    dsegs.push_back(sg->dev);
  }
  if (!b->d_queries.alloc(b->queries.size() * sizeof(DevQuery)) ||
      !b->d_qterms.alloc(b->qterms.size() * sizeof(DevQTerm)) ||
      !b->d_segs.alloc(dsegs.size() * sizeof(DevSegment)) ||
      !b->up.copy(b->d_segs.p, dsegs.data(), dsegs.size() * sizeof(DevSegment)) ||
      !b->up.copy(b->d_qterms.p, b->qterms.data(), b->qterms.size() * sizeof(DevQTerm)))
    return IRS_HIP_ENOMEM;
  return IRS_HIP_OK;
}

// A batch under construction: a failed create takes its term pass with it
struct BatchDeleter {
  void operator()(irs_hip_batch* b) const {
    if (b->opt) irs_hip_batch_destroy(b->opt);
    delete b;
  }
};

// The steps of create (units.h; DESIGN.md "From queries to units").  Whatever it throws is a failed
// allocation: IRS_HIP_ENOMEM.  *out stays null on every failure.
static int batch_create_multi_impl(irs_hip_segment* const* segs, uint32_t n_segs,
                               const irs_hip_query* queries, uint32_t nq_user,
                               const irs_hip_term_scorer* all_terms, uint32_t n_entries,
                               irs_hip_batch** out) try {
  if (!segs || !n_segs || !queries || !all_terms || !out || !nq_user) return IRS_HIP_EINVAL;
  HostTrace trace("batch_create (query records)");
  *out = nullptr;
  if (uint64_t(n_segs) * nq_user > 0x7FFFFFFFull) return IRS_HIP_EINVAL;
  for (uint32_t s = 0; s < n_segs; ++s) {
    if (!segs[s]) return IRS_HIP_EINVAL;
    if (!segs[s]->dev.has_freq) return IRS_HIP_EUNSUPPORTED;  // scorers need IndexFeatures::FREQ
    // one launch per kernel covers every segment: same device, same block layout
    if (segs[s]->device != segs[0]->device) return IRS_HIP_EINVAL;
    if (segs[s]->dev.layout != segs[0]->dev.layout) return IRS_HIP_EUNSUPPORTED;
  }
  if (!rt::set_device(segs[0]->device)) return IRS_HIP_EHIP;
  std::unique_ptr<irs_hip_batch, BatchDeleter> owner(new (std::nothrow) irs_hip_batch);
  irs_hip_batch* b = owner.get();
  if (!b) return IRS_HIP_ENOMEM;
  b->seg = segs[0];
  b->knobs = Knobs::from_env();
  const uint32_t nq = n_segs * nq_user;
  b->nq = nq;
  b->nq_user = nq_user;
  b->segs.assign(segs, segs + n_segs);
  b->queries.resize(nq);
  b->count_precise.assign(nq, 0);
  b->groups.upper.assign(nq, 0.0);
  b->blocks.opens.assign(nq, 0);
  b->blocks.n_phrase.assign(nq, 0);
  b->blocks.phrase_opens.assign(nq, 0);
  b->any.opens.assign(nq, 0);
  b->qterms.reserve(size_t(n_entries) * n_segs);
  b->excl.unit_first.assign(1, 0u);
  b->excl.unit_live.assign(nq, 0);
  std::vector<uint32_t> grouped_units;   // units of grouped conjunctions (IRS_HIP_GROUP_ALT)
  UnitScratch scratch;
  for (uint32_t q = 0; q < nq; ++q) {
    // unit q = (segment q / nq_user, query q % nq_user); the segment's own term entries
    const irs_hip_segment* seg = segs[q / nq_user];
    const irs_hip_term_scorer* terms = all_terms + size_t(q / nq_user) * n_entries;
    const irs_hip_query& in = queries[q % nq_user];
    Unit u;
    int rc = unit_shape(in, terms, n_entries, seg, u.shape, scratch.excl, scratch.tab);
    if (rc != IRS_HIP_OK) return rc;
    const irs_hip_term_scorer* ents = terms + in.first_term;
    rc = phrase_only_rule(b, q, u.shape);
    if (rc == IRS_HIP_OK && u.shape.phrase()) rc = phrase_parts_ok(ents, u.shape, seg);
    if (rc == IRS_HIP_OK) rc = unit_rows(ents, seg, u, scratch);
    if (rc == IRS_HIP_OK) rc = phrase_kernel_rule(b, u.shape);
    if (rc == IRS_HIP_OK) rc = unit_need(in, u, scratch);
    if (rc != IRS_HIP_OK) return rc;
    unit_run(in, seg, u, scratch);
    u.n_caches = assign_table_slots(scratch.row);
    if (u.shape.wide() || u.shape.clause || u.shape.tree) rc = wide_terms_ok(seg, scratch.row);
    if (rc == IRS_HIP_OK) rc = unit_scale(u, !scratch.row.empty());
    if (rc != IRS_HIP_OK) return rc;
    commit_unit(b, q, in, seg, u, scratch, grouped_units);
  }
  if (b->knobs.acc64) b->acc32 = false;   // tuning / test knob
  if (const int rc = build_masks(b)) return rc;
  widen_fixed_point(b);
  if (b->phrase) {
    if (const int rc = build_phrase_work(b)) return rc;
    if (b->blocks.optional)
      if (const int rc = create_term_pass(b, segs, n_segs, queries, all_terms, n_entries)) return rc;
  }
  if (!grouped_units.empty())
    if (const int rc = build_any_work(b, grouped_units)) return rc;
  // (the block-driven kernels read the norms of a lead block's docs from the posting-order copy)
  // — a permanent copy per segment, one byte per posting (irs_hip_segment_device_bytes counts
  // it): built the first time a conjunction / phrase whose scorer reads norms arrives
  if (b->phrase || !b->all_conj_units.empty() || !b->any.units.empty()) {
    bool wanted = false;
    for (const DevQTerm& qt : b->qterms) wanted = wanted || needs_norm(qt.kind);
    for (irs_hip_segment* sg : b->segs)
      if (wanted)
        if (const int rc = prepare_posting_norms(sg)) return rc;
  }
  if (const int rc = upload_create_tables(b)) return rc;
  *out = owner.release();
  return IRS_HIP_OK;
} catch (...) {
  return IRS_HIP_ENOMEM;
}

static int batch_configure_impl(irs_hip_batch* b, uint32_t tile_docs, uint32_t pilot_stride,
                            uint32_t cand_cap) {
  if (!b) return IRS_HIP_EINVAL;
  if (tile_docs && tile_docs != 4096 && tile_docs != 6144 && tile_docs != 8192 &&
      tile_docs != 12288)
    return IRS_HIP_EINVAL;
  if (cand_cap && cand_cap < b->k_max) return IRS_HIP_EINVAL;
  if (!quiet_for_setter(b)) return IRS_HIP_EHIP;
  if (!b->phrase) b->tiles.asked = b->tiles.docs = tile_docs;  // phrase tiles are fixed; 0: by the units' needs
  if (pilot_stride) b->stride = pilot_stride;
  b->cand_cap = cand_cap;
  deal_is_stale(b);
  // (optional terms: the term pass takes the tile, and the same stride and candidate slots)
  if (b->opt) return batch_configure_impl(b->opt, tile_docs, pilot_stride, cand_cap);
  return IRS_HIP_OK;
}

static int batch_set_path_impl(irs_hip_batch* b, int path) {
  if (!b || path < IRS_HIP_PATH_AUTO || path > IRS_HIP_PATH_JOINED) return IRS_HIP_EINVAL;
  if (!quiet_for_setter(b)) return IRS_HIP_EHIP;
  b->path_pref = path;
  deal_is_stale(b);
  return IRS_HIP_OK;
}

static int batch_set_shared_threshold_impl(irs_hip_batch* b, int enable) {
  if (!b) return IRS_HIP_EINVAL;
  if (!quiet_for_setter(b)) return IRS_HIP_EHIP;
  b->groups.shared = enable != 0;
  deal_is_stale(b);
  if (b->opt) return batch_set_shared_threshold_impl(b->opt, enable);   // (both passes)
  return IRS_HIP_OK;
}

static int batch_set_comm_impl(irs_hip_batch* b, irs_hip_comm* comm) {
  if (!b) return IRS_HIP_EINVAL;
  if (b->opt) return IRS_HIP_EUNSUPPORTED;   // (optional terms: two passes, one rank)
  if (b->wide.on() || b->clause.on() || b->tree.on()) return IRS_HIP_EUNSUPPORTED;   // (wide units, Ors of clauses and tree queries keep thresholds of their own)
  if (!quiet_for_setter(b)) return IRS_HIP_EHIP;
  if (comm && !b->groups.d_agree.p && !b->groups.d_agree.alloc(64)) return IRS_HIP_ENOMEM;
  b->comm = comm;
  deal_is_stale(b);
  return IRS_HIP_OK;
}

static int batch_set_paired_tiles_impl(irs_hip_batch* b, int enable) {
  if (!b) return IRS_HIP_EINVAL;
  if (!quiet_for_setter(b)) return IRS_HIP_EHIP;
  const bool allowed = enable != 0, forced = enable == 2;
  // (the deal makes bound images only for a launch that will run paired: dealt anew)
  if (allowed != b->join.pairs_allowed || forced != b->join.pairs_forced) deal_is_stale(b);
  b->join.pairs_allowed = allowed;
  b->join.pairs_forced = forced;
  return IRS_HIP_OK;
}
static int batch_set_wand_impl(irs_hip_batch* b, int enable) {
  if (!b) return IRS_HIP_EINVAL;
  if (b->ran) return IRS_HIP_EINVAL;   // before the first run: the segment records are uploaded once
  if (!quiet_for_setter(b)) return IRS_HIP_EHIP;
  if (b->opt) return IRS_HIP_OK;   // (optional terms: neither pass is pruned)
  b->wand = enable != 0;
  // (which path the batch takes depends on it; a plan queued ahead was made without the tile bounds)
  deal_is_stale(b);
  if (!b->wand) return IRS_HIP_OK;
  std::vector<DevSegment> dsegs;
  for (irs_hip_segment* sg : b->segs) {
    if (const int rc = prepare_blockmax(sg)) return rc;
    dsegs.push_back(sg->dev);
  }
  if (!b->up.copy(b->d_segs.p, dsegs.data(), dsegs.size() * sizeof(DevSegment)))
    return IRS_HIP_ENOMEM;
  return IRS_HIP_OK;
}

static int batch_set_min_scores_impl(irs_hip_batch* b, const float* min_scores) {
  if (!b) return IRS_HIP_EINVAL;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  // (optional terms: a doc's score is whole in either pass, so both filter by the caller's own)
  if (b->opt)
    if (const int rc = batch_set_min_scores_impl(b->opt, min_scores)) return rc;
  if (!min_scores) {
    b->has_min = false;
    return IRS_HIP_OK;
  }
  std::vector<float> mins(b->nq, 0.f);
  for (uint32_t u = 0; u < b->nq; ++u) {
    const float m = min_scores[u % b->nq_user];
    if (!(m >= 0.f)) return IRS_HIP_EINVAL;   // (also NaN)
    mins[u] = m;
  }
  if (!quiesce(b)) return IRS_HIP_EHIP;
  if (!b->d_min_bin.alloc(mins.size() * 4) || !b->d_min_score.alloc(mins.size() * 4))
    return IRS_HIP_ENOMEM;
  b->min_scores.swap(mins);
  b->has_min = true;
  b->min_dirty = true;   // (the bins go out with the next run: stage_min_bins)
  return IRS_HIP_OK;
}

// irs_hip_batch_set_doc_sets / _host: the rows ([n_rows][n_words] u64, device memory the caller
// keeps valid — or host memory, copied into a block of the batch) and every unit's row.  The masks
// are made anew and the units dealt again: a restricted unit is a masked unit.
static int batch_set_doc_sets_impl(irs_hip_batch* b, const void* sets, bool host, uint64_t n_rows,
                                   uint64_t n_words, const uint32_t* row_of_unit) {
  if (!b) return IRS_HIP_EINVAL;
  // (optional terms: the term pass's doc sets are the phrase pass's output)
  if (b->opt) return IRS_HIP_EUNSUPPORTED;
  // (wide units, Ors of clauses and tree queries read the streams every unit shares: a mask of their own cannot ride there)
  if (b->wide.on() || b->clause.on() || b->tree.on()) return IRS_HIP_EUNSUPPORTED;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  std::vector<uint32_t> rows;
  if (row_of_unit && n_rows) {
    bool any = false;
    for (uint32_t u = 0; u < b->nq; ++u) {
      const uint32_t r = row_of_unit[u];
      if (r == IRS_HIP_NO_DOC_SET) continue;
      // every doc of the unit's segment has a bit in its row
      if (r >= n_rows || 64u * n_words <= uint64_t(b->segs[u / b->nq_user]->dev.num_docs) ||
          n_words > 0x4000000ull)
        return IRS_HIP_EINVAL;
      any = true;
    }
    if (any && !sets) return IRS_HIP_EINVAL;
    if (any) rows.assign(row_of_unit, row_of_unit + b->nq);   // (none restricted: the same as cleared)
  }
  if (!quiesce(b)) return IRS_HIP_EHIP;
  ExclWork& x = b->excl;
  b->up.pending.erase(std::remove_if(b->up.pending.begin(), b->up.pending.end(), [&](const Stager::Piece& p) {
    return x.d_own.p && p.dst == x.d_own.p;
  }), b->up.pending.end());
  int rc = IRS_HIP_OK;
  x.sets = static_cast<const uint64_t*>(sets);
  if (rows.empty() || !host) {
    x.d_own.release();
  } else {
    // the host form: the rows go out with the batch's next uploads, into memory of its own
    const size_t bytes = size_t(n_rows) * n_words * 8u;
    void* at = x.d_own.alloc(bytes) ? b->up.put(x.d_own.p, bytes) : nullptr;
    if (at) {
      std::memcpy(at, sets, bytes);
      x.sets = x.d_own.as<uint64_t>();
    } else {   // (the batch is left without filters)
      x.d_own.release();
      rows.clear();
      rc = IRS_HIP_ENOMEM;
    }
  }
  x.row_of.swap(rows);
  x.set_rows = x.sets_on() ? n_rows : 0;
  x.set_words = x.sets_on() ? n_words : 0;
  if (!x.sets_on()) x.sets = nullptr;
  b->match.built = false;   // (the match units carry the masks' addresses)
  b->score_docs.built = false;   // (and so do the score-docs units)
  deal_is_stale(b);
  const int rc2 = build_masks(b);
  return rc != IRS_HIP_OK ? rc : rc2;
}

// irs_hip_batch_doc_set_stats: what the doc sets let the last run skip
static int batch_doc_set_stats_impl(irs_hip_batch* b, uint64_t* tiles, uint64_t* tiles_skipped,
                                    uint64_t* leads, uint64_t* leads_skipped) {
  if (!b || !b->ran) return IRS_HIP_EINVAL;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  uint64_t t = 0, ts = 0, l[2] = {0, 0};
  const ExclWork& x = b->excl;
  if (x.sets_on()) {
    if (!run_done(b)) return IRS_HIP_EHIP;
    if (!b->phrase && !b->tiles.units.empty()) {
      std::vector<uint8_t> live(b->tiles.n_total);
      if (!live.empty() && (!rt::d2h(live.data(), x.d_tile_live.p, live.size(), nullptr) || !rt::sync(nullptr)))
        return IRS_HIP_EHIP;
      for (uint32_t u : b->tiles.units) {
        if (!x.restricted[u]) continue;
        const DevQuery& dq = b->queries[u];
        t += dq.n_tiles;
        for (uint32_t i = 0; i < dq.n_tiles; ++i) ts += live[dq.tile_base + i] ? 0u : 1u;
      }
    }
    if (x.leads_counted && x.d_leads.p) {
      if (!rt::d2h(l, x.d_leads.p, sizeof l, nullptr) || !rt::sync(nullptr)) return IRS_HIP_EHIP;
    }
  }
  if (tiles) *tiles = t;
  if (tiles_skipped) *tiles_skipped = ts;
  if (leads) *leads = l[0];
  if (leads_skipped) *leads_skipped = l[1];
  return IRS_HIP_OK;
}

static int comm_init_rank_impl(int32_t device, const uint8_t* id, int32_t n_ranks, int32_t rank,
                               irs_hip_comm** out) {
  if (!id || !out || n_ranks < 1 || rank < 0 || rank >= n_ranks) return IRS_HIP_EINVAL;
  *out = nullptr;
  if (!device_usable(device)) return IRS_HIP_EHIP;
  irs_hip_comm* c = new (std::nothrow) irs_hip_comm;
  if (!c) return IRS_HIP_ENOMEM;
  c->device = device;
  c->n_ranks = n_ranks;
  c->rank = rank;
  if (!rt::comm::init_rank(&c->h, n_ranks, id, rank)) {
    delete c;
    return IRS_HIP_EHIP;
  }
  *out = c;
  return IRS_HIP_OK;
}

static int topk_allgather_impl(irs_hip_comm* c, const void* d_send, void* d_recv,
                               uint64_t bytes_per_rank, void* stream) {
  if (!c || !d_send || !d_recv || !bytes_per_rank) return IRS_HIP_EINVAL;
  if (!rt::set_device(c->device)) return IRS_HIP_EHIP;
  return rt::comm::all_gather(c->h, d_send, d_recv, bytes_per_rank,
                              static_cast<rt::stream_t>(stream))
             ? IRS_HIP_OK : IRS_HIP_EHIP;
}

static int batch_touched_impl(irs_hip_batch* b, uint64_t* doc_bytes, uint64_t* positions) {
  if (!b || !b->ran || !b->count_touched) return IRS_HIP_EINVAL;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  std::vector<uint64_t> v(size_t(b->nq) * 2);
  if (!run_done(b) || !rt::d2h(v.data(), b->d_touched.p, v.size() * 8, b->stream) || !rt::sync(b->stream))
    return IRS_HIP_EHIP;
  uint64_t bytes = 0, pos = 0;
  for (uint32_t u = 0; u < b->nq; ++u) {
    bytes += v[2 * u];
    pos += v[2 * u + 1];
  }
  if (doc_bytes) *doc_bytes = bytes;
  if (positions) *positions = pos;
  return IRS_HIP_OK;
}

static int batch_profile_impl(irs_hip_batch* b, int enable) {
  if (!b) return IRS_HIP_EINVAL;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  if (enable & 1)
    for (Event& e : b->sync.prof)
      if (!e.create()) return IRS_HIP_EHIP;
  b->profile = (enable & 1) != 0;
  b->count_touched = (enable & 2) != 0;
  return IRS_HIP_OK;
}

// irs_hip_batch_unit_mask: the mask the unit's last run tested, in irs_hip_bit_union's layout
static int batch_unit_mask_impl(irs_hip_batch* b, uint32_t unit, uint64_t* set, uint64_t n_words) {
  if (!b || !set || unit >= b->nq || !b->ran) return IRS_HIP_EINVAL;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  if (!run_done(b)) return IRS_HIP_EHIP;
  const DevQuery& dq = b->queries[unit];
  const uint32_t num_docs = b->segs[dq.seg]->dev.num_docs;
  std::fill(set, set + n_words, uint64_t(0));
  if (!dq.dead) return IRS_HIP_OK;
  std::vector<uint32_t> w(dead_words(num_docs));
  if (!rt::d2h(w.data(), dq.dead, w.size() * 4, nullptr) || !rt::sync(nullptr)) return IRS_HIP_EHIP;
  for (uint64_t j = 0; j < uint64_t(num_docs); ++j) {   // bit j = doc j + kDocMin
    const uint64_t doc = j + kDocMin;
    if ((w[j >> 5] >> (j & 31u)) & 1u && doc < 64 * n_words) set[doc >> 6] |= uint64_t(1) << (doc & 63u);
  }
  return IRS_HIP_OK;
}

// the stages of a run, run_impl and batch_plan_impl (here, behind everything they call: the kernel
// templates they launch are instantiated — and laid out in the code object — in this order)
#include "run.h"

static int batch_run_impl(irs_hip_batch* b, void* stream) {
  if (!b) return IRS_HIP_EINVAL;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  rt::stream_t st = static_cast<rt::stream_t>(stream);
  // (what a queued run returns is reported by the next call on the batch)
  if (worker::wanted(b) && worker::submit(b, [b, st] { return run_impl(b, st); })) return IRS_HIP_OK;
  return run_impl(b, st);
}

// k_select flagged a problem with the candidates of some query.
//   underflow: the estimated threshold was too high.  Re-run with the sound one
//     (the batch stays in sound mode from then on).
//   overflow: the candidate buffer was too small — the pilot sample was not
//     representative, or many docs tie at the k-th score bin.  Re-run exactly:
//     first with a full histogram pass (stride 1), then with the buffer grown to
//     the largest candidate count seen.
// Results are never silently truncated.
// Recovery of a batch whose threshold spans ranks (irs_hip_batch_set_comm) is decided by ALL ranks
// or by none.  Every rank enters recover() together — the status bits are all-reduced inside the
// run — but whether a rank CAN re-run is its own business (memory for a larger candidate buffer,
// an overflow it cannot afford): one that returned by itself would leave the others waiting in the
// re-run's collectives for ever.  So each such exit is a vote: the ranks all-reduce "I cannot", and
// a re-run happens only when the sum is zero.  local_rc: what this rank would return by itself
// (IRS_HIP_OK: it can go on).  Returns IRS_HIP_OK when every rank can, this rank's own error when
// it cannot, IRS_HIP_EPEER when only others cannot.  Without a communicator: local_rc.
static int all_ranks_can(irs_hip_batch* b, int local_rc) {
  if (!b->comm || b->phrase) return local_rc;
  uint32_t vote = local_rc == IRS_HIP_OK ? 0u : 1u;
  if (!b->groups.d_agree.p || !rt::h2d(b->groups.d_agree.p, &vote, 4, b->stream) ||
      !rt::comm::all_reduce_u32(b->comm->h, b->groups.d_agree.p, 1, b->stream) ||
      !rt::d2h(&vote, b->groups.d_agree.p, 4, b->stream) || !rt::sync(b->stream))
    return local_rc != IRS_HIP_OK ? local_rc : IRS_HIP_EHIP;
  if (local_rc != IRS_HIP_OK) return local_rc;
  return vote ? IRS_HIP_EPEER : IRS_HIP_OK;
}

static int recover_overflow(irs_hip_batch* b) {
  constexpr uint64_t kMaxCandBytes = 16ull << 30;
  for (int attempt = 0; attempt < 3; ++attempt) {
    // the failed run counted every candidate it met, also those it could not store: with the
    // same threshold a buffer of that size holds them all.  Growing it is the cheap way out;
    // only when that is not affordable, a full histogram pass (stride 1: the tightest sound
    // threshold) comes first — it costs as much as the scoring pass itself.
    std::vector<uint32_t> cc(b->nq);
    if (!run_done(b) || !rt::d2h(cc.data(), b->d_cand_count.p, size_t(b->nq) * 4, b->stream) ||
        !rt::sync(b->stream))
      return IRS_HIP_EHIP;
    const uint64_t need = uint64_t(*std::max_element(cc.begin(), cc.end())) + 1024;
    const bool affordable = need * b->nq * sizeof(uint64_t) <= kMaxCandBytes;
    if (need - 1024 > b->cand_cap && need <= 262144) {
      for (irs_hip_segment* sg : b->segs) {   // (what later batches on these segments start with)
        uint32_t seen = sg->cand_cap_hint.load();
        while (seen < need && !sg->cand_cap_hint.compare_exchange_weak(seen, uint32_t(need))) {}
      }
    }
    int can = IRS_HIP_OK;
    if (b->comm && need - 1024 <= b->cand_cap) {
      // (the overflow is another rank's: this one only takes part in the re-run's collectives)
    } else if (need > b->cand_cap && affordable) {
      if (b->d_cands.alloc(need * b->nq * sizeof(uint64_t))) b->cand_cap = uint32_t(need);
      else can = IRS_HIP_ENOMEM;
    } else if (b->stride_eff != 1) {
      b->stride_eff = 1;
    } else {
      can = IRS_HIP_EOVERFLOW;
    }
    if (const int all = all_ranks_can(b, can)) return all;
    int rc = run_impl(b, b->stream);
    if (rc != IRS_HIP_OK) return rc;
    uint32_t status = 0;
    if (!run_status(b, &status)) return IRS_HIP_EHIP;
    if (!(status & kStatusOverflow)) return IRS_HIP_OK;
  }
  return IRS_HIP_EOVERFLOW;
}

static int recover_now(irs_hip_batch* b, uint32_t status) {
  ++b->reruns;
  if (std::getenv("IRS_HIP_TRACE")) {   // which units made the batch run again
    std::vector<uint32_t> cc(b->nq), oc(b->nq);
    std::vector<unsigned long long> hh(b->nq);
    if (run_done(b) && rt::d2h(cc.data(), b->d_cand_count.p, size_t(b->nq) * 4, b->stream) &&
        rt::d2h(oc.data(), b->d_out_count.p, size_t(b->nq) * 4, b->stream) &&
        rt::d2h(hh.data(), b->d_hits.p, size_t(b->nq) * 8, b->stream) && rt::sync(b->stream)) {
      uint32_t under = 0, over = 0, first_u = ~0u, first_o = ~0u;
      for (uint32_t u = 0; u < b->nq; ++u) {
        if (cc[u] > b->cand_cap) { ++over; if (first_o == ~0u) first_o = u; }
        if (oc[u] < b->queries[u].k && hh[u] > oc[u]) { ++under; if (first_u == ~0u) first_u = u; }
      }
      std::fprintf(stderr, "[irs_hip] re-run: status %u, %u units short of k (first %u: listed %u of %llu matches, "
                   "%u candidates), %u over the candidate cap %u (first %u: %u)\n", status, under, first_u,
                   first_u != ~0u ? oc[first_u] : 0u, first_u != ~0u ? hh[first_u] : 0ull,
                   first_u != ~0u ? cc[first_u] : 0u, over, b->cand_cap, first_o, first_o != ~0u ? cc[first_o] : 0u);
    }
  }
  if (status & kStatusUnderflow) {
    b->estimate = false;
    // the sound threshold admits about k * (pilot stride) candidates per unit: a denser pilot
    // keeps the candidate buffer of a large batch (units x cap x 8 bytes) in bounds
    b->stride_eff = std::min<uint32_t>(b->stride_eff, 16);
    const uint32_t cap = default_cand_cap(b);  // the sound threshold admits more candidates
    int can = IRS_HIP_OK;
    if (cap > b->cand_cap) {
      if (b->d_cands.alloc(uint64_t(b->nq) * cap * sizeof(uint64_t))) b->cand_cap = cap;
      else can = IRS_HIP_ENOMEM;
    }
    if (const int all = all_ranks_can(b, can)) return all;
    const int rc = run_impl(b, b->stream);
    if (rc != IRS_HIP_OK) return rc;
    if (!run_status(b, &status)) return IRS_HIP_EHIP;
    if (status & kStatusUnderflow) return IRS_HIP_EHIP;  // cannot happen with a sound threshold
  }
  return (status & kStatusOverflow) ? recover_overflow(b) : IRS_HIP_OK;
}

// The re-run of a batch whose threshold spans ranks issues collectives (the vote, the run's two
// all-reduces): it takes its turn in the device's worker queue BEHIND the runs the caller has
// submitted since — on every rank alike, because every rank makes the same calls in the same order
// and reaches the same verdict — instead of racing them from the caller's thread.
static int recover(irs_hip_batch* b, uint32_t status) {
  if (b->comm && !b->phrase && worker::wanted(b) &&
      worker::submit(b, [b, status] { return recover_now(b, status); }))
    return settle(b);
  return recover_now(b, status);
}

static int batch_timings_impl(irs_hip_batch* b, float ms[IRS_HIP_K_COUNT]) {
  if (!b || !ms || !b->profile || !b->ran) return IRS_HIP_EINVAL;
  // (the batch's own last run: later work on the stream is not waited for)
  if (!rt::set_device(b->seg->device) || !run_done(b)) return IRS_HIP_EHIP;
  for (int i = 0; i < IRS_HIP_K_COUNT; ++i)
    if (!rt::event_elapsed(&ms[i], b->sync.prof[2 * i].e, b->sync.prof[2 * i + 1].e)) return IRS_HIP_EHIP;
  return IRS_HIP_OK;
}

static int verify_term_pass(irs_hip_batch* b);

static int batch_results_impl(irs_hip_batch* b, irs_hip_hit* hits, uint32_t k_stride,
                          uint32_t* counts, uint64_t* total_hits) {
  if (!b || !hits || !counts || !b->ran || k_stride < b->k_max) return IRS_HIP_EINVAL;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  uint32_t status = 0;
  // hits land in a page-locked buffer owned by the batch (a pageable destination would
  // be staged by the runtime at a fraction of the PCIe rate), then go to the caller's layout
  const size_t hit_bytes = size_t(b->nq) * b->k_max * sizeof(Hit);
  if (b->sync.h_pin.n < hit_bytes && !b->sync.h_pin.alloc(hit_bytes)) return IRS_HIP_ENOMEM;
  const Hit* tmp = b->sync.h_pin.as<Hit>();
  // (behind the run's own end — `done`, which may lie on the tail stream — AND, as ever, behind
  // whatever else the caller's stream holds)
  if (!run_status(b, &status) || !rt::sync(b->stream)) return IRS_HIP_EHIP;
  if (status & (kStatusOverflow | kStatusUnderflow)) {
    const int rc = recover(b, status);
    if (rc != IRS_HIP_OK) return rc;
    status = 0;
  }
  if (const int rc = verify_term_pass(b)) return rc;
  if (!rt::d2h(b->sync.h_pin.p, out_hits(b), hit_bytes, b->stream) ||
      !rt::d2h(counts, out_counts(b), size_t(b->nq) * 4, b->stream) ||
      (total_hits && !rt::d2h(total_hits, out_totals(b), size_t(b->nq) * 8, b->stream)) ||
      !rt::sync(b->stream))
    return IRS_HIP_EHIP;
  if (status & kStatusOverflow) return IRS_HIP_EOVERFLOW;
  for (uint32_t q = 0; q < b->nq; ++q) {
    for (uint32_t i = 0; i < counts[q]; ++i) {
      const Hit& h = tmp[size_t(q) * b->k_max + i];
      hits[size_t(q) * k_stride + i].score = h.score;
      hits[size_t(q) * k_stride + i].doc = h.doc;
    }
  }
  return IRS_HIP_OK;
}

// Waits for the batch, reads its status word and re-executes it when the candidate
// buffer or the threshold estimate fell short.  Afterwards d_out / d_out_count hold the
// exact top-k.
// Waits for the batch's own last run (its event: work the caller queued behind it on the same
// stream — the next batch's kernels, say — keeps running) and reads the status it left.
static int verify_run(irs_hip_batch* b) {
  uint32_t status = 0;
  if (!run_status(b, &status)) return IRS_HIP_EHIP;
  if (status & (kStatusOverflow | kStatusUnderflow)) {
    const int rc = recover(b, status);
    if (rc != IRS_HIP_OK) return rc;
    if (!after_run(b)) return IRS_HIP_EHIP;
  }
  return verify_term_pass(b);
}

// Optional terms: the phrase pass is through and sound (a re-run of it ran the term pass and the
// union again); now the term pass's own status.  Its re-run changes nothing the phrase pass wrote —
// k_phrase_or takes every doc the phrase matches out of the doc sets, whatever the threshold — so
// only the union is made again.
static int verify_term_pass(irs_hip_batch* b) {
  if (!b->opt) return IRS_HIP_OK;
  const uint32_t before = b->opt->reruns;
  if (const int rc = verify_run(b->opt)) return rc;
  if (b->opt->reruns == before) return IRS_HIP_OK;
  if (!launch_union(b, b->stream) || !rt::sync(b->stream)) return IRS_HIP_EHIP;
  return IRS_HIP_OK;
}

static int batch_device_results_impl(irs_hip_batch* b, void** d_hits, void** d_counts,
                                 uint32_t* k_max) {
  if (!b || !b->ran) return IRS_HIP_EINVAL;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  const int rc = verify_run(b);
  if (rc != IRS_HIP_OK) return rc;
  if (d_hits) *d_hits = out_hits(b);
  if (d_counts) *d_counts = out_counts(b);
  if (k_max) *k_max = b->k_max;
  return IRS_HIP_OK;
}

static int batch_results_to_device_impl(irs_hip_batch* b, void* d_hits, void* d_counts,
                                    void* stream) {
  if (!b || !b->ran || !d_hits || !d_counts) return IRS_HIP_EINVAL;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  rt::stream_t st = static_cast<rt::stream_t>(stream);
  const int rc = verify_run(b);
  if (rc != IRS_HIP_OK) return rc;
  if (!rt::d2d(d_hits, out_hits(b), size_t(b->nq) * b->k_max * sizeof(Hit), st) ||
      !rt::d2d(d_counts, out_counts(b), size_t(b->nq) * 4, st))
    return IRS_HIP_EHIP;
  // (destroy must not hand d_out back to the pool while these copies are queued)
  return b->sync.used.mark(st) ? IRS_HIP_OK : IRS_HIP_EHIP;
}

// sync.h_res: the hits, then the counts, then the totals of irs_hip_batch_results_to_host
struct HostResults {
  size_t hit_bytes, cnt_off, tot_off, total;
  explicit HostResults(const irs_hip_batch* b)
      : hit_bytes(size_t(b->nq) * b->k_max * sizeof(Hit)), cnt_off((hit_bytes + 63) & ~size_t(63)),
        tot_off(cnt_off + ((size_t(b->nq) * 4 + 63) & ~size_t(63))), total(tot_off + size_t(b->nq) * 8) {}
};

// The checked results on their way to page-locked host memory, asynchronously: where the
// reference's harness ends (index-search.cpp:782-807: the sorted (score, doc) pairs of every task
// in host memory).  The copy is queued on `stream` (null: the device's download stream) behind the
// batch's own last run — NOT behind whatever the caller has queued since, so the results of batch i
// cross PCIe while the kernels of batch i + 1 run.
static int batch_results_to_host_impl(irs_hip_batch* b, void* stream) {
  if (!b || !b->ran) return IRS_HIP_EINVAL;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  const int rc = verify_run(b);
  if (rc != IRS_HIP_OK) return rc;
  const HostResults r(b);
  if (!b->sync.host.sync()) return IRS_HIP_EHIP;   // (the previous copy)
  if (b->sync.h_res.n < r.total && !b->sync.h_res.alloc(r.total)) return IRS_HIP_ENOMEM;
  rt::stream_t st = stream ? static_cast<rt::stream_t>(stream) : download_stream(b->seg->device);
  if (!st) st = b->stream;
  uint8_t* h = b->sync.h_res.as<uint8_t>();
  if (!run_done_on(b, st) ||
      !rt::d2h(h, out_hits(b), r.hit_bytes, st) ||
      !rt::d2h(h + r.cnt_off, out_counts(b), size_t(b->nq) * 4, st) ||
      !rt::d2h(h + r.tot_off, out_totals(b), size_t(b->nq) * 8, st) ||
      !b->sync.host.mark(st))
    return IRS_HIP_EHIP;
  return IRS_HIP_OK;
}

static int batch_host_results_impl(irs_hip_batch* b, const irs_hip_hit** hits, uint32_t* k_stride,
                                   const uint32_t** counts, const uint64_t** total_hits) {
  if (!b || !b->sync.host.pending()) return IRS_HIP_EINVAL;   // (no copy since the last run)
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  if (!b->sync.host.sync_keep()) return IRS_HIP_EHIP;   // (they stay there to be handed out again)
  const HostResults r(b);
  const uint8_t* h = b->sync.h_res.as<uint8_t>();
  static_assert(sizeof(irs_hip_hit) == sizeof(Hit), "irs_hip_hit is the device's Hit");
  if (hits) *hits = reinterpret_cast<const irs_hip_hit*>(h);
  if (k_stride) *k_stride = b->k_max;
  if (counts) *counts = reinterpret_cast<const uint32_t*>(h + r.cnt_off);
  if (total_hits) *total_hits = reinterpret_cast<const uint64_t*>(h + r.tot_off);
  return IRS_HIP_OK;
}

void irs_hip_batch_destroy(irs_hip_batch* b) {
  if (!b) return;
  settle(b);
  rt::set_device(b->seg->device);
  // (its buffers go back to the pool)
  bool waited = quiet_for_destroy(b);
  if (!waited && b->ran) {
    bool made = false;
    rt::stream_t ts = tail_stream(b->seg->device, &made);
    waited = rt::sync(b->stream) && (!b->sync.tail_used || !made || rt::sync(ts));
  }
  release_streams(b, waited);   // (its pins in the device's stream cache)
  // (optional terms: the term pass reads this batch's d_taken — it goes first)
  if (b->opt) irs_hip_batch_destroy(b->opt);
  // (the batch's events go with it)
  delete b;
}

static int merge_topk_impl(int32_t device, const void* const* d_lists, const void* const* d_counts,
                       const uint32_t* seg_ids, uint32_t n_lists, uint32_t n_queries,
                       uint32_t k, void* d_out, void* d_out_seg, void* d_out_counts,
                       void* stream) {
  if (!d_lists || !d_counts || !seg_ids || !n_lists || n_lists > 16 || !n_queries || !k ||
      !d_out || !d_out_seg || !d_out_counts)
    return IRS_HIP_EINVAL;
  if (uint64_t(n_lists) * k > kMergeMax) return IRS_HIP_EUNSUPPORTED;
  if (!device_usable(device)) return IRS_HIP_EHIP;
  MergeLists ml{};
  for (uint32_t i = 0; i < n_lists; ++i) {
    ml.hits[i] = static_cast<const Hit*>(d_lists[i]);
    ml.counts[i] = static_cast<const uint32_t*>(d_counts[i]);
    ml.seg_ids[i] = seg_ids[i];
  }
  const size_t smem = merge_smem_bytes(n_lists, k);
  if (!big_smem(k_merge_topk, smem)) return IRS_HIP_EHIP;
  RT_LAUNCH(k_merge_topk, n_queries, kThreads, smem, static_cast<rt::stream_t>(stream), ml,
            n_lists, k, static_cast<Hit*>(d_out), static_cast<uint32_t*>(d_out_seg),
            static_cast<uint32_t*>(d_out_counts));
  return rt::last_error_ok() ? IRS_HIP_OK : IRS_HIP_EHIP;
}


// ---- the exported entry points: nothing C++ leaves this library (status codes only) ----
int irs_hip_device_arch(int32_t device, char* buf, size_t cap) {
  return guarded([&]() -> int {
    if (!buf || !cap) return IRS_HIP_EINVAL;
    if (device < 0 || device >= rt::device_count() || !rt::device_arch(device, buf, cap))
      return IRS_HIP_EHIP;
    return IRS_HIP_OK;
  });
}
int irs_hip_segment_open(const irs_hip_segment_desc* d, irs_hip_segment** out) {
  return guarded([&] { return segment_open_impl(d, out); });
}
int irs_hip_decode_term(irs_hip_segment* seg, uint32_t term, uint32_t* docs, uint32_t* freqs, uint32_t cap, uint32_t* count) {
  return guarded([&] { return decode_term_impl(seg, term, docs, freqs, cap, count); });
}
int irs_hip_decode_positions(irs_hip_segment* seg, uint32_t term, uint32_t* positions, uint64_t cap, uint64_t* count) {
  return guarded([&] { return decode_positions_impl(seg, term, positions, cap, count); });
}
int irs_hip_bit_union(irs_hip_segment* seg, const uint32_t* terms, uint32_t n_terms, uint64_t* set, uint64_t n_words, uint64_t* count) {
  return guarded([&] { return bit_union_impl(seg, terms, n_terms, set, n_words, count); });
}
int irs_hip_bit_union_counts(irs_hip_segment* seg, const uint32_t* terms, const uint32_t* offsets, uint32_t n_sets, uint64_t* counts) {
  return guarded([&] { return bit_union_counts_impl(seg, terms, offsets, n_sets, counts); });
}
int irs_hip_term_directory(irs_hip_segment* seg, uint32_t term, uint32_t* last_docs, uint64_t* offsets, uint32_t cap, uint32_t* count) {
  return guarded([&] { return term_directory_impl(seg, term, last_docs, offsets, cap, count); });
}
int irs_hip_batch_create(irs_hip_segment* seg, const irs_hip_query* queries, uint32_t nq, const irs_hip_term_scorer* terms, uint32_t n_entries, irs_hip_batch** out) {
  return guarded([&] { return irs_hip_batch_create_multi(&seg, 1, queries, nq, terms, n_entries, out); });
}
int irs_hip_batch_create_multi(irs_hip_segment* const* segs, uint32_t n_segs, const irs_hip_query* queries, uint32_t nq_user, const irs_hip_term_scorer* all_terms, uint32_t n_entries, irs_hip_batch** out) {
  return guarded([&] { return batch_create_multi_impl(segs, n_segs, queries, nq_user, all_terms, n_entries, out); });
}
int irs_hip_batch_configure(irs_hip_batch* b, uint32_t tile_docs, uint32_t pilot_stride, uint32_t cand_cap) {
  return settled(b, [&] { return batch_configure_impl(b, tile_docs, pilot_stride, cand_cap); });
}
int irs_hip_batch_profile(irs_hip_batch* b, int enable) {
  return settled(b, [&] { return batch_profile_impl(b, enable); });
}
int irs_hip_batch_set_path(irs_hip_batch* b, int path) {
  return settled(b, [&] { return batch_set_path_impl(b, path); });
}
int irs_hip_batch_set_shared_threshold(irs_hip_batch* b, int enable) {
  return settled(b, [&] { return batch_set_shared_threshold_impl(b, enable); });
}
int irs_hip_batch_set_comm(irs_hip_batch* b, irs_hip_comm* comm) {
  return settled(b, [&] { return batch_set_comm_impl(b, comm); });
}
int irs_hip_batch_set_async(irs_hip_batch* b, int enable) {
  return settled(b, [&]() -> int {
    if (!b) return IRS_HIP_EINVAL;
    b->sync.async_pref = enable < 0 ? -1 : (enable ? 1 : 0);
    return IRS_HIP_OK;
  });
}
int irs_hip_batch_path(irs_hip_batch* b, int* path) {
  return settled(b, [&]() -> int {
    if (!b || !path) return IRS_HIP_EINVAL;
    *path = b->join.on() ? IRS_HIP_PATH_JOINED : IRS_HIP_PATH_ITEMS;
    return IRS_HIP_OK;
  });
}
int irs_hip_batch_set_paired_tiles(irs_hip_batch* b, int enable) {
  return settled(b, [&] { return batch_set_paired_tiles_impl(b, enable); });
}
int irs_hip_batch_paired_tiles(irs_hip_batch* b, int* used) {
  return settled(b, [&]() -> int {
    if (!b || !used) return IRS_HIP_EINVAL;
    *used = (b->join.on() && b->join.pairs_used) ? 1 : 0;
    return IRS_HIP_OK;
  });
}
int irs_hip_batch_tail_stream_used(irs_hip_batch* b, int* used) {
  return settled(b, [&]() -> int {
    if (!b || !used) return IRS_HIP_EINVAL;
    *used = (b->ran && b->sync.tail_used) ? 1 : 0;
    return IRS_HIP_OK;
  });
}
int irs_hip_batch_set_wand(irs_hip_batch* b, int enable) {
  return settled(b, [&] { return batch_set_wand_impl(b, enable); });
}
int irs_hip_batch_set_min_scores(irs_hip_batch* b, const float* min_scores) {
  return settled(b, [&] { return batch_set_min_scores_impl(b, min_scores); });
}
int irs_hip_term_blockmax(irs_hip_segment* seg, uint32_t term, uint32_t* max_freqs,
                          uint32_t* min_norms, uint32_t cap, uint32_t* count) {
  return guarded([&] { return term_blockmax_impl(seg, term, max_freqs, min_norms, cap, count); });
}
int irs_hip_segment_wand_source(irs_hip_segment* seg, uint64_t* from_index, uint64_t* total) {
  return guarded([&] { return segment_wand_source_impl(seg, from_index, total); });
}
int irs_hip_device_alloc(int32_t device, uint64_t bytes, void** d_out) {
  return guarded([&] {
    if (!d_out) return int(IRS_HIP_EINVAL);
    *d_out = nullptr;
    if (!device_usable(device)) return int(IRS_HIP_EHIP);
    *d_out = rt::dmalloc(bytes);
    return int(*d_out ? IRS_HIP_OK : IRS_HIP_ENOMEM);
  });
}
void irs_hip_device_free(int32_t device, void* d_ptr) {
  if (rt::set_device(device)) rt::dfree(d_ptr);
}
int irs_hip_device_upload(int32_t device, void* d_dst, const void* h_src, uint64_t bytes) {
  return guarded([&] {
    if ((!d_dst || !h_src) && bytes) return int(IRS_HIP_EINVAL);
    if (!rt::set_device(device)) return int(IRS_HIP_EHIP);
    return int(rt::h2d(d_dst, h_src, bytes, nullptr) && rt::sync(nullptr) ? IRS_HIP_OK : IRS_HIP_EHIP);
  });
}
int irs_hip_device_download(int32_t device, void* h_dst, const void* d_src, uint64_t bytes) {
  return guarded([&] {
    if ((!h_dst || !d_src) && bytes) return int(IRS_HIP_EINVAL);
    if (!rt::set_device(device)) return int(IRS_HIP_EHIP);
    return int(rt::d2h(h_dst, d_src, bytes, nullptr) && rt::sync(nullptr) ? IRS_HIP_OK : IRS_HIP_EHIP);
  });
}
int irs_hip_device_trim(int32_t device) {
  return guarded([&] {
    if (device < 0 || device >= rt::device_count() || !rt::set_device(device)) return int(IRS_HIP_EHIP);
    scache::drop_unpinned(device, 0);   // (the decoded streams no batch alive references)
    pool::release_all(device, false);
    pool::release_all(device, true);
    return int(IRS_HIP_OK);
  });
}
int irs_hip_device_set_stream_cache(int32_t device, uint64_t bytes) {
  return guarded([&] {
    if (device < 0 || device >= rt::device_count() || !rt::set_device(device)) return int(IRS_HIP_EHIP);
    scache::set_budget(device, bytes);
    return int(IRS_HIP_OK);
  });
}
int irs_hip_device_stream_cache_stats(int32_t device, irs_hip_stream_cache_stats* out) {
  return guarded([&] {
    if (!out) return int(IRS_HIP_EINVAL);
    if (device < 0 || device >= rt::device_count() || !rt::set_device(device)) return int(IRS_HIP_EHIP);
    const uint64_t budget = scache::budget_bytes(device);
    scache::Cache& c = scache::of(device);
    std::lock_guard<std::mutex> lock(c.m);
    out->bytes_held = c.held;
    out->budget = budget;
    out->streams = c.map.size();
    out->hits = c.hits;
    out->misses = c.misses;
    out->evictions = c.evictions;
    return int(IRS_HIP_OK);
  });
}
int irs_hip_batch_stream_counts(irs_hip_batch* b, uint32_t* distinct, uint32_t* decoded) {
  return settled(b, [&]() -> int {
    if (!b || !b->ran) return IRS_HIP_EINVAL;
    if (distinct) *distinct = streams_on(b) ? b->join.n_streams : 0u;
    if (decoded) *decoded = streams_on(b) ? b->join.decoded_last : 0u;
    return IRS_HIP_OK;
  });
}
int irs_hip_batch_wide_units(irs_hip_batch* b, uint32_t* units) {
  return settled(b, [&]() -> int {
    if (!b || !units) return IRS_HIP_EINVAL;
    *units = uint32_t(b->wide.units.size());
    return IRS_HIP_OK;
  });
}
int irs_hip_batch_clause_units(irs_hip_batch* b, uint32_t* units) {
  return settled(b, [&]() -> int {
    if (!b || !units) return IRS_HIP_EINVAL;
    *units = uint32_t(b->clause.units.size());
    return IRS_HIP_OK;
  });
}
int irs_hip_batch_phrase_conj_units(irs_hip_batch* b, uint32_t* units) {
  return settled(b, [&]() -> int {
    if (!b || !units) return IRS_HIP_EINVAL;
    *units = b->blocks.n_several;
    return IRS_HIP_OK;
  });
}
int irs_hip_batch_phrase_disj_units(irs_hip_batch* b, uint32_t* units) {
  return settled(b, [&]() -> int {
    if (!b || !units) return IRS_HIP_EINVAL;
    *units = b->blocks.n_disj;
    return IRS_HIP_OK;
  });
}
int irs_hip_batch_tree_units(irs_hip_batch* b, uint32_t* units) {
  return settled(b, [&]() -> int {
    if (!b || !units) return IRS_HIP_EINVAL;
    *units = uint32_t(b->tree.units.size());
    return IRS_HIP_OK;
  });
}
int irs_hip_batch_image_counts(irs_hip_batch* b, uint32_t* distinct, uint32_t* built) {
  return settled(b, [&]() -> int {
    if (!b || !b->ran) return IRS_HIP_EINVAL;
    const bool on = b->join.on() && b->join.img_on;
    if (distinct) *distinct = on ? b->join.n_images : 0u;
    if (built) *built = on ? b->join.images_built_last : 0u;
    return IRS_HIP_OK;
  });
}
int irs_hip_batch_rescore_paths(irs_hip_batch* b, uint32_t paths[3]) {
  return settled(b, [&]() -> int {
    if (!b || !b->ran || !paths) return IRS_HIP_EINVAL;
    paths[0] = paths[1] = paths[2] = 0;
    if (!b->join.on() || !b->join.pairs_used) return IRS_HIP_OK;
    if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
    if (!run_done(b) || !rt::d2h(paths, rescore_paths(b), 12, b->stream) || !rt::sync(b->stream))
      return IRS_HIP_EHIP;
    return IRS_HIP_OK;
  });
}
int irs_hip_device_image_count(int32_t device, uint64_t* images) {
  return guarded([&] {
    if (!images) return int(IRS_HIP_EINVAL);
    if (device < 0 || device >= rt::device_count() || !rt::set_device(device)) return int(IRS_HIP_EHIP);
    scache::Cache& c = scache::of(device);
    std::lock_guard<std::mutex> lock(c.m);
    *images = c.imap.size();
    return int(IRS_HIP_OK);
  });
}
int irs_hip_join_bound_rule(int32_t kind, float norm_const, float norm_length, uint32_t tf_bound,
                            uint16_t* u, float* scale, float* slack, uint32_t* tile_docs) {
  return guarded([&] {
    if (slack) *slack = kJoinBoundSlack;
    if (tile_docs) *tile_docs = kJoinBoundTile;
    if (!table_kind(kind)) return int(IRS_HIP_EUNSUPPORTED);
    const float sup = join_bound_sup(kind, norm_const, norm_length, tf_bound);
    if (!(sup > 0.f)) return int(IRS_HIP_EUNSUPPORTED);
    const float U = join_bound_scale(sup);
    if (scale) *scale = U;
    if (u)
      for (uint32_t tf = 0; tf < 256u; ++tf)
        for (uint32_t n = 0; n < 256u; ++n)
          u[tf * 256u + n] = uint16_t(join_bound_u(kind, norm_const, norm_length, U, tf, n));
    return int(IRS_HIP_OK);
  });
}
int irs_hip_join_half_rule(float cs, float scale, uint32_t* k) {
  return guarded([&] {
    if (!k || !(cs >= 0.f) || !(scale > 0.f)) return int(IRS_HIP_EINVAL);
    *k = join_half_k(cs, scale);
    return int(IRS_HIP_OK);
  });
}
int irs_hip_join_half_probe(int32_t device, const uint32_t* entries, uint32_t n, uint32_t k,
                            uint32_t high_half, uint32_t* out) {
  return guarded([&] {
    if (!entries || !out || !n || !k || k > 65535u) return int(IRS_HIP_EINVAL);
    if (device < 0 || device >= rt::device_count() || !rt::set_device(device)) return int(IRS_HIP_EHIP);
    uint32_t* d = static_cast<uint32_t*>(rt::dmalloc(size_t(n) * 8));
    if (!d) return int(IRS_HIP_ENOMEM);
    bool ok = rt::h2d(d, entries, size_t(n) * 4, nullptr) && rt::sync(nullptr);
    if (ok) {
      RT_LAUNCH(k_join_half_probe, 1, kThreads, 0, nullptr, d, n, k, high_half, d + n);
      ok = rt::last_error_ok() && rt::d2h(out, d + n, size_t(n) * 4, nullptr) && rt::sync(nullptr);
    }
    rt::dfree(d);
    return int(ok ? IRS_HIP_OK : IRS_HIP_EHIP);
  });
}
int irs_hip_device_sync(int32_t device, void* stream) {
  return guarded([&] {
    if (!rt::set_device(device)) return int(IRS_HIP_EHIP);
    return int(rt::sync(static_cast<rt::stream_t>(stream)) ? IRS_HIP_OK : IRS_HIP_EHIP);
  });
}
int irs_hip_comm_unique_id(uint8_t id[IRS_HIP_COMM_ID_BYTES]) {
  return guarded([&]() -> int {
    if (!id) return IRS_HIP_EINVAL;
    return rt::comm::unique_id(id) ? IRS_HIP_OK : IRS_HIP_EHIP;
  });
}
int irs_hip_comm_init_rank(int32_t device, const uint8_t id[IRS_HIP_COMM_ID_BYTES], int32_t n_ranks,
                           int32_t rank, irs_hip_comm** out) {
  return guarded([&] { return comm_init_rank_impl(device, id, n_ranks, rank, out); });
}
int irs_hip_comm_library(char* buf, size_t cap) {
  return guarded([&] {
    if (!buf || !cap) return int(IRS_HIP_EINVAL);
    return rt::comm::library(buf, cap) ? int(IRS_HIP_OK) : int(IRS_HIP_EHIP);
  });
}
void irs_hip_comm_destroy(irs_hip_comm* c) {
  if (!c) return;
  rt::set_device(c->device);
  rt::comm::destroy(c->h);
  delete c;
}
int irs_hip_topk_allgather(irs_hip_comm* c, const void* d_send, void* d_recv,
                           uint64_t bytes_per_rank, void* stream) {
  return guarded([&] { return topk_allgather_impl(c, d_send, d_recv, bytes_per_rank, stream); });
}
int irs_hip_batch_touched(irs_hip_batch* b, uint64_t* doc_bytes, uint64_t* positions) {
  return settled(b, [&] { return batch_touched_impl(b, doc_bytes, positions); });
}
int irs_hip_batch_unit_mask(irs_hip_batch* b, uint32_t unit, uint64_t* set, uint64_t n_words) {
  return settled(b, [&] { return batch_unit_mask_impl(b, unit, set, n_words); });
}
int irs_hip_batch_set_doc_sets(irs_hip_batch* b, const void* d_sets, uint64_t n_rows, uint64_t n_words, const uint32_t* row_of_unit) {
  return settled(b, [&] { return batch_set_doc_sets_impl(b, d_sets, false, n_rows, n_words, row_of_unit); });
}
int irs_hip_batch_set_doc_sets_host(irs_hip_batch* b, const uint64_t* sets, uint64_t n_rows, uint64_t n_words, const uint32_t* row_of_unit) {
  return settled(b, [&] { return batch_set_doc_sets_impl(b, sets, true, n_rows, n_words, row_of_unit); });
}
int irs_hip_batch_doc_set_stats(irs_hip_batch* b, uint64_t* tiles, uint64_t* tiles_skipped, uint64_t* leads, uint64_t* leads_skipped) {
  return settled(b, [&] { return batch_doc_set_stats_impl(b, tiles, tiles_skipped, leads, leads_skipped); });
}
int irs_hip_batch_match_sets(irs_hip_batch* b, uint64_t* sets, uint64_t n_words, uint64_t* counts) {
  return settled(b, [&] {
    // (plan_match.h: 16 rows per unit, no clauses and no trees)
    if (b && (b->wide.on() || b->clause.on() || b->tree.on())) return int(IRS_HIP_EUNSUPPORTED);
    return batch_match_sets_impl(b, sets, nullptr, n_words, counts, nullptr, nullptr, false);
  });
}
int irs_hip_batch_match_sets_to_device(irs_hip_batch* b, void* d_sets, uint64_t n_words, void* d_counts,
                                       void* stream) {
  return settled(b, [&] {
    if (b && (b->wide.on() || b->clause.on() || b->tree.on())) return int(IRS_HIP_EUNSUPPORTED);
    return batch_match_sets_impl(b, nullptr, d_sets, n_words, nullptr, d_counts,
                                 static_cast<rt::stream_t>(stream), true);
  });
}
int irs_hip_batch_score_docs(irs_hip_batch* b, const uint32_t* docs, const uint64_t* offsets, float* scores,
                             uint8_t* matched) {
  return settled(b, [&] {
    return batch_score_docs_impl(b, docs, offsets, scores, matched, nullptr, nullptr, 0, nullptr, nullptr, nullptr, false);
  });
}
int irs_hip_batch_score_docs_to_device(irs_hip_batch* b, const void* d_docs, const void* d_offsets, uint64_t n_docs,
                                       void* d_scores, void* d_matched, void* stream) {
  return settled(b, [&] {
    return batch_score_docs_impl(b, nullptr, nullptr, nullptr, nullptr, d_docs, d_offsets, n_docs, d_scores,
                                 d_matched, static_cast<rt::stream_t>(stream), true);
  });
}
int irs_hip_batch_nested_sets(irs_hip_batch* b, const irs_hip_nested* nested, uint64_t* sets, uint64_t* counts) {
  return settled(b, [&] { return batch_nested_sets_impl(b, nested, sets, counts, nullptr, nullptr, nullptr, false); });
}
int irs_hip_batch_nested_sets_to_device(irs_hip_batch* b, const irs_hip_nested* nested, void* d_sets, void* d_counts,
                                        void* stream) {
  return settled(b, [&] {
    return batch_nested_sets_impl(b, nested, nullptr, nullptr, d_sets, d_counts, static_cast<rt::stream_t>(stream), true);
  });
}
int irs_hip_batch_nested_topk(irs_hip_batch* b, const irs_hip_nested* nested, irs_hip_hit* hits, uint32_t k_stride,
                              uint32_t* counts, uint64_t* total_hits) {
  return settled(b, [&] { return batch_nested_topk_impl(b, nested, hits, k_stride, counts, total_hits); });
}
int irs_hip_batch_plan(irs_hip_batch* b, void* stream) {
  return settled(b, [&] { return batch_plan_impl(b, stream); });
}
int irs_hip_batch_run(irs_hip_batch* b, void* stream) {
  return settled(b, [&] { return batch_run_impl(b, stream); });
}
int irs_hip_batch_results_to_host(irs_hip_batch* b, void* stream) {
  return settled(b, [&] { return batch_results_to_host_impl(b, stream); });
}
int irs_hip_batch_host_results(irs_hip_batch* b, const irs_hip_hit** hits, uint32_t* k_stride,
                               const uint32_t** counts, const uint64_t** total_hits) {
  return settled(b, [&] { return batch_host_results_impl(b, hits, k_stride, counts, total_hits); });
}
int irs_hip_batch_timings(irs_hip_batch* b, float ms[IRS_HIP_K_COUNT]) {
  return settled(b, [&] { return batch_timings_impl(b, ms); });
}
int irs_hip_batch_reruns(irs_hip_batch* b, uint32_t* count) {
  return settled(b, [&]() -> int {
    if (!b || !count) return IRS_HIP_EINVAL;
    *count = b->reruns + (b->opt ? b->opt->reruns : 0u);   // (optional terms: both passes)
    return IRS_HIP_OK;
  });
}
int irs_hip_batch_work(irs_hip_batch* b, uint64_t* algorithmic_bytes, uint64_t* postings) {
  return settled(b, [&]() -> int {
    if (!b) return IRS_HIP_EINVAL;
    if (algorithmic_bytes) *algorithmic_bytes = b->alg_bytes + b->excl.set_bytes;
    if (postings) *postings = b->postings;
    return IRS_HIP_OK;
  });
}
int irs_hip_batch_results(irs_hip_batch* b, irs_hip_hit* hits, uint32_t k_stride, uint32_t* counts, uint64_t* total_hits) {
  return settled(b, [&] { return batch_results_impl(b, hits, k_stride, counts, total_hits); });
}
int irs_hip_batch_device_results(irs_hip_batch* b, void** d_hits, void** d_counts, uint32_t* k_max) {
  return settled(b, [&] { return batch_device_results_impl(b, d_hits, d_counts, k_max); });
}
int irs_hip_batch_results_to_device(irs_hip_batch* b, void* d_hits, void* d_counts, void* stream) {
  return settled(b, [&] { return batch_results_to_device_impl(b, d_hits, d_counts, stream); });
}
int irs_hip_query_batch(irs_hip_segment* seg, const irs_hip_query* queries, uint32_t nq, const irs_hip_term_scorer* terms, uint32_t n_entries, irs_hip_hit* hits, uint32_t k_stride, uint32_t* counts, uint64_t* total_hits) {
  return guarded([&]() -> int {
    irs_hip_batch* b = nullptr;
    int rc = irs_hip_batch_create(seg, queries, nq, terms, n_entries, &b);
    if (rc != IRS_HIP_OK) return rc;
    rc = irs_hip_batch_run(b, nullptr);
    if (rc == IRS_HIP_OK) rc = irs_hip_batch_results(b, hits, k_stride, counts, total_hits);
    irs_hip_batch_destroy(b);
    return rc;
  });
}
int irs_hip_merge_topk(int32_t device, const void* const* d_lists, const void* const* d_counts, const uint32_t* seg_ids, uint32_t n_lists, uint32_t n_queries, uint32_t k, void* d_out, void* d_out_seg, void* d_out_counts, void* stream) {
  return guarded([&] { return merge_topk_impl(device, d_lists, d_counts, seg_ids, n_lists, n_queries, k, d_out, d_out_seg, d_out_counts, stream); });
}

}  // extern "C"

