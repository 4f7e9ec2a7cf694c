// run.h — the host half of a batch's run, in named stages: what a run gets behind (batch.h), its
// uploads and fills, the plan stage (also queued ahead: irs_hip_batch_plan), pilot, score — where a
// run may move to the device's tail stream —, select, the term pass of a batch with optional terms,
// and the run's end.  run_impl, last in this file, is their sequence.
// Included by irs_hip.hip (one translation unit).
#pragma once

namespace {

int run_impl(irs_hip_batch* b, rt::stream_t st);

// irs_hip_batch_profile: the events around every stage of a run, on the stream the stage's end is on
static bool run_mark(irs_hip_batch* b, int i, rt::stream_t st) {
  return !b->profile || b->sync.prof[i].record(st);
}
static bool tile_units_on(const irs_hip_batch* b) { return !b->phrase && !b->tiles.units.empty(); }

// The caller's min scores as score bins, in the scale the units bin with NOW: ensure_scratch may
// have re-scaled a unit (build_groups: one bound for a query on every rank), so this runs behind it.
static bool stage_min_bins(irs_hip_batch* b) {
  if (!b->has_min || !b->min_dirty) return true;
  std::vector<uint32_t> bins(b->nq, 0u);
  for (uint32_t u = 0; u < b->nq; ++u) {
    // the bin score_bin() puts a score of m into: docs at or above m land in it or higher
    const float x = std::fmin(b->min_scores[u] * b->queries[u].bin_scale, float(kBins - 1));
    bins[u] = uint32_t(x);
  }
  if (!b->up.copy(b->d_min_bin.p, bins.data(), bins.size() * 4) ||
      !b->up.copy(b->d_min_score.p, b->min_scores.data(), b->min_scores.size() * 4))
    return false;
  b->min_dirty = false;
  return true;
}

// The planning stage of a run: tile -> first block tables, per-term records, the work items of
// the tile kernels.  A pure function of (batch, segments): it touches nothing a run of ANOTHER
// batch reads, so a caller may queue it ahead on a second stream (irs_hip_batch_plan).
static bool plan_stage(irs_hip_batch* b, rt::stream_t st) {
  bool ok = run_mark(b, 2 * IRS_HIP_K_PLAN, st);
  // the doc masks of the units with excluded terms (excl.h), before anything reads them
  if (ok && b->excl.on()) ok = launch_excl_masks(b, st);
  // (a joined batch without conjunctions needs none of k_plan's tables)
  if (ok && (b->phrase || !b->tiles.units.empty() || !b->blocks.units.empty() || !b->any.units.empty())) {
    RT_LAUNCH(k_plan, b->nq * b->jt, kThreads, 0, st, b->d_segs.as<DevSegment>(),
              b->d_queries.as<DevQuery>(), b->d_qterms.as<DevQTerm>(), b->jt, b->tiles.docs,
              b->d_first.as<uint32_t>(), b->d_tails.as<DevTail>());
    ok = rt::last_error_ok();
  }
  if (ok && streams_on(b)) ok = launch_join(b, st);
  if (ok && tile_units_on(b)) ok = launch_items(b, st);
  return ok && run_mark(b, 2 * IRS_HIP_K_PLAN + 1, st);
}

static int batch_plan_impl(irs_hip_batch* b, void* stream) {
  if (!b) return IRS_HIP_EINVAL;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  if (!ensure_scratch(b) || !stage_min_bins(b)) return IRS_HIP_ENOMEM;
  rt::stream_t st = static_cast<rt::stream_t>(stream);
  const bool ok = plan_get_behind(b, st) && b->up.flush(st) && plan_stage(b, st) && b->sync.plan.mark(st);
  if (!ok) abandon_fills(b);
  b->sync.planned = ok;
  return ok ? IRS_HIP_OK : IRS_HIP_EHIP;
}

// The union of the two passes of a batch with optional terms (k_union_topk, phrase.h) into
// d_union_*: behind both passes' k_select on `st`.
static bool launch_union(irs_hip_batch* b, rt::stream_t st) {
  const irs_hip_batch* c = b->opt;
  RT_LAUNCH(k_union_topk, b->nq, kThreads, 0, st, b->d_queries.as<DevQuery>(), b->k_max,
            b->d_out.as<Hit>(), b->d_out_count.as<uint32_t>(), b->d_hits.as<unsigned long long>(),
            c->d_out.as<Hit>(), c->d_out_count.as<uint32_t>(), c->d_hits.as<unsigned long long>(),
            b->d_union_out.as<Hit>(), b->d_union_count.as<uint32_t>(),
            b->d_union_hits.as<unsigned long long>());
  return rt::last_error_ok();
}
// What the result calls hand out: the batch's own tables, or the union of its two passes
static void* out_hits(irs_hip_batch* b) { return b->opt ? b->d_union_out.p : b->d_out.p; }
static void* out_counts(irs_hip_batch* b) { return b->opt ? b->d_union_count.p : b->d_out_count.p; }
static void* out_totals(irs_hip_batch* b) { return b->opt ? b->d_union_hits.p : b->d_hits.p; }

// The batch's tables (built in page-locked memory since create) go out: before the batch's first
// run on the device's copy stream `up_st` (nothing on the GPU reads or writes these buffers yet),
// afterwards in the run's own stream order (a running kernel may still read what they replace).
// Then what every run starts from zero.
static bool run_uploads_and_fills(irs_hip_batch* b, rt::stream_t st, rt::stream_t up_st) {
  // (a counting run of a batch with doc sets: the lead pieces' tallies, irs_hip_batch_doc_set_stats)
  b->excl.leads_counted = b->count_touched && b->excl.sets_on();
  bool ok = up_st ? b->up.flush(up_st) && b->sync.uploaded.record(up_st) && b->sync.uploaded.wait(st)
                  : b->up.flush(st);
  if (ok && streams_on(b) && !b->join.slack_zeroed) {
    // (the slack behind the last stream is only ever read by masked-off look-ahead: zero it once)
    ok = rt::dmemset(b->join.d_entries.as<uint32_t>() + b->join.entries, 0, kJoinSlack * 4, st);
    b->join.slack_zeroed = ok;
  }
  ok = ok && rt::dmemset(b->d_zeroed.p, 0, b->d_zeroed.n, st);   // (ensure_scratch: six tables)
  // (optional terms: no doc is taken until k_phrase_or matches it)
  if (b->opt) ok = ok && rt::dmemset(b->d_taken.p, 0, b->d_taken.n, st);
  if (ok && b->excl.leads_counted)
    ok = (b->excl.d_leads.p || b->excl.d_leads.alloc(16)) && rt::dmemset(b->excl.d_leads.p, 0, 16, st);
  // (streams out of the device's cache that another stream is still filling)
  if (streams_on(b)) ok = ok && wait_for_streams(b, st);
  return ok;
}

// 1. plan: queued ahead by irs_hip_batch_plan — `st` is behind it since run_get_behind, and asks
// once more — or made here.  Either way no later run waits for `plan` again: `st` is behind it,
// and whatever touches the tables later gets behind this run's `done`.
static bool run_plan(irs_hip_batch* b, rt::stream_t st) {
  const bool ahead = b->sync.planned;
  b->sync.planned = false;
  const bool ok = ahead ? b->sync.plan.wait(st) : plan_stage(b, st);
  b->sync.plan.settle();
  return ok;
}

// 2. pilot: per-query score-bin threshold (phrase batches have none: few docs match)
static bool run_pilot(irs_hip_batch* b, rt::stream_t st) {
  bool ok = run_mark(b, 2 * IRS_HIP_K_PILOT, st);
  if (b->groups.n) ok = ok && rt::dmemset(b->groups.d_hist.p, 0, b->groups.d_hist.n, st);
  if (b->join.on()) ok = ok && launch_join_pilot(b, st);
  if (b->wide.on()) ok = ok && launch_wide_pilot(b, st);
  if (b->clause.on()) ok = ok && launch_clause_pilot(b, st);
  if (b->tree.on()) ok = ok && launch_tree_pilot(b, st);
  ok = ok && launch_group_threshold(b, st);
  if (tile_units_on(b))
    ok = ok && with_tile_kernel(b, [&](auto k) { return launch_pilot(b, st, k); });
  return ok && run_mark(b, 2 * IRS_HIP_K_PILOT + 1, st);
}

// Where a run ends: on the caller's stream, or — `tail` — on the device's tail stream
struct RunEnd {
  rt::stream_t ts;
  bool tail;
};

// 3. score every tile / every lead block — behind the tail queued last on the device (pool.h):
// a started k_join_score workgroup holds the LDS that tail's k_select asks for.
// A batch that passes tail_ok: from behind its paired launch on, the run is queued on the device's
// tail stream `end->ts`, and nothing of it follows on `st`; `tail_lock` (the device's Tail::m,
// run_impl's) is taken and spans everything the run queues from here on.
static bool run_score(irs_hip_batch* b, rt::stream_t st, std::unique_lock<std::mutex>& tail_lock, RunEnd* end) {
  if (!wait_for_tail(b->seg->device, st) || !run_mark(b, 2 * IRS_HIP_K_SCORE, st)) return false;
  if (tail_ok(b)) {
    rt::stream_t s = tail_stream(b->seg->device, &end->tail);
    if (end->tail) end->ts = s;
  }
  if (end->tail) tail_lock.lock();
  const bool simd = b->seg->dev.layout == kSimd4;
  bool ok = true;
  if (b->phrase)
    ok = simd ? launch_phrase_terms<kSimd4>(b, st) : launch_phrase_terms<kScalar>(b, st);
  else if (tile_units_on(b))
    ok = with_tile_kernel(b, [&](auto k) { return launch_score(b, st, k); });
  if (b->join.on()) ok = ok && launch_join_score(b, st, end->tail ? &end->ts : nullptr);
  if (b->wide.on()) ok = ok && launch_wide_score(b, st);
  if (b->clause.on()) ok = ok && launch_clause_score(b, st);
  if (b->tree.on()) ok = ok && launch_tree_score(b, st);
  if (!b->phrase) ok = ok && (simd ? launch_conj<kSimd4>(b, st) : launch_conj<kScalar>(b, st));
  if (!b->phrase) ok = ok && (simd ? launch_any<kSimd4>(b, st) : launch_any<kScalar>(b, st));
  return ok && run_mark(b, 2 * IRS_HIP_K_SCORE + 1, end->ts);
}

// ... the group sums behind k_select (a batch with groups never takes the tail: `st`), summed over
// the communicator's ranks, and the groups' verdict
static bool run_group_sums(irs_hip_batch* b, rt::stream_t st) {
  RT_LAUNCH(k_group_sums, (b->groups.n + 63u) / 64u, 64, 0, st, b->d_queries.as<DevQuery>(),
            b->groups.d_members.as<uint32_t>(), uint32_t(b->segs.size()), b->groups.n,
            b->d_out_count.as<uint32_t>(), b->d_hits.as<unsigned long long>(),
            b->d_bstar.as<uint32_t>(), min_bins(b), b->d_status.as<uint32_t>(),
            b->groups.d_sums.as<uint32_t>());
  bool ok = rt::last_error_ok();
  if (ok && b->comm && !b->phrase)
    ok = rt::comm::all_reduce_u32(b->comm->h, b->groups.d_sums.p,
                                  size_t(b->groups.n) * kGroupSumWords + 2, st);
  if (ok)
    RT_LAUNCH(k_group_verdict, (b->groups.n + 63u) / 64u, 64, 0, st, b->d_queries.as<DevQuery>(),
              b->groups.n, b->groups.d_sums.as<uint32_t>(), b->d_status.as<uint32_t>());
  return ok;
}

// 4. exact top-k, on the stream the run ends on
static bool run_select(irs_hip_batch* b, rt::stream_t st, rt::stream_t ts) {
  if (!run_mark(b, 2 * IRS_HIP_K_SELECT, ts)) return false;
  uint32_t sort_cap = 64;
  while (sort_cap < b->k_max) sort_cap <<= 1;
  const uint32_t stage_cap = std::min<uint32_t>(b->cand_cap, kSelectStage);
  const size_t smem = size_t(sort_cap + stage_cap) * sizeof(uint64_t);
  if (!big_smem(k_select, smem)) return false;
  RT_LAUNCH(k_select, b->nq, kThreads, smem, ts, b->d_queries.as<DevQuery>(),
            b->d_cands.as<uint64_t>(), b->cand_cap, b->d_cand_count.as<uint32_t>(),
            b->d_hits.as<unsigned long long>(), b->d_out.as<Hit>(), b->k_max,
            b->d_out_count.as<uint32_t>(), b->d_status.as<uint32_t>(), stage_cap, sort_cap,
            b->d_bstar.as<uint32_t>(), min_bins(b), b->d_pruned.as<uint32_t>(),
            b->has_min ? b->d_min_score.as<float>() : static_cast<const float*>(nullptr),
            b->groups.n ? b->groups.d_of.as<uint32_t>() : static_cast<const uint32_t*>(nullptr));
  if (b->groups.n && !run_group_sums(b, st)) return false;
  return rt::last_error_ok() && run_mark(b, 2 * IRS_HIP_K_SELECT + 1, ts);
}

// Optional terms: the term pass behind the phrase pass, on the same stream, then the union of
// their results (the batch's `done` covers all three).  What the term pass returned, if it failed.
static int run_term_pass_and_union(irs_hip_batch* b, rt::stream_t st) {
  const uint64_t n32 = b->d_taken.n / 4u;   // (taken -> the term pass's doc sets)
  RT_LAUNCH(k_not_words, uint32_t((n32 + kThreads - 1) / kThreads), kThreads, 0, st, b->d_taken.as<uint32_t>(), n32);
  if (!rt::last_error_ok()) return IRS_HIP_EHIP;
  if (const int rc = run_impl(b->opt, st)) return rc;
  return launch_union(b, st) ? IRS_HIP_OK : IRS_HIP_EHIP;
}

// The end of a run, `ok` or not: the status word follows the kernels into page-locked memory and
// `done` marks this run, both on the stream the run ends on; whatever of a tail got queued, the next
// score launch of the device waits for it (Tail::done).
static bool run_finish(irs_hip_batch* b, const RunEnd& end, bool ok) {
  if (ok && !b->sync.h_status.p) ok = b->sync.h_status.alloc(64);
  ok = ok && rt::d2h(b->sync.h_status.p, b->d_status.p, 4, end.ts) && b->sync.done.mark(end.ts);
  if (end.tail && !tail_of(b->seg->device).done.mark(end.ts)) ok = false;
  b->sync.tail_used = end.tail;
  if (!ok) abandon_fills(b);
  b->ran = true;
  return ok;
}

int run_impl(irs_hip_batch* b, rt::stream_t st) {
  HostTrace trace("batch_run (scratch + uploads + launches queued)");
  if (!ensure_scratch(b) || !stage_min_bins(b)) return IRS_HIP_ENOMEM;
  b->stream = st;
  rt::stream_t up_st = nullptr;
  if (!run_get_behind(b, st, &up_st)) return IRS_HIP_EHIP;
  // (the device's tail mutex: run_score takes it with the tail stream, and it is held until this
  // function returns — across everything the run queues from there on)
  std::unique_lock<std::mutex> tail_lock(tail_of(b->seg->device).m, std::defer_lock);
  RunEnd end{st, false};
  int rc = IRS_HIP_OK;
  bool ok = run_uploads_and_fills(b, st, up_st) && run_plan(b, st) && run_pilot(b, st) &&
            run_score(b, st, tail_lock, &end) && run_select(b, st, end.ts);
  if (ok && b->opt) {
    rc = run_term_pass_and_union(b, st);
    ok = rc == IRS_HIP_OK;
  }
  if (!ok) b->sync.planned = false;   // (a stage that did not get as far as run_plan)
  ok = run_finish(b, end, ok);
  return rc != IRS_HIP_OK ? rc : ok ? IRS_HIP_OK : IRS_HIP_EHIP;
}

}  // namespace
