// plan_nested.h — host side of irs_hip_batch_nested_sets / _sets_to_device / _topk (nested.h): the
// checks, the child rows (batch_match_sets_impl's device form), the launches, and — for the scored
// form — the groups of units whose lists, scores and candidate keys fit a byte budget, each scored
// by batch_score_docs_impl's device form and selected by k_select.
// Nothing of the batch is kept: every buffer comes from the pool for the call and goes back when the
// stream has run it.  Included by irs_hip.hip (one translation unit).
#pragma once

namespace {

// IRS_HIP_NESTED_SCRATCH_MB, read per call: what the lists, scores and keys of one group of units may
// take together (0: every unit a group of its own).  A unit that exceeds it alone still runs, alone.
static uint64_t nested_budget_bytes() {
  if (const char* e = std::getenv("IRS_HIP_NESTED_SCRATCH_MB")) {
    const long long v = std::atoll(e);
    if (v >= 0) return uint64_t(v) << 20;
  }
  return uint64_t(256) << 20;
}

enum NestedForm { kNestedSetsHost, kNestedSetsDevice, kNestedTopk };

static int nested_check(const irs_hip_batch* b, const irs_hip_nested* d, NestedForm form) {
  if (!b || !d || !d->d_parents) return IRS_HIP_EINVAL;
  if (d->match_min > d->match_max || d->merge > IRS_HIP_MERGE_MIN) return IRS_HIP_EINVAL;
  if (!(d->none_boost >= 0.f) || std::isinf(d->none_boost)) return IRS_HIP_EINVAL;
  uint32_t max_docs = 0;
  for (const irs_hip_segment* sg : b->segs) max_docs = std::max(max_docs, sg->dev.num_docs);
  if (d->n_words == 0 || d->n_words > 0x4000000ull || 64u * d->n_words <= uint64_t(max_docs)) return IRS_HIP_EINVAL;
  // (what irs_hip_batch_match_sets refuses: 16 rows per unit, no clauses and no trees)
  if (b->wide.on() || b->clause.on() || b->tree.on()) return IRS_HIP_EUNSUPPORTED;
  // (what irs_hip_batch_score_docs refuses — {0, 0} asks for no child score)
  const bool none = d->match_min == 0 && d->match_max == 0;
  if (form == kNestedTopk && !none && (b->phrase || b->opt)) return IRS_HIP_EUNSUPPORTED;
  return IRS_HIP_OK;
}

static NestedArgs nested_args(const irs_hip_batch* b, const irs_hip_nested* d, const void* d_child) {
  NestedArgs a{};
  a.segs = b->d_segs.as<DevSegment>();
  a.child = static_cast<const uint64_t*>(d_child);
  a.parents = static_cast<const uint64_t*>(d->d_parents);
  a.n_words = d->n_words;
  a.nq_user = b->nq_user;
  a.match_min = d->match_min;
  a.match_max = d->match_max;
  return a;
}

// The hit parents of every unit, unscored.  Host form: sets / counts are host memory; device form:
// device memory.  The child rows are scratch: the call returns when `st` has run it.
static int batch_nested_sets_impl(irs_hip_batch* b, const irs_hip_nested* d, uint64_t* sets, uint64_t* counts,
                                  void* d_sets, void* d_counts, rt::stream_t st, bool to_device) {
  if (const int rc = nested_check(b, d, to_device ? kNestedSetsDevice : kNestedSetsHost)) return rc;
  const bool want_sets = to_device ? d_sets != nullptr : sets != nullptr;
  const bool want_counts = to_device ? d_counts != nullptr : counts != nullptr;
  if (!want_sets && !want_counts) return IRS_HIP_EINVAL;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  const size_t set_bytes = size_t(b->nq) * d->n_words * 8u, count_bytes = size_t(b->nq) * 8u;
  DevBuf child, own_sets, own_counts;
  if (!child.alloc(set_bytes)) return IRS_HIP_ENOMEM;
  if (!to_device) {
    if ((want_sets && !own_sets.alloc(set_bytes)) || (want_counts && !own_counts.alloc(count_bytes))) return IRS_HIP_ENOMEM;
    d_sets = own_sets.p;
    d_counts = own_counts.p;
  }
  // (queues the segments' records, the masks and k_match_slice / the phrase kernels on `st`)
  if (const int rc = batch_match_sets_impl(b, nullptr, child.p, d->n_words, nullptr, nullptr, st, true)) {
    rt::sync(st);
    return rc;
  }
  RT_LAUNCH(k_nested_match, b->nq, kThreads, 0, st, nested_args(b, d, child.p), static_cast<uint64_t*>(d_sets),
            static_cast<unsigned long long*>(d_counts), static_cast<unsigned long long*>(nullptr));
  bool ok = rt::last_error_ok();
  if (ok && !to_device)
    ok = (!want_sets || rt::d2h(sets, d_sets, set_bytes, st)) && (!want_counts || rt::d2h(counts, d_counts, count_bytes, st));
  const bool synced = rt::sync(st);   // (also after a failure: nothing queued may outlive the blocks)
  return ok && synced ? IRS_HIP_OK : IRS_HIP_EHIP;
}

// The k best hit parents of every unit.  Synchronous.
static int batch_nested_topk_impl(irs_hip_batch* b, const irs_hip_nested* d, irs_hip_hit* hits, uint32_t k_stride,
                                  uint32_t* counts, uint64_t* total_hits) {
  if (const int rc = nested_check(b, d, kNestedTopk)) return rc;
  if ((!hits && !counts && !total_hits) || k_stride < b->k_max) return IRS_HIP_EINVAL;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  rt::stream_t st = nullptr;
  const uint32_t nq = b->nq;
  const size_t set_bytes = size_t(nq) * d->n_words * 8u;
  const bool none = d->match_min == 0 && d->match_max == 0;
  const uint32_t from_zero = d->match_min == 0 && d->match_max == kNestedNoMax ? 1u : 0u;
  DevBuf child, hit, tally;
  if (!child.alloc(set_bytes) || !hit.alloc(set_bytes) || !tally.alloc(size_t(nq) * 16u)) return IRS_HIP_ENOMEM;
  if (const int rc = batch_match_sets_impl(b, nullptr, child.p, d->n_words, nullptr, nullptr, st, true)) {
    rt::sync(st);
    return rc;
  }
  const NestedArgs a = nested_args(b, d, child.p);
  unsigned long long* d_hits = tally.as<unsigned long long>();
  RT_LAUNCH(k_nested_match, nq, kThreads, 0, st, a, hit.as<uint64_t>(), d_hits, d_hits + nq);
  std::vector<uint64_t> tallies(size_t(nq) * 2u);   // [0, nq): hit parents; [nq, 2 nq): the children under them
  if (!rt::last_error_ok() || !rt::d2h(tallies.data(), tally.p, size_t(nq) * 16u, st) || !rt::sync(st)) {
    rt::sync(st);
    return IRS_HIP_EHIP;
  }
  if (total_hits) std::copy(tallies.begin(), tallies.begin() + nq, total_hits);
  if (counts) std::fill(counts, counts + nq, 0u);
  if (!hits && !counts) return IRS_HIP_OK;

  uint32_t sort_cap = 64;
  while (sort_cap < b->k_max) sort_cap <<= 1;
  const uint64_t budget = nested_budget_bytes();
  constexpr uint64_t kMost = 0x7FFFFFFFull;   // list entries / hits / keys of one group
  std::vector<uint64_t> offsets(size_t(nq) + 1u);
  std::vector<uint32_t> hoff, cand_count;
  std::vector<DevQuery> qs;
  std::vector<Hit> out;
  std::vector<uint32_t> out_count;
  DevBuf d_docs, d_scores, d_pdoc, d_ends, d_keys, d_tables, d_out;
  int rc = IRS_HIP_OK;
  for (uint32_t u0 = 0; u0 < nq && rc == IRS_HIP_OK;) {
    // the group: units [u0, u1) while lists, scores, hit records and the keys' [units][cap] fit
    uint32_t u1 = u0;
    uint64_t n_list = 0, n_hit = 0, cap = 0;
    while (u1 < nq) {
      const uint64_t h = tallies[u1], l = none ? 0u : tallies[nq + u1];
      const uint64_t cap2 = std::max(cap, h), keys2 = uint64_t(u1 - u0 + 1u) * cap2;
      const bool fits = (n_list + l) * 8u + (n_hit + h) * 8u + keys2 * 8u <= budget && n_list + l <= kMost &&
                        n_hit + h <= kMost && keys2 <= kMost;
      if (u1 > u0 && !fits) break;
      n_list += l;
      n_hit += h;
      cap = cap2;
      ++u1;
    }
    const uint32_t gu = u1 - u0;
    if (n_list > kMost || n_hit > kMost) {   // (a single unit beyond what one score-docs call takes)
      rc = IRS_HIP_EUNSUPPORTED;
      break;
    }
    if (n_hit == 0) {   // no unit of the group has a hit
      u0 = u1;
      continue;
    }
    // the tables of the group: offsets of every unit's list (units outside the group: empty lists),
    // the hits' offsets, k_select's records
    uint64_t at = 0;
    hoff.assign(gu + 1u, 0u);
    cand_count.assign(gu, 0u);
    qs.assign(gu, DevQuery{});
    for (uint32_t u = 0; u <= nq; ++u) {
      offsets[u] = at;
      if (u >= u0 && u < u1 && !none) at += tallies[nq + u];
    }
    for (uint32_t g = 0; g < gu; ++g) {
      hoff[g + 1u] = hoff[g] + uint32_t(tallies[u0 + g]);
      cand_count[g] = uint32_t(tallies[u0 + g]);
      qs[g].k = b->queries[u0 + g].k;
    }
    // one block: offsets | hoff | cand_count | queries | zeros (k_select's hits and pruned) | status | out counts
    const size_t off_b = (size_t(nq) + 1u) * 8u, hoff_b = (size_t(gu) + 1u) * 4u, cc_b = size_t(gu) * 4u;
    auto up8 = [](size_t n) { return (n + 7u) & ~size_t(7); };
    const size_t at_hoff = off_b, at_cc = at_hoff + up8(hoff_b), at_q = at_cc + up8(cc_b),
                 at_zero = at_q + size_t(gu) * sizeof(DevQuery), at_status = at_zero + size_t(gu) * 8u,
                 at_oc = at_status + 8u, table_b = at_oc + up8(cc_b);
    const size_t out_b = size_t(gu) * b->k_max * sizeof(Hit);
    if (!d_tables.alloc(table_b) || !d_out.alloc(out_b) || !d_pdoc.alloc(n_hit * 4u) || !d_ends.alloc(n_hit * 4u) ||
        !d_keys.alloc(size_t(gu) * cap * 8u) || (n_list && (!d_docs.alloc(n_list * 4u) || !d_scores.alloc(n_list * 4u)))) {
      rc = IRS_HIP_ENOMEM;
      break;
    }
    uint8_t* T = d_tables.as<uint8_t>();
    bool ok = rt::dmemset(T + at_zero, 0, table_b - at_zero, st) && rt::h2d(T, offsets.data(), off_b, st) &&
              rt::h2d(T + at_hoff, hoff.data(), hoff_b, st) && rt::h2d(T + at_cc, cand_count.data(), cc_b, st) &&
              rt::h2d(T + at_q, qs.data(), size_t(gu) * sizeof(DevQuery), st);
    const uint64_t* d_offsets = reinterpret_cast<const uint64_t*>(T);
    const uint32_t* d_hoff = reinterpret_cast<const uint32_t*>(T + at_hoff);
    if (ok) {
      RT_LAUNCH(k_nested_list, gu, kThreads, 0, st, a, hit.as<uint64_t>(), u0, d_offsets, d_hoff,
                d_docs.as<uint32_t>(), d_pdoc.as<uint32_t>(), d_ends.as<uint32_t>());
      ok = rt::last_error_ok();
    }
    if (ok && n_list) {
      rc = batch_score_docs_impl(b, nullptr, nullptr, nullptr, nullptr, d_docs.p, d_offsets, n_list, d_scores.p,
                                 nullptr, st, true);
      ok = rc == IRS_HIP_OK;
    }
    if (ok) {
      RT_LAUNCH(k_nested_merge, uint32_t((n_hit + kThreads - 1u) / kThreads), kThreads, 0, st, d_hoff, gu,
                uint32_t(n_hit), u0, d_offsets, d_pdoc.as<uint32_t>(), d_ends.as<uint32_t>(),
                n_list ? d_scores.as<float>() : static_cast<const float*>(nullptr), d->merge, from_zero,
                none ? d->none_boost : 0.f, d_keys.as<uint64_t>(), uint32_t(cap));
      ok = rt::last_error_ok();
    }
    if (ok) {
      // (no bstar, no caller thresholds, no groups; hits and pruned all zero: never an underflow)
      const uint32_t stage_cap = uint32_t(std::min<uint64_t>(cap, kSelectStage));
      const size_t smem = size_t(sort_cap + stage_cap) * sizeof(uint64_t);
      ok = big_smem(k_select, smem);
      if (ok) {
        RT_LAUNCH(k_select, gu, kThreads, smem, st, reinterpret_cast<const DevQuery*>(T + at_q), d_keys.as<uint64_t>(),
                  uint32_t(cap), reinterpret_cast<const uint32_t*>(T + at_cc),
                  reinterpret_cast<const unsigned long long*>(T + at_zero), d_out.as<Hit>(), b->k_max,
                  reinterpret_cast<uint32_t*>(T + at_oc), reinterpret_cast<uint32_t*>(T + at_status), stage_cap, sort_cap,
                  static_cast<const uint32_t*>(nullptr), static_cast<const uint32_t*>(nullptr),
                  reinterpret_cast<const uint32_t*>(T + at_zero), static_cast<const float*>(nullptr),
                  static_cast<const uint32_t*>(nullptr));
        ok = rt::last_error_ok();
      }
    }
    out.resize(size_t(gu) * b->k_max);
    out_count.assign(gu, 0u);
    ok = ok && rt::d2h(out.data(), d_out.p, out_b, st) && rt::d2h(out_count.data(), T + at_oc, cc_b, st);
    const bool synced = rt::sync(st);   // (also after a failure: nothing queued may outlive the blocks)
    if (rc == IRS_HIP_OK && !(ok && synced)) rc = IRS_HIP_EHIP;
    if (rc != IRS_HIP_OK) break;
    for (uint32_t g = 0; g < gu; ++g) {
      if (counts) counts[u0 + g] = out_count[g];
      for (uint32_t i = 0; hits && i < out_count[g]; ++i) {
        const Hit& h = out[size_t(g) * b->k_max + i];
        hits[size_t(u0 + g) * k_stride + i].score = h.score;
        hits[size_t(u0 + g) * k_stride + i].doc = h.doc;
      }
    }
    u0 = u1;
  }
  return rc;
}

}  // namespace
