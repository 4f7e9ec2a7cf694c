// plan_score_docs.h — host side of irs_hip_batch_score_docs (score_docs.h): the units' records and
// rows, built from the batch's query records the first time the call is made, the checks of the
// caller's lists (score_docs_shape.h) and the launch.
// Included by irs_hip.hip (one translation unit).
#pragma once

namespace {

// SdUnit records and rows of every unit, from what create left in b->queries / b->qterms: the rows
// as they are (term ordinal, scorer values, pad0: a clause unit's need-mask, a tree unit's leaf),
// a grouped conjunction's groups from AnyWork::opens, a tree unit's records from TreeWork::nodes
static int build_score_docs_work(irs_hip_batch* b) {
  ScoreDocsWork& s = b->score_docs;
  if (s.built) return IRS_HIP_OK;
  std::vector<uint8_t> grouped(b->nq, 0);
  for (uint32_t u : b->any.units) grouped[u] = 1;
  std::vector<uint32_t> tree_at(b->nq, 0);
  for (size_t i = 0; i < b->tree.units.size(); ++i) tree_at[b->tree.units[i]] = uint32_t(i * kTreeMaxNodes);
  s.units.clear();
  s.seg_docs.clear();
  for (const irs_hip_segment* sg : b->segs) s.seg_docs.push_back(sg->dev.num_docs);
  for (uint32_t q = 0; q < b->nq; ++q) {
    const DevQuery& dq = b->queries[q];
    if (dq.n_terms > kMaxTerms) return IRS_HIP_EUNSUPPORTED;
    SdUnit u{};
    u.dead = dq.dead;
    u.seg = dq.seg;
    u.first = dq.first_term;
    u.op = dq.op;
    u.n_rows = dq.n_terms;
    u.opens = grouped[q] ? b->any.opens[q] : (1u << dq.n_terms) - 1u;
    u.nodes = tree_at[q];
    s.units.push_back(u);
  }
  const size_t row_bytes = std::max<size_t>(b->qterms.size(), 1) * sizeof(DevQTerm);
  const size_t node_bytes = std::max<size_t>(b->tree.nodes.size(), 1) * sizeof(TreeNode);
  if (!s.d_units.alloc(s.units.size() * sizeof(SdUnit)) || !s.d_rows.alloc(row_bytes) || !s.d_nodes.alloc(node_bytes))
    return IRS_HIP_ENOMEM;
  s.built = true;
  s.sent = false;
  return IRS_HIP_OK;
}

// irs_hip_batch_score_docs (docs / offsets / scores / matched: host memory, synchronous) and
// _to_device (device memory, queued on `st`).  Reads the segments, the batch's exclusion masks
// (rebuilt here, as match sets do) and tables of its own — nothing a run leaves behind, nothing a
// run reads is changed.
static int batch_score_docs_impl(irs_hip_batch* b, const uint32_t* docs, const uint64_t* offsets, float* scores,
                                 uint8_t* matched, const void* d_docs, const void* d_offsets, uint64_t n_docs,
                                 void* d_scores, void* d_matched, rt::stream_t st, bool to_device) {
  if (!b) return IRS_HIP_EINVAL;
  if (to_device ? (!d_docs || !d_offsets || !d_scores) : (!docs || !offsets || !scores)) return IRS_HIP_EINVAL;
  // (phrase units run on lead items of their own, wide units have more rows than a presence word)
  if (b->phrase || b->opt || b->wide.on()) return IRS_HIP_EUNSUPPORTED;
  if (!rt::set_device(b->seg->device)) return IRS_HIP_EHIP;
  if (const int rc = build_score_docs_work(b)) return rc;
  ScoreDocsWork& s = b->score_docs;
  std::vector<ScoreDocsChunk> chunks;
  if (to_device) {
    if (n_docs > kScoreDocsMax) return IRS_HIP_EUNSUPPORTED;
  } else {
    if (const int rc = score_docs_offsets(offsets, b->nq, &n_docs)) return rc;
    if (const int rc = score_docs_lists(docs, offsets, b->nq, b->nq_user, s.seg_docs.data())) return rc;
    score_docs_cut(offsets, b->nq, chunks);
  }
  const uint64_t waves = to_device ? score_docs_grid(n_docs, b->nq) : chunks.size();
  if (n_docs == 0) return IRS_HIP_OK;   // every list is empty: nothing to write
  auto release = [&] {   // (sized by the call: back to the pool, not kept for the batch's life)
    s.d_docs.release();
    s.d_chunks.release();
    s.d_scores.release();
    s.d_matched.release();
  };
  if (!to_device) {
    if (!s.d_docs.alloc(n_docs * 4u) || !s.d_chunks.alloc(chunks.size() * sizeof(ScoreDocsChunk)) ||
        !s.d_scores.alloc(n_docs * 4u) || (matched && !s.d_matched.alloc(n_docs))) {
      release();   // (nothing is queued yet: the blocks that did come go back at once)
      return IRS_HIP_ENOMEM;
    }
  }
  // behind the batch's own queued work, as match sets are: a run or a plan stage writes the masks, an
  // earlier call on another stream reads this one's tables
  bool ok = match_get_behind(b, st) && b->up.flush(st);   // (the segments' records and the masks' tables, staged since create)
  if (ok && !s.sent) {
    ok = rt::h2d(s.d_units.p, s.units.data(), s.units.size() * sizeof(SdUnit), st) &&
         (b->qterms.empty() || rt::h2d(s.d_rows.p, b->qterms.data(), b->qterms.size() * sizeof(DevQTerm), st)) &&
         (b->tree.nodes.empty() || rt::h2d(s.d_nodes.p, b->tree.nodes.data(), b->tree.nodes.size() * sizeof(TreeNode), st));
    s.sent = ok;
  }
  if (ok && b->excl.on()) ok = launch_excl_masks(b, st);
  SdArgs a{};
  a.segs = b->d_segs.as<DevSegment>();
  a.units = s.d_units.as<SdUnit>();
  a.rows = s.d_rows.as<DevQTerm>();
  a.nodes = s.d_nodes.as<TreeNode>();
  a.n_units = b->nq;
  a.n_chunks = uint32_t(waves);
  a.n_docs = uint32_t(n_docs);
  if (to_device) {
    a.offsets = static_cast<const uint64_t*>(d_offsets);
    a.docs = static_cast<const uint32_t*>(d_docs);
    a.scores = static_cast<float*>(d_scores);
    a.matched = static_cast<uint8_t*>(d_matched);
  } else {
    ok = ok && rt::h2d(s.d_docs.p, docs, n_docs * 4u, st) &&
         rt::h2d(s.d_chunks.p, chunks.data(), chunks.size() * sizeof(ScoreDocsChunk), st);
    a.chunks = s.d_chunks.as<ScoreDocsChunk>();
    a.docs = s.d_docs.as<uint32_t>();
    a.scores = s.d_scores.as<float>();
    a.matched = matched ? s.d_matched.as<uint8_t>() : nullptr;
  }
  if (ok) {
    const uint32_t grid = uint32_t((waves + kSdWaves - 1u) / kSdWaves);
    ok = with_layout(b->seg->dev.layout, [&](auto L) {
      RT_LAUNCH((k_score_docs<decltype(L)::value>), grid, kSdWaves * 64, 0, st, a);
      return rt::last_error_ok();
    });
  }
  if (to_device) {
    // (a later run, setter or destroy gets behind this: the masks and the tables are still read)
    if (!ok) return IRS_HIP_EHIP;
    return b->sync.docs_scored.mark(st) ? IRS_HIP_OK : IRS_HIP_EHIP;
  }
  const bool copied = ok && rt::d2h(scores, s.d_scores.p, n_docs * 4u, st) &&
                      (!matched || rt::d2h(matched, s.d_matched.p, n_docs, st));
  const bool synced = rt::sync(st);   // (also after a failure: nothing queued may outlive the blocks)
  release();
  return copied && synced ? IRS_HIP_OK : IRS_HIP_EHIP;
}

}  // namespace
