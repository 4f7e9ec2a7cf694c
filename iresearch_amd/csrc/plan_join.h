// plan_join.h — host half of the units on joined posting streams (join.h): which units join, the
// batch's distinct streams and k_join's work list, the shared-threshold groups, the k_join /
// k_join_pilot / k_join_score launches.  Included by irs_hip.hip (one translation unit).
#pragma once

namespace {

// Can the batch's doc-tile units run as joined streams?  (Anything else keeps score.h's work
// items: per-doc match counters, Max / Min merged scores, scorers outside the table family,
// 64-bit accumulators, a frequency that does not fit an entry.)
bool join_allowed(const irs_hip_batch* b) {   // batch level
  if (b->path_pref == IRS_HIP_PATH_ITEMS) return false;
  if (b->knobs.join_off && b->path_pref != IRS_HIP_PATH_JOINED) return false;   // tuning / test knob
  // (a unit on joined streams runs exhaustively under ExecutionContext::wand: the top k is the
  // exhaustive one by construction; pruning stays with the block-driven / work-item kernels)
  return !b->phrase && b->acc32;
}
// Conjunction as joined streams or block driven?  Measured on 10 M docs (tools/sweep.py --op and,
// GPU time summed over the chip, picoseconds): joined = 4200 per doc tile of the unit (barriers,
// epilogue: the part that does not depend on the postings) + 1.5 per posting of its terms
// (k_join_score 0.3 + a share of k_join's decode); block driven = 2300 + 400 x terms per
// 128-posting block of the rarest term: its decode plus a seek and a block decode in every other
// term.  The conjunctions of two frequent terms are the ones that join.
// (With the device's stream cache — stream_cache.h — a stream that is already held costs no
// k_join at all: these coefficients, join_or_pays' 2.9 per distinct posting and join_half_ok's
// sizes price every batch as a cold one and so UNDER-state the joined path.  They are kept: AUTO
// joins wherever it did before and nowhere earlier, as §3.13 kept them for paired tiles — what a
// warm cache would let join in addition has not been measured.)
// Returns the picoseconds saved by joining (<= 0: block driven is cheaper).
int64_t join_and_saving(const irs_hip_batch* b, const DevQuery& dq) {
  const irs_hip_segment* sg = b->segs[dq.seg];
  uint64_t sum = 0, lead = ~0ull;
  for (uint32_t j = 0; j < dq.n_terms; ++j) {
    const uint64_t df = sg->terms[b->qterms[dq.first_term + j].term].docs_count;
    sum += df;
    lead = std::min(lead, df);
  }
  const uint64_t tiles = sg->dev.num_docs / kJoinTile + 1;
  const uint64_t lead_blocks = lead / kBlock + 1;
  return int64_t(lead_blocks * (2300ull + 400ull * dq.n_terms)) -
         int64_t(4200ull * tiles + (3ull * sum) / 2);
}
// ... and the launches of the joined kernels themselves (k_join, the pilot, one more score
// kernel) only pay when the conjunctions that would join save more than that together
constexpr int64_t kJoinAndLaunchCost = 500000000;   // 0.5 ms
int join_and_forced(const irs_hip_batch* b) {   // -1: decide by cost
  if (b->path_pref == IRS_HIP_PATH_JOINED) return 1;   // (forced: wherever it is possible)
  return b->knobs.join_and;   // tuning / test knob (-1: not set)
}
// Plain disjunctions as joined streams or as work items?  Measured on one MI355X, BM25, 10 M docs
// (tools/cost_sweep.py, profiles/r04_sweeps.txt; picoseconds of step time):
//   joined:     2.9 per posting of every DISTINCT stream (k_join: decode + 4 B written)
//             + 0.47 per posting a query references + 3800 per (unit, doc tile)
//   work items: 1.14 per referenced posting + 6200 per (unit, doc tile)
// A stream pays for itself when it is shared (the headline batch: 5.7 G referenced postings on
// 0.31 G distinct ones) or when there are many units (the per-tile cost is lower): joining wins
// iff  2.9 D < 0.67 R + 2400 T.  128 queries x 8 terms without one shared term: 1.51 ms as work
// items against 1.60 joined; on a corpus of 1000-word docs 0.75 against 1.35.
bool join_or_pays(const irs_hip_batch* b, const std::vector<uint32_t>& units) {
  if (units.empty()) return false;
  uint64_t refs = 0, distinct = 0, tiles = 0;
  std::vector<std::vector<uint8_t>> seen(b->segs.size());
  for (uint32_t u : units) {
    const DevQuery& dq = b->queries[u];
    const irs_hip_segment* sg = b->segs[dq.seg];
    tiles += sg->dev.num_docs / kJoinTile + 1;
    if (seen[dq.seg].empty()) seen[dq.seg].assign(sg->dev.num_terms, 0);
    for (uint32_t j = 0; j < dq.n_terms; ++j) {
      const uint32_t term = b->qterms[dq.first_term + j].term;
      const uint64_t df = sg->terms[term].docs_count;
      refs += df;
      if (!seen[dq.seg][term]) {
        seen[dq.seg][term] = 1;
        distinct += df;
      }
    }
  }
  return 29ull * distinct < (67ull * refs) / 10ull + 24000ull * tiles;
}
int join_or_forced(const irs_hip_batch* b) {   // -1: decide by cost
  if (b->path_pref == IRS_HIP_PATH_JOINED) return 1;
  return b->knobs.join_or;   // tuning / test knob (-1: not set)
}
bool unit_counts_matches(const DevQuery& dq) {   // min-match / the kMin disjunction of two
  return query_run(dq.op) == kRunCount || query_min_both(dq.op);
}
bool unit_joinable(const irs_hip_batch* b, uint32_t u) {
  const DevQuery& dq = b->queries[u];
  if (query_min_both(dq.op) || query_merge(dq.op) != kScoreSum) return false;
  // a unit with excluded terms: k_join applies the SEGMENT's deleted docs while it decodes the
  // streams every unit shares, the unit's own mask (excl.h) cannot ride there
  if (dq.dead != b->segs[dq.seg]->dev.dead) return false;
  if (query_run(dq.op) != kRunTiles) {
    // min-match / conjunction: the match count rides in the accumulator's low bits (join.h
    // COUNT) where that costs no precision that matters
    if (!dq.n_terms || !b->count_precise[u] || !b->knobs.join_counts) return false;
  }
  const irs_hip_segment* sg = b->segs[dq.seg];
  for (uint32_t j = 0; j < dq.n_terms; ++j) {
    const DevQTerm& qt = b->qterms[dq.first_term + j];
    if (!table_kind(qt.kind) || qt.cache_id >= kMaxCaches) return false;
    if (sg->terms[qt.term].tf_bound > kJoinTfMax) return false;
  }
  return true;
}

// What the deal holds of the device's stream cache goes back: its pins, and the slabs it claimed
// and never queued a decode for — those leave the cache unfilled, nobody was ever served them.
// `waited`: the caller has waited for the batch's queued work (irs_hip_batch_destroy).
void release_streams(irs_hip_batch* b, bool waited) {
  if (b->join.pinned.empty()) return;
  scache::Cache& c = scache::of(b->seg->device);
  std::vector<scache::SlabPtr> gone;
  {
    std::lock_guard<std::mutex> lock(c.m);
    for (const scache::SlabPtr& s : b->join.fills) {
      if (!s->queued) scache::drop_locked(c, s.get(), gone);
      else if (waited) s->settled.store(true);
    }
    for (const scache::SlabPtr& s : b->join.pinned) --s->pins;
  }
  b->join.fills.clear();
  b->join.pinned.clear();   // (outside the lock: a slab that left the cache is freed here)
  b->join.fill_pending = false;
}
// A run or a plan stage of the batch failed: whatever it was to decode for the cache is not trusted
// — the slabs leave the cache (the batch keeps them: a later run of it decodes into them again).
void abandon_fills(irs_hip_batch* b) {
  if (b->join.fills.empty()) return;
  scache::Cache& c = scache::of(b->seg->device);
  std::vector<scache::SlabPtr> gone;
  std::lock_guard<std::mutex> lock(c.m);
  for (const scache::SlabPtr& s : b->join.fills) scache::drop_locked(c, s.get(), gone);
}

bool join_half_ok(const irs_hip_batch* b);

// Does the batch read decoded streams at all: units on joined streams, wide multi-term units, Ors
// of clauses or tree queries (wide.h, clauses.h, tree.h: their terms are streams of the same set)
bool streams_on(const irs_hip_batch* b) { return b->join.on() || b->wide.on() || b->clause.on() || b->tree.on(); }

// The batch's distinct (segment, term) streams, k_join's work list and the per-(unit, term)
// records of k_join_score.  Static per batch: built once.  Every stream is looked up in the
// device's stream cache (stream_cache.h): a hit costs no k_join work, a miss is decoded once into
// a slab of the cache by the deal's first plan stage; what the cache cannot take is decoded into
// the batch's own buffers in every run.
bool build_streams(irs_hip_batch* b) {
  struct WgRef { uint32_t stream, first; };   // a k_join workgroup before its record is made
  release_streams(b, false);
  std::unique_ptr<HostTrace> tr(new HostTrace("  streams: distinct terms"));
  auto lap = [&](const char* what) { tr.reset(); tr.reset(new HostTrace(what)); };
  std::vector<StreamRec> streams;
  std::vector<WgRef> wgs;
  std::vector<JoinTerm> jterms(b->qterms.size());
  // A stream = a distinct (segment, term, scorer signature) of the joined units: the signature
  // — (kind, norm_const, norm_length) — is normally ONE per batch.  stream_of[unit term] by an
  // open-addressing table: the streams come out in first-use order.
  struct Sig { int32_t kind; float nc, nl; };
  std::vector<Sig> sigs;
  std::vector<uint32_t> stream_of(b->qterms.size(), 0xFFFFFFFFu);
  std::vector<uint8_t> stream_sig;
  // (the joined units' terms first: a batch's streams come out as they do without wide units)
  std::vector<uint32_t> readers(b->join.units);
  readers.insert(readers.end(), b->wide.units.begin(), b->wide.units.end());
  readers.insert(readers.end(), b->clause.units.begin(), b->clause.units.end());
  readers.insert(readers.end(), b->tree.units.begin(), b->tree.units.end());
  {
    size_t slots = 64;
    size_t n_keys = 0;
    for (uint32_t u : readers) n_keys += b->queries[u].n_terms;
    while (slots < 2 * n_keys + 2) slots <<= 1;
    std::vector<uint64_t> hkey(slots, ~0ull);
    std::vector<uint32_t> hval(slots, 0);
    for (uint32_t u : readers) {
      const DevQuery& dq = b->queries[u];
      for (uint32_t j = 0; j < dq.n_terms; ++j) {
        const DevQTerm& qt = b->qterms[dq.first_term + j];
        uint32_t sg_id = 0;
        for (; sg_id < sigs.size(); ++sg_id)
          if (sigs[sg_id].kind == qt.kind && sigs[sg_id].nc == qt.norm_const && sigs[sg_id].nl == qt.norm_length) break;
        if (sg_id == sigs.size()) {
          if (sigs.size() >= 255) return false;
          sigs.push_back(Sig{qt.kind, qt.norm_const, qt.norm_length});
        }
        if (dq.seg >= (1u << 24)) return false;
        const uint64_t key = (uint64_t(sg_id) << 56) | (uint64_t(dq.seg) << 32) | qt.term;
        size_t h = size_t((key * 0x9E3779B97F4A7C15ull) >> 32) & (slots - 1);
        while (hkey[h] != ~0ull && hkey[h] != key) h = (h + 1) & (slots - 1);
        if (hkey[h] == ~0ull) {
          hkey[h] = key;
          hval[h] = uint32_t(streams.size());
          StreamRec r{};
          r.seg = dq.seg;
          r.term = qt.term;
          r.n = b->segs[dq.seg]->terms[qt.term].docs_count;
          streams.push_back(r);
          stream_sig.push_back(uint8_t(sg_id));
        }
        stream_of[dq.first_term + j] = hval[h];
      }
    }
  }
  // where every stream lies: a slab of the cache (hit / fill) or the batch's own buffers
  enum : uint8_t { kPrivate = 0, kHit = 1, kFill = 2 };
  std::vector<uint8_t> where(streams.size(), kPrivate);
  std::vector<uint64_t> ent_at(streams.size(), 0), bnd_at(streams.size(), 0);   // device addresses
  for (size_t si = 0; si < streams.size(); ++si)
    streams[si].n_tiles = (b->segs[streams[si].seg]->dev.num_docs + kJoinTile - 1) / kJoinTile;
  lap("  streams: cache lookup");
  const int device = b->seg->device;
  const uint64_t budget = scache::budget_bytes(device);
  if (budget) {
    scache::Cache& c = scache::of(device);
    std::vector<scache::SlabPtr> gone;   // evicted: freed behind the lock
    std::vector<uint32_t> missed;
    {
      std::unordered_set<scache::Slab*> seen;
      std::lock_guard<std::mutex> lock(c.m);
      for (size_t si = 0; si < streams.size(); ++si) {
        if (!streams[si].n) continue;   // (an empty list: no entries, no k_join work)
        auto it = c.map.find(scache::key_of(b->segs[streams[si].seg]->uid, streams[si].term));
        if (it == c.map.end()) {
          ++c.misses;
          missed.push_back(uint32_t(si));
          continue;
        }
        scache::Slab* sl = it->second.slab;
        if (!sl->queued) {   // claimed by a batch that has not queued its decode yet: not waited for
          ++c.misses;
          continue;
        }
        ++c.hits;
        where[si] = kHit;
        ent_at[si] = it->second.entries;
        bnd_at[si] = it->second.bounds;
        sl->last_use = ++c.clock;
        if (seen.insert(sl).second) {
          ++sl->pins;
          for (const scache::SlabPtr& sp : c.slabs)
            if (sp.get() == sl) b->join.pinned.push_back(sp);
        }
      }
    }
    // the misses, segment by segment, in slabs of at most kSlabEntries entries
    std::stable_sort(missed.begin(), missed.end(),
                     [&](uint32_t x, uint32_t y) { return streams[x].seg < streams[y].seg; });
    for (size_t from = 0; from < missed.size();) {
      size_t to = from;
      uint64_t e = 0, bn = 0;
      std::vector<uint64_t> e_off, b_off;
      while (to < missed.size() && streams[missed[to]].seg == streams[missed[from]].seg &&
             (to == from || e + streams[missed[to]].n <= scache::kSlabEntries)) {
        e_off.push_back(e);
        b_off.push_back(bn);
        e += (uint64_t(streams[missed[to]].n) + scache::kAlign - 1) / scache::kAlign * scache::kAlign;
        bn += uint64_t(streams[missed[to]].n_tiles) + 1;
        ++to;
      }
      const uint64_t bytes = pool::size_class((e + kJoinSlack + bn) * 4);
      bool room = false;
      {
        std::lock_guard<std::mutex> lock(c.m);
        room = bytes <= budget && scache::make_room_locked(c, bytes, budget, gone);
        if (room) c.held += bytes;   // (reserved: the allocation itself happens outside the lock)
      }
      gone.clear();
      scache::SlabPtr sl;
      if (room) {
        sl = std::make_shared<scache::Slab>();
        if (!sl->mem.alloc((e + kJoinSlack + bn) * 4)) {
          std::lock_guard<std::mutex> lock(c.m);
          c.held -= bytes;
          sl.reset();
        }
      }
      if (sl) {
        irs_hip_segment* sg = b->segs[streams[missed[from]].seg];
        sl->bytes = bytes;
        sl->entries = e;
        sl->seg_uid = sg->uid;
        sl->n_streams = uint32_t(to - from);
        sl->pins = 1;
        sl->listed = true;
        uint32_t* base = sl->mem.as<uint32_t>();
        std::lock_guard<std::mutex> lock(c.m);
        sl->last_use = ++c.clock;
        for (size_t i = from; i < to; ++i) {
          const uint32_t si = missed[i];
          where[si] = kFill;
          ent_at[si] = reinterpret_cast<uint64_t>(base + e_off[i - from]);
          bnd_at[si] = reinterpret_cast<uint64_t>(base + e + kJoinSlack + b_off[i - from]);
          // (another batch may have claimed the term since the lookup: its slab keeps the name)
          if (c.map.emplace(scache::key_of(sg->uid, streams[si].term),
                            scache::Where{sl.get(), ent_at[si], bnd_at[si]}).second)
            sl->terms.push_back(streams[si].term);
        }
        c.slabs.push_back(sl);
        b->join.pinned.push_back(sl);
        b->join.fills.push_back(sl);
      }
      from = to;
    }
  }
  b->join.fill_pending = !b->join.fills.empty();
  uint64_t entries = 0, bounds = 0;   // of the private streams
  b->join.n_private = b->join.n_fill = 0;
  for (size_t si = 0; si < streams.size(); ++si) {
    const irs_hip_segment* sg = b->segs[streams[si].seg];
    const DevTerm& t = sg->terms[streams[si].term];
    if (where[si] == kHit) continue;
    ++(where[si] == kFill ? b->join.n_fill : b->join.n_private);
    const uint32_t nb = t.nblk + ((t.docs_count == 1 || t.tail_n) ? 1u : 0u);
    for (uint32_t first = 0; first < nb; first += kJoinBlocks)
      wgs.push_back(WgRef{uint32_t(si), first});
    if (where[si] == kFill) continue;
    ent_at[si] = entries;   // (offsets until the buffers are there)
    bnd_at[si] = bounds;
    entries += t.docs_count;
    bounds += uint64_t(streams[si].n_tiles) + 1;
  }
  if (wgs.size() > 0x7FFFFFFFull) return false;
  lap("  streams: work list order");
  // k_join reads a norm byte per posting: launched term after term, the workgroups in flight
  // would touch the whole norm column at once (10 MB at 10 M docs against 4 MB of L2 per XCD).
  // Ordered by where in the doc space a workgroup's blocks lie — estimated as its position
  // inside its list — the ones in flight share a doc range, i.e. norm cache lines.
  {
    // (a counting sort over 1024 positions per segment: this runs once per batch on the host,
    // in front of the batch's first kernel)
    constexpr uint32_t kPos = 1024;
    // (the private streams' workgroups first, then the fills': a later run launches only the first)
    std::vector<uint32_t> key(wgs.size()), start(2 * b->segs.size() * kPos + 1, 0);
    for (size_t i = 0; i < wgs.size(); ++i) {
      const StreamRec& sr = streams[wgs[i].stream];
      const DevTerm& t = b->segs[sr.seg]->terms[sr.term];
      const uint32_t nb = t.nblk + ((t.docs_count == 1 || t.tail_n) ? 1u : 0u);
      const uint64_t at = (uint64_t(2u * wgs[i].first + kJoinBlocks) * kPos) / (2ull * (nb + kJoinBlocks));
      key[i] = ((where[wgs[i].stream] == kFill ? uint32_t(b->segs.size()) : 0u) + sr.seg) * kPos +
               uint32_t(std::min<uint64_t>(at, kPos - 1));
      ++start[key[i] + 1];
    }
    for (size_t k = 1; k < start.size(); ++k) start[k] += start[k - 1];
    std::vector<WgRef> sorted(wgs.size());
    for (size_t i = 0; i < wgs.size(); ++i) sorted[start[key[i]]++] = wgs[i];
    wgs.swap(sorted);
  }
  lap("  streams: buffers");
  if (b->join.n_private) {
    if (!b->join.d_entries.alloc((entries + kJoinSlack) * 4) || !b->join.d_bounds.alloc((bounds + 1) * 4))
      return false;
  } else {   // (every stream lies in the cache)
    b->join.d_entries.release();
    b->join.d_bounds.release();
  }
  if (!b->join.d_streams.alloc(std::max<size_t>(1, streams.size()) * sizeof(StreamRec)) ||
      !b->join.d_wgs.alloc(std::max<size_t>(1, wgs.size()) * sizeof(JoinWg)) ||
      !b->join.d_jterms.alloc(jterms.size() * sizeof(JoinTerm)) ||
      !b->join.d_args.alloc(2 * sizeof(JoinArgs)) ||
      !b->join.d_units.alloc(std::max<size_t>(1, b->join.units.size()) * 4) ||
      !b->join.d_order.alloc(std::max<size_t>(1, b->join.units.size()) * 4))
    return false;
  // k_join_score's queues (JoinArgs): per launch — the plain disjunctions, then the units with
  // match counts — the units sorted by (segment, heaviest term) and cut into kJoinQueues runs of
  // about equal work, one queue per XCD: the workgroups that share an L2 work on units that share
  // their longest stream (and the same doc range: chunk-major within a queue).
  lap("  streams: queue order");
  std::vector<uint32_t> order;
  {
    struct Item { uint64_t work; uint64_t key; uint32_t unit; };
    b->join.n_plain = 0;
    for (uint32_t part = 0; part < 2; ++part) {
      std::vector<Item> items;
      for (uint32_t u : b->join.units) {
        const DevQuery& dq = b->queries[u];
        if ((query_need(dq.op) > 1u) != (part == 1u)) continue;
        uint64_t w = 0, top = 0, top_term = 0;
        for (uint32_t j = 0; j < dq.n_terms; ++j) {
          const uint32_t term = b->qterms[dq.first_term + j].term;
          const uint64_t df = b->segs[dq.seg]->terms[term].docs_count;
          w += df;
          if (df > top) { top = df; top_term = term; }
        }
        items.push_back({w, (uint64_t(dq.seg) << 32) | top_term, u});
      }
      if (part == 0) b->join.n_plain = uint32_t(items.size());
      std::stable_sort(items.begin(), items.end(),
                       [](const Item& x, const Item& y) { return x.key < y.key; });
      uint64_t total = 0;
      for (const Item& it : items) total += it.work + 1;
      uint32_t (&first)[kJoinQueues + 1] = b->join.first[part];
      size_t at = 0;
      uint64_t done = 0;
      for (uint32_t g = 0; g < kJoinQueues; ++g) {
        first[g] = uint32_t(order.size());
        const uint64_t goal = total * (g + 1) / kJoinQueues;
        const size_t from = at;
        while (at < items.size() && (done < goal || g + 1 == kJoinQueues)) done += items[at++].work + 1;
        // (round 6: the units of a queue by decreasing work instead — longest processing time first
        // within every chunk round — changes nothing: 0.956 ms either way for a 1.25 M-doc share)
        for (size_t i = from; i < at; ++i) order.push_back(items[i].unit);
      }
      first[kJoinQueues] = uint32_t(order.size());
    }
  }
  for (size_t i = 0; i < streams.size(); ++i) {
    if (where[i] == kPrivate) {
      ent_at[i] = reinterpret_cast<uint64_t>(b->join.d_entries.as<uint32_t>() + ent_at[i]);
      bnd_at[i] = reinterpret_cast<uint64_t>(b->join.d_bounds.as<uint32_t>() + bnd_at[i]);
    }
    streams[i].entries = ent_at[i];
    streams[i].bounds = bnd_at[i];
    const Sig& sig = sigs[stream_sig[i]];
    streams[i].kind = sig.kind;
    streams[i].nc = sig.nc;
    streams[i].nl = sig.nl;
  }
  for (irs_hip_segment* sg : b->segs)
    if (prepare_posting_norms(sg) != IRS_HIP_OK) return false;
  // Bound images (join.h k_join_bound) of the streams the plain disjunctions read — where that
  // launch will run paired, and every one of those streams can have one (join_bound_sup).  Looked
  // up in the cache's image map like the streams above: a hit costs nothing, a miss is made once
  // into an image slab by the deal's first plan stage (behind k_join: an image miss whose exact
  // stream is a hit runs only k_join_bound), what the budget cannot take is made into the batch's
  // own buffers in every run.
  lap("  streams: bound images");
  std::vector<BoundWg> bwgs;
  std::vector<JoinTerm> jimgs;
  b->join.img_on = false;
  b->join.img_n_max = 0;
  b->join.n_images = b->join.n_img_private = b->join.n_img_fill = 0;
  b->join.n_bwgs = b->join.n_bwgs_fill = 0;
  if (join_half_ok(b)) {
    std::vector<uint8_t> want(streams.size(), 0), iwhere(streams.size(), kPrivate);
    std::vector<float> img_U(streams.size(), 0.f);
    std::vector<uint64_t> img_ent(streams.size(), 0), img_bnd(streams.size(), 0);
    std::vector<uint32_t> img_tiles(streams.size(), 0), imgs;   // imgs: the streams with an image
    // what an image takes (join.h: slab-aligned pieces): its entries by join_image_entries' bound,
    // whole slabs from a 256-byte-aligned offset — known without a read-back — and two boundary
    // tables, the padded one k_join_score reads and the raw one k_join_bound places postings by
    auto img_entries = [&](uint32_t si) {
      return (join_image_entries(streams[si].n, img_tiles[si]) + kJoinSlab - 1) / kJoinSlab * kJoinSlab;
    };
    auto img_bounds = [&](uint32_t si) { return 2 * (uint64_t(img_tiles[si]) + 1); };
    static_assert(kJoinSlab % scache::kAlign == 0, "a slab-aligned image is stream-aligned");
    // Tsup per (signature, frequency bound): 256 table values each, so kept per deal
    std::vector<std::vector<float>> sup_of(sigs.size(), std::vector<float>(kJoinTfMax + 1u, -1.f));
    bool all = true;
    for (uint32_t u : b->join.units) {
      const DevQuery& dq = b->queries[u];
      if (query_need(dq.op) > 1u) continue;
      if (!b->segs[dq.seg]->dev.has_freq) all = false;
      b->join.img_n_max = std::max(b->join.img_n_max,
                                   (b->segs[dq.seg]->dev.num_docs + kJoinBoundTile - 1) / kJoinBoundTile);
      for (uint32_t j = 0; j < dq.n_terms && all; ++j) {
        const uint32_t si = stream_of[dq.first_term + j];
        if (want[si]) continue;
        want[si] = 1;
        imgs.push_back(si);
        const Sig& sig = sigs[stream_sig[si]];
        const uint32_t tfb = sqrt_kind(sig.kind)
            ? std::min<uint32_t>(std::max<uint32_t>(b->segs[dq.seg]->terms[streams[si].term].tf_bound, 1u), kJoinTfMax)
            : kJoinTfMax;
        float& sup = sup_of[stream_sig[si]][tfb];
        if (sup < 0.f) sup = join_bound_sup(sig.kind, sig.nc, sig.nl, tfb);
        if (!(sup > 0.f)) { all = false; break; }
        img_U[si] = join_bound_scale(sup);
        img_tiles[si] = (b->segs[dq.seg]->dev.num_docs + kJoinBoundTile - 1) / kJoinBoundTile;
      }
      if (!all) break;
    }
    if (all && !imgs.empty()) {
      auto ikey = [&](uint32_t si) {
        const Sig& sig = sigs[stream_sig[si]];
        scache::ImageKey k;
        k.seg_uid = b->segs[streams[si].seg]->uid;
        k.term = streams[si].term;
        k.kind = sig.kind;
        std::memcpy(&k.nc, &sig.nc, 4);
        std::memcpy(&k.nl, &sig.nl, 4);
        return k;
      };
      if (budget) {
        scache::Cache& c = scache::of(device);
        std::vector<scache::SlabPtr> gone;
        std::vector<uint32_t> missed;
        {
          std::unordered_set<scache::Slab*> seen;
          for (const scache::SlabPtr& sp : b->join.pinned) seen.insert(sp.get());
          std::lock_guard<std::mutex> lock(c.m);
          for (uint32_t si : imgs) {
            auto it = c.imap.find(ikey(si));
            if (it == c.imap.end()) {
              missed.push_back(si);
              continue;
            }
            scache::Slab* sl = it->second.slab;
            if (!sl->queued) continue;   // (claimed, not queued yet: not waited for — private)
            iwhere[si] = kHit;
            img_ent[si] = it->second.entries;
            img_bnd[si] = it->second.bounds;
            sl->last_use = ++c.clock;
            if (seen.insert(sl).second) {
              ++sl->pins;
              for (const scache::SlabPtr& sp : c.slabs)
                if (sp.get() == sl) b->join.pinned.push_back(sp);
            }
          }
        }
        std::stable_sort(missed.begin(), missed.end(),
                         [&](uint32_t x, uint32_t y) { return streams[x].seg < streams[y].seg; });
        for (size_t from = 0; from < missed.size();) {
          size_t to = from;
          uint64_t e = 0, bn = 0;
          std::vector<uint64_t> e_off, b_off;
          while (to < missed.size() && streams[missed[to]].seg == streams[missed[from]].seg &&
                 (to == from || e + img_entries(missed[to]) <= scache::kSlabEntries)) {
            e_off.push_back(e);
            b_off.push_back(bn);
            e += img_entries(missed[to]);
            bn += img_bounds(missed[to]);
            ++to;
          }
          const uint64_t bytes = pool::size_class((e + kJoinSlack + bn) * 4);
          bool room = false;
          {
            std::lock_guard<std::mutex> lock(c.m);
            room = bytes <= budget && scache::make_room_locked(c, bytes, budget, gone);
            if (room) c.held += bytes;
          }
          gone.clear();
          scache::SlabPtr sl;
          if (room) {
            sl = std::make_shared<scache::Slab>();
            if (!sl->mem.alloc((e + kJoinSlack + bn) * 4)) {
              std::lock_guard<std::mutex> lock(c.m);
              c.held -= bytes;
              sl.reset();
            }
          }
          if (sl) {
            sl->bytes = bytes;
            sl->entries = e;
            sl->seg_uid = b->segs[streams[missed[from]].seg]->uid;
            sl->n_streams = uint32_t(to - from);
            sl->pins = 1;
            sl->listed = true;
            uint32_t* base = sl->mem.as<uint32_t>();
            std::lock_guard<std::mutex> lock(c.m);
            sl->last_use = ++c.clock;
            for (size_t i = from; i < to; ++i) {
              const uint32_t si = missed[i];
              iwhere[si] = kFill;
              img_ent[si] = reinterpret_cast<uint64_t>(base + e_off[i - from]);
              img_bnd[si] = reinterpret_cast<uint64_t>(base + e + kJoinSlack + b_off[i - from]);
              const scache::ImageKey k = ikey(si);
              if (c.imap.emplace(k, scache::Where{sl.get(), img_ent[si], img_bnd[si]}).second)
                sl->images.push_back(k);
            }
            c.slabs.push_back(sl);
            b->join.pinned.push_back(sl);
            b->join.fills.push_back(sl);
          }
          from = to;
        }
        b->join.fill_pending = !b->join.fills.empty();
      }
      uint64_t ie = 0, ib = 0;   // of the private images
      for (uint32_t si : imgs) {
        if (iwhere[si] != kPrivate) continue;
        img_ent[si] = ie;
        img_bnd[si] = ib;
        ie += img_entries(si);
        ib += img_bounds(si);
      }
      if (ie + ib) {
        if (!b->join.d_img_entries.alloc((ie + kJoinSlack) * 4) || !b->join.d_img_bounds.alloc((ib + 1) * 4))
          return false;
      } else {
        b->join.d_img_entries.release();
        b->join.d_img_bounds.release();
      }
      // k_join_bound's work: the private images' workgroups first (every run), then the fills'
      for (uint32_t pass = 0; pass < 2; ++pass) {
        for (uint32_t si : imgs) {
          if (iwhere[si] != (pass ? kFill : kPrivate)) continue;
          if (!pass) {
            img_ent[si] = reinterpret_cast<uint64_t>(b->join.d_img_entries.as<uint32_t>() + img_ent[si]);
            img_bnd[si] = reinterpret_cast<uint64_t>(b->join.d_img_bounds.as<uint32_t>() + img_bnd[si]);
          }
          ++(pass ? b->join.n_img_fill : b->join.n_img_private);
          const Sig& sig = sigs[stream_sig[si]];
          BoundWg w{};
          w.src = streams[si].entries;
          w.src_bounds = streams[si].bounds;
          w.dst = img_ent[si];
          w.dst_bounds = img_bnd[si];
          w.n = streams[si].n;
          w.n_src_tiles = streams[si].n_tiles;
          w.n_dst_tiles = img_tiles[si];
          w.kind = sig.kind;
          w.nc = sig.nc;
          w.nl = sig.nl;
          w.U = img_U[si];
          for (uint64_t first = 0; first == 0 || first < w.n; first += kJoinBoundPerWg) {
            w.first = uint32_t(first);
            bwgs.push_back(w);
            ++(pass ? b->join.n_bwgs_fill : b->join.n_bwgs);
          }
        }
      }
      if (bwgs.size() > 0x7FFFFFFFull) return false;
      b->join.n_images = uint32_t(imgs.size());
      // the per-(unit, term) records of k_join_score<kJKHalf>: the image, k = ceil(cs 2^-15 / U 2^16)
      // (its bits in the cs field: join_half_term's integer weight), the tiles
      jimgs.assign(b->qterms.size(), JoinTerm{});
      for (uint32_t u : b->join.units) {
        const DevQuery& dq = b->queries[u];
        if (query_need(dq.op) > 1u) continue;
        for (uint32_t j = 0; j < dq.n_terms; ++j) {
          const uint32_t si = stream_of[dq.first_term + j];
          JoinTerm& ji = jimgs[dq.first_term + j];
          ji.entries = img_ent[si];
          ji.bounds = img_bnd[si];
          const uint32_t k16 = join_half_k(b->qterms[dq.first_term + j].c0 * dq.fx_mul, img_U[si]);
          std::memcpy(&ji.cs, &k16, 4);
          ji.mode = 0;
          ji.pad[0] = img_tiles[si];
          ji.pad[1] = 0;
        }
      }
      b->join.img_on = true;
    }
  }
  if (b->join.img_on) {
    // (k_join_score<kJKHalf> reads kJoinSafeBytes at the records' address for every request that
    // nobody uses: join_load4)
    const size_t jimgs_bytes = std::max<size_t>(kJoinSafeBytes, jimgs.size() * sizeof(JoinTerm));
    if (!b->join.d_jimgs.alloc(jimgs_bytes) || b->join.d_jimgs.n < kJoinSafeBytes ||
        !b->join.d_bwgs.alloc(std::max<size_t>(1, bwgs.size()) * sizeof(BoundWg)) ||
        !b->up.copy(b->join.d_jimgs.p, jimgs.data(), jimgs.size() * sizeof(JoinTerm)) ||
        (!bwgs.empty() && !b->up.copy(b->join.d_bwgs.p, bwgs.data(), bwgs.size() * sizeof(BoundWg))))
      return false;
  }
  lap("  streams: k_join records");
  // the workgroups' records (JoinWg: everything k_join reads before its first payload byte)
  JoinWg* wg_recs = static_cast<JoinWg*>(b->up.put(b->join.d_wgs.p, wgs.size() * sizeof(JoinWg)));
  if (!wg_recs && !wgs.empty()) return false;
  for (size_t i = 0; i < wgs.size(); ++i) {
    const StreamRec& sr = streams[wgs[i].stream];
    const irs_hip_segment* sg = b->segs[sr.seg];
    const DevSegment& ds = sg->dev;
    const DevTerm& t = sg->terms[sr.term];
    JoinWg& w = wg_recs[i];
    w.entries = sr.entries;
    w.bounds = sr.bounds;
    w.doc = reinterpret_cast<uint64_t>(ds.doc) + t.doc_start;
    w.dir = reinterpret_cast<uint64_t>(ds.blk_dir + t.dir_off);
    const bool tiny = sg->d_pnorm.p != nullptr;
    w.pnorm = tiny ? reinterpret_cast<uint64_t>(sg->d_pnorm.as<uint8_t>() + t.dir_off * kBlock) : 0ull;
    w.tail_norms = tiny ? reinterpret_cast<uint64_t>(sg->d_tail_norms.as<uint8_t>() + t.tail_row) : 0ull;
    w.tail_docs = reinterpret_cast<uint64_t>(ds.tail_docs + t.tail_row);
    w.tail_freqs = reinterpret_cast<uint64_t>(ds.tail_freqs + t.tail_row);
    w.first = wgs[i].first;
    w.nblk = t.nblk;
    w.tail_n = t.docs_count == 1u ? 1u : t.tail_n;
    w.tail_base = t.nblk ? t.tail_base : 0u;
    w.last_doc = t.last_doc;
    w.n_tiles = (ds.num_docs + kJoinTile - 1) / kJoinTile;
    w.n = sr.n;
    w.dead_lo = uint32_t(reinterpret_cast<uint64_t>(ds.dead));
    w.dead_hi = uint32_t(reinterpret_cast<uint64_t>(ds.dead) >> 32);
    w.pad = 0;
    w.pk = reinterpret_cast<uint64_t>(ds.pk);
    w.pad2 = 0;
  }
  lap("  streams: per-term records");
  for (uint32_t u : readers) {   // (a wide, clause or tree unit's cs carries its own 64-bit scale: DevQuery::fx_mul)
    DevQuery& dq = b->queries[u];
    const uint32_t rows = table_rows(dq.n_caches);
    for (uint32_t j = 0; j < dq.n_terms; ++j) {
      const DevQTerm& qt = b->qterms[dq.first_term + j];
      const size_t sid = stream_of[dq.first_term + j];
      JoinTerm& jt = jterms[dq.first_term + j];
      jt.pad[0] = jt.pad[1] = 0;
      jt.entries = streams[sid].entries;
      jt.bounds = streams[sid].bounds;
      jt.cs = qt.c0 * dq.fx_mul;
      // (the form only matters for a term with frequencies beyond the table's rows: a TF-IDF
      // batch whose terms all fit the tables runs the table-only loop like a BM25 one)
      const bool general = qt.pad1 >= rows;
      jt.mode = (qt.cache_id * rows * 1024u) |
                (general ? kJoinGeneral | (sqrt_kind(qt.kind) ? kJoinSqrt : 0u) : 0u);
      if (qt.kind == kBM1) jt.mode = kWideConst;   // (wide, clause and tree units only: joined units are of the table family)
    }
  }
  // (the slack behind the last stream is only ever read by masked-off look-ahead: zero it once)
  b->join.slack_zeroed = !b->join.n_private;   // (run_uploads_and_fills zeroes it on the run's stream)
  if (!b->up.copy(b->join.d_streams.p, streams.data(), streams.size() * sizeof(StreamRec)) ||
      !b->up.copy(b->join.d_jterms.p, jterms.data(), jterms.size() * sizeof(JoinTerm)) ||
      !b->up.copy(b->join.d_units.p, b->join.units.data(), b->join.units.size() * 4) ||
      !b->up.copy(b->join.d_order.p, order.data(), order.size() * 4))
    return false;
  b->join.n_streams = uint32_t(streams.size());
  b->join.n_wgs = b->join.n_wgs_fill = 0;
  for (const WgRef& w : wgs) ++(where[w.stream] == kFill ? b->join.n_wgs_fill : b->join.n_wgs);
  b->join.entries = entries;
  return true;
}

// k_join for what the batch has to decode in this run: its private streams, and — once — the slabs
// it claimed in the stream cache.  A run whose streams all lie in the cache queues nothing.
bool wait_for_streams(irs_hip_batch* b, rt::stream_t st);
bool launch_join(irs_hip_batch* b, rt::stream_t st) {
  const bool fill = b->join.fill_pending;
  const uint32_t grid = b->join.n_wgs + (fill ? b->join.n_wgs_fill : 0u);
  const uint32_t bgrid = b->join.img_on ? b->join.n_bwgs + (fill ? b->join.n_bwgs_fill : 0u) : 0u;
  b->join.decoded_last = b->join.n_private + (fill ? b->join.n_fill : 0u);
  b->join.images_built_last = b->join.img_on ? b->join.n_img_private + (fill ? b->join.n_img_fill : 0u) : 0u;
  if (!grid && !bgrid) return true;
  bool ok = true;
  if (fill)   // (the slack behind a slab's last stream is only ever read by masked-off look-ahead)
    for (const scache::SlabPtr& s : b->join.fills)
      ok = ok && rt::dmemset(s->mem.as<uint32_t>() + s->entries, 0, kJoinSlack * 4, st);
  if (!ok) return false;
  if (grid)
    with_layout(b->seg->dev.layout, [&](auto L) {
      RT_LAUNCH((k_join<decltype(L)::value>), grid, kThreads, 0, st, b->join.d_wgs.as<JoinWg>());
    });
  ok = rt::last_error_ok();
  if (ok && bgrid) {
    // the images' exact streams: this stage's own k_join is ahead in `st`; a slab out of the cache
    // may still be filling on another stream
    ok = wait_for_streams(b, st);
    if (ok) {
      // the bounds pass and the padded prefix (a stream's first workgroup), then the write pass
      RT_LAUNCH(k_join_bound_tiles, bgrid, kThreads, 0, st, b->join.d_bwgs.as<BoundWg>());
      ok = rt::last_error_ok();
      if (ok) {
        RT_LAUNCH(k_join_bound, bgrid, kThreads, 0, st, b->join.d_bwgs.as<BoundWg>());
        ok = rt::last_error_ok();
      }
    }
  }
  if (ok && fill) {
    // from here on other batches are served these slabs: their runs wait for `filled`
    for (const scache::SlabPtr& s : b->join.fills) {
      s->fill_stream = st;
      ok = ok && s->filled.mark(st);
    }
    if (ok) {
      scache::Cache& c = scache::of(b->seg->device);
      std::lock_guard<std::mutex> lock(c.m);
      for (const scache::SlabPtr& s : b->join.fills) s->queued = true;
      b->join.fill_pending = false;
    }
  }
  return ok;
}
// The slabs the batch reads out of the stream cache may still be filling on another stream (another
// batch's plan stage, or this batch's own, queued ahead): the run's stream gets behind them.
bool wait_for_streams(irs_hip_batch* b, rt::stream_t st) {
  bool ok = true;
  for (const scache::SlabPtr& s : b->join.pinned)
    if (!s->settled.load() && s->fill_stream != st) ok = ok && s->filled.wait(st);
  return ok;
}

// Groups of a batch over several segments (irs_hip_batch_set_shared_threshold): the units of one
// query — where every one of them runs on joined streams and they bin scores alike (the bins
// span [0, upper bound of the query's score]: equal for scorers whose bound does not depend on the
// segment's frequencies).  Anything else keeps a threshold per unit.
bool build_groups(irs_hip_batch* b) {
  b->groups.n = 0;
  const uint32_t n_segs = uint32_t(b->segs.size());
  const bool across = b->comm != nullptr && !b->phrase;
  if (!across && (!b->groups.shared || n_segs < 2 || n_segs > 64 || b->join.units.empty())) return true;
  const uint32_t nq_user = b->nq_user;
  std::vector<uint8_t> is_join(b->nq, 0);
  for (uint32_t u : b->join.units) is_join[u] = 1;
  std::vector<uint32_t> group_of(b->nq, 0), members(size_t(nq_user) * n_segs, 0xFFFFFFFFu);
  uint32_t grouped = 0;
  for (uint32_t g = 0; g < nq_user && n_segs <= 64; ++g) {
    bool ok = true;
    uint32_t live = 0;
    for (uint32_t sgi = 0; sgi < n_segs && ok; ++sgi) {
      const uint32_t u = sgi * nq_user + g;
      const DevQuery& dq = b->queries[u];
      if (!dq.n_terms) continue;   // (nothing of the query in this segment)
      ok = is_join[u] != 0;
      if (across) {
        // the other ranks' units cannot be asked: only a bound that every segment of the index
        // arrives at by itself qualifies (the boosts of ALL the query's terms, present or not)
        ok = ok && b->groups.upper[u] > 0.0;
      } else {
        for (uint32_t s2 = 0; s2 < sgi && ok; ++s2) {
          const DevQuery& other = b->queries[s2 * nq_user + g];
          if (other.n_terms) ok = other.bin_scale == dq.bin_scale && other.k == dq.k;
        }
      }
      ++live;
    }
    if (!ok || live < (across ? 1u : 2u)) continue;
    for (uint32_t sgi = 0; sgi < n_segs; ++sgi) {
      const uint32_t u = sgi * nq_user + g;
      if (!b->queries[u].n_terms) continue;
      if (across) b->queries[u].bin_scale = float(double(kBins) / b->groups.upper[u]);
      group_of[u] = g + 1;
      members[size_t(g) * n_segs + sgi] = u;
    }
    ++grouped;
  }
  // (across ranks the collectives run whatever this rank's own units look like)
  if (!grouped && !across) return true;
  if (!b->groups.d_of.alloc(group_of.size() * 4) || !b->groups.d_members.alloc(members.size() * 4) ||
      !b->groups.d_hist.alloc(uint64_t(nq_user) * (kBins + 2) * 4) ||
      !b->groups.d_sums.alloc((uint64_t(nq_user) * kGroupSumWords + 2) * 4) ||
      !b->up.copy(b->groups.d_of.p, group_of.data(), group_of.size() * 4) ||
      !b->up.copy(b->groups.d_members.p, members.data(), members.size() * 4))
    return false;
  b->groups.n = nq_user;
  return true;
}

bool launch_join_pilot(irs_hip_batch* b, rt::stream_t st) {
  const size_t smem = JoinOff::end + kBins * sizeof(uint32_t);
  if (!big_smem(k_join_pilot, smem)) return false;
  RT_LAUNCH(k_join_pilot, uint32_t(b->join.units.size()), b->join.threads, smem, st,
            b->join.d_units.as<uint32_t>(), b->d_queries.as<DevQuery>(),
            b->d_qterms.as<DevQTerm>(), b->join.d_jterms.as<JoinTerm>(), b->stride_eff,
            b->join.nw_log2, b->d_bstar.as<uint32_t>(), b->estimate ? kPilotMargin : 0u,
            min_bins(b), b->groups.n ? b->groups.d_of.as<uint32_t>() : nullptr,
            b->groups.d_hist.as<uint32_t>());
  return rt::last_error_ok();
}

// One threshold per group from the summed pilot histograms — summed over the ranks first when the
// batch has a communicator: the units of a query on ALL segments of the index then admit together
// what one heap over all segments would (index-search.cpp:719-779).
bool launch_group_threshold(irs_hip_batch* b, rt::stream_t st) {
  if (!b->groups.n) return true;
  if (b->comm && !b->phrase &&
      !rt::comm::all_reduce_u32(b->comm->h, b->groups.d_hist.p, size_t(b->groups.n) * (kBins + 2), st))
    return false;
  RT_LAUNCH(k_group_threshold, b->groups.n, 64, 0, st, b->d_queries.as<DevQuery>(),
            b->groups.d_members.as<uint32_t>(), uint32_t(b->segs.size()),
            b->groups.d_hist.as<uint32_t>(), b->estimate ? kPilotMargin : 0u, min_bins(b),
            b->d_bstar.as<uint32_t>());
  return rt::last_error_ok();
}

// Paired tiles (join.h join_pairs) for the launch of the plain disjunctions: no segment of theirs
// has deleted docs (their entries leave the doc order k_join_rescore searches in).
// IRS_HIP_JOIN_HALF=0 / irs_hip_batch_set_paired_tiles(0) keeps the 32-bit tiles (A/B runs, tests:
// the two must agree bit for bit).
bool join_half_ok(const irs_hip_batch* b) {
  if (b->knobs.join_half == 0) return false;
  if (!b->join.pairs_allowed || !b->acc32 || !b->join.n_plain) return false;
  // Where it pays (measured on one MI355X, GPU time summed over the chip): a (unit, doc tile)
  // visited in a pair saves ~1.4 ns — half of that when the batch is too small to keep the chip
  // busy through the tail of the work queue (fewer than ~400 k visits) —, a look-up of
  // k_join_rescore costs ~40 ps, and a unit looks up about min(3 k / G, k) docs in each of its
  // terms (G: the units that share its threshold — the segments of a batch with a shared
  // threshold times the ranks of its communicator; 3 = kPilotMargin).  10 M docs in one segment,
  // k = 1000: 1.14 us saved against 0.35 per unit (5.65 -> 4.74 ms per 1000 units); a 1.25 M-doc
  // share of it alone: 0.07 against 0.2 (stays on 32-bit tiles: 0.97 against 1.10 ms); the
  // same as 8 segments of one batch: 0.14 against 0.08 (5.79 -> 5.27 ms).
  // IRS_HIP_JOIN_HALF=1 / set_paired_tiles(2) pair whatever the size (tests on small segments).
  // (Since the paired launch reads bound images on kJoinBoundTile-doc tiles — a quarter fewer
  // visits, no table read per posting — these sizes under-state pairing a little more; they are
  // kept: AUTO pairs wherever it did and nowhere earlier.)
  const bool forced = b->join.pairs_forced || b->knobs.join_half == 1;
  uint64_t visits = 0, lookups = 0;
  for (uint32_t u : b->join.units) {
    const DevQuery& dq = b->queries[u];
    if (query_need(dq.op) > 1u) continue;
    if (b->segs[dq.seg]->dev.dead) return false;
    const uint64_t group = uint64_t((b->groups.shared || b->comm) ? b->segs.size() : 1) *
                           uint64_t(b->comm ? std::max(1, b->comm->n_ranks) : 1);
    visits += b->segs[dq.seg]->dev.num_docs / kJoinTile + 1;
    lookups += std::min<uint64_t>((uint64_t(kPilotMargin) * dq.k + group - 1) / group, uint64_t(dq.k) + 64) *
               dq.n_terms;
  }
  if (!forced && (visits >= 400000 ? 1400ull : 700ull) * visits <= 40ull * lookups) return false;
  return true;
}

// k_join_rescore's three unit counters: words 4..6 of the block every run starts from zero (the
// status word's line)
uint32_t* rescore_paths(irs_hip_batch* b) { return b->d_zeroed.as<uint32_t>() + 4; }

// A batch whose whole score stage is the one paired launch — the headline batch — ends its run on
// the device's tail stream (pool.h): k_join_rescore and k_select beside the k_join_pilot of the next
// batch.  Every other batch queues what it always did: a COUNT launch, work items, wide units, block-
// driven units and phrases follow the paired launch in stream order, group thresholds and collectives
// are ordered against other ranks, and the union of a batch with optional terms follows both passes.
bool tail_ok(const irs_hip_batch* b) {
  if (!b->knobs.tail_stream || b->term_pass || b->phrase || b->opt || b->groups.n || b->comm) return false;
  if (!b->join.on() || b->join.n_plain != b->join.units.size()) return false;
  if (!b->tiles.units.empty() || b->wide.on() || b->clause.on() || b->tree.on() || !b->blocks.units.empty() || !b->any.units.empty()) return false;
  return join_half_ok(b) && b->join.img_on;
}

// `tail`: the stream k_join_rescore goes to (a batch that passes tail_ok: it waits for `scored`,
// recorded behind the paired launch on `st`); null: everything on `st`
bool launch_join_score(irs_hip_batch* b, rt::stream_t st, const rt::stream_t* tail) {
  // (paired tiles run on bound images, made at the deal: no images, no pairs)
  const bool half = join_half_ok(b) && b->join.img_on;
  b->join.pairs_used = half;
  const size_t smem_plain = JoinOff::end, smem_half = JoinOffH::end;
  if (!big_smem(k_join_score<kJKPlain>, smem_plain) || !big_smem(k_join_score<kJKCount>, smem_plain) ||
      !big_smem(k_join_score<kJKHalf>, smem_half))
    return false;
  const uint32_t waves = b->join.threads / 64;
  // workgroups resident per CU: what the LDS block leaves of a CU's 160 KB
  auto resident = [&](size_t smem) {
    return std::max<uint32_t>(1, std::min<uint32_t>(uint32_t((160u * 1024u) / smem), 32u / waves));
  };
  static_assert(2u * JoinOffH::end <= 160u * 1024u && 2u * JoinOff::end <= 160u * 1024u,
                "two k_join_score workgroups per CU");
  // chunks of up to kJoinChunkTiles tiles, the unit's tiles cut evenly (102 tiles: 4 x 26, not
  // 3 x 32 + 6 — a short last chunk pays the whole per-chunk prologue for a few tiles).  A small
  // batch takes shorter chunks: with fewer than ~20 chunks per resident workgroup the last round
  // of the work queue leaves CUs idle (1000 units x 102 tiles: 8 chunks per workgroup at 26 tiles,
  // 1.12 ms; 21 at 10 tiles, 0.95 ms — profiles/r05_chunks.txt), while a large batch loses to the
  // per-chunk prologue below 26 (10 M docs: 5.61 ms at 32, 5.88 at 16, 6.50 at 8).
  // (paired tiles: up to the docs of kJoinChunkTiles = 64 exact tiles per chunk, 4.98 -> 4.91 ms:
  // kJoinChunkBound = 48 image tiles = 24 visits)
  auto chunking = [&](uint32_t cap, uint32_t n_max, uint32_t per_cu, uint32_t& cpq, uint32_t& chunk_tiles) {
    const uint64_t tiles = uint64_t(b->join.units.size()) * n_max;
    const uint64_t wgs = uint64_t(b->seg->cus) * per_cu;
    uint32_t max_chunk = uint32_t(std::min<uint64_t>(cap, std::max<uint64_t>(8, tiles / (20 * wgs))));
    const uint32_t v = b->knobs.join_chunk;   // tuning knob: tiles per chunk at most
    if (v >= 1 && v <= cap) max_chunk = v;
    cpq = std::max<uint32_t>(1, (n_max + max_chunk - 1) / max_chunk);
    chunk_tiles = std::max<uint32_t>(1, (n_max + cpq - 1) / cpq);
  };
  const uint32_t n_all = uint32_t(b->join.units.size());
  // [0]: the live counters, [1]: their start values (copied over [0] on the device every run)
  if (!b->join.d_ctr.p && !b->join.d_ctr.alloc(2 * sizeof b->join.ctr_init)) return false;
  // two launches: the plain disjunctions, then the units whose accumulators count matches
  for (uint32_t part = 0; part < 2; ++part) {
    const uint32_t n_units = part ? n_all - b->join.n_plain : b->join.n_plain;
    if (!n_units) continue;
    const bool paired = !part && half;   // (its chunks and tiles count kJoinBoundTile docs)
    const size_t smem = paired ? smem_half : smem_plain;
    const uint32_t per_cu = resident(smem);
    uint32_t cpq = 1, chunk_tiles = 1;
    chunking(paired ? kJoinChunkBound : kJoinChunkPlain, paired ? b->join.img_n_max : b->join.n_max,
             per_cu, cpq, chunk_tiles);
    const uint64_t chunks = uint64_t(n_units) * cpq;
    if (chunks > 0xFFFF0000ull) return false;
    const uint32_t grid = uint32_t(std::min<uint64_t>(chunks, uint64_t(b->seg->cus) * per_cu));
    JoinArgs& a = b->join.args[part];   // read by the kernel from device memory
    a.queries = b->d_queries.as<DevQuery>();
    a.qterms = b->d_qterms.as<DevQTerm>();
    a.jterms = paired ? b->join.d_jimgs.as<JoinTerm>() : b->join.d_jterms.as<JoinTerm>();
    a.bstar = b->d_bstar.as<uint32_t>();
    a.cands = b->d_cands.as<uint64_t>();
    a.cand_count = b->d_cand_count.as<uint32_t>();
    a.hits = b->d_hits.as<unsigned long long>();
    a.order = b->join.d_order.as<uint32_t>();
    a.work_counter = b->join.d_ctr.as<uint32_t>() + part * kJoinQueues;
    uint32_t base = 0;
    for (uint32_t g = 0; g <= kJoinQueues; ++g) {
      a.first[g] = b->join.first[part][g];
      a.base[g] = base;
      if (g < kJoinQueues) {
        b->join.ctr_init[part][g] = base;
        base += (b->join.first[part][g + 1] - b->join.first[part][g]) * cpq;
      }
    }
    a.cpq = cpq;
    a.n_units = n_units;
    a.nw_log2 = b->join.nw_log2;
    const uint32_t v = b->knobs.join_split_log2;   // tuning knob: a tile's entries among the first
    if (v < a.nw_log2) a.nw_log2 = v;                // 2^v wavefronts only
    a.cand_cap = b->cand_cap;
    a.chunk_tiles = chunk_tiles;
    JoinArgs* d_args = b->join.d_args.as<JoinArgs>() + part;
    uint32_t* d_init = a.work_counter + 2 * kJoinQueues;
    if (!b->join.args_valid[part] || std::memcmp(&a, &b->join.args_sent[part], sizeof a) != 0) {
      if (!b->up.copy(d_args, &a, sizeof a) ||
          !b->up.copy(d_init, b->join.ctr_init[part], sizeof b->join.ctr_init[part]) ||
          !b->up.flush(st))
        return false;
      std::memcpy(&b->join.args_sent[part], &a, sizeof a);
      b->join.args_valid[part] = true;
    }
    if (!rt::d2d(a.work_counter, d_init, sizeof b->join.ctr_init[part], st)) return false;
    if (part) {
      RT_LAUNCH(k_join_score<kJKCount>, grid, b->join.threads, smem, st, d_args);
    } else if (half) {
      // (join.d_order: the plain units first — one k_join_rescore workgroup each)
      RT_LAUNCH(k_join_score<kJKHalf>, grid, b->join.threads, smem, st, d_args);
      if (tail && !(rt::last_error_ok() && b->sync.scored.record(st) && b->sync.scored.wait(*tail))) return false;
      RT_LAUNCH(k_join_rescore, n_units, kRescoreThreads, 0, tail ? *tail : st, b->join.d_order.as<uint32_t>(),
                b->d_queries.as<DevQuery>(), b->d_qterms.as<DevQTerm>(), b->join.d_jterms.as<JoinTerm>(),
                b->d_bstar.as<uint32_t>(), b->d_cands.as<uint64_t>(), b->d_cand_count.as<uint32_t>(),
                b->cand_cap, rescore_paths(b));
    } else {
      RT_LAUNCH(k_join_score<kJKPlain>, grid, b->join.threads, smem, st, d_args);
    }
  }
  return rt::last_error_ok();
}

}  // namespace
