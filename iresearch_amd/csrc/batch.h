// batch.h — the state of a batch: what every execution path reads at the top level, and one record
// per path (work items in doc tiles, joined posting streams, wide multi-term units, block-driven
// conjunctions and phrases),
// for thresholds shared across segments and for a run's place on the streams (RunSync) — and, at
// the end, the waits of a batch: one function per thing a caller is about to touch (a run, a plan
// stage, match sets, a setter's re-deal, a reader of the last run, destroy).  The run itself: run.h.
// The unit lists and who fills them (units.h: commit_unit is create's only writer per unit):
//   all_tile_units, all_conj_units, wide.units, clause.units, tree.units   commit_unit, fixed at create
//   blocks.units   a phrase batch: build_phrase_work at create; else deal_units, from all_conj_units
//   any.units      build_any_work at create, from the grouped units commit_unit listed
//   tiles.units, join.units   deal_units (ensure_scratch), from all_tile_units / all_conj_units
//   excl.unit_terms / unit_first / unit_live   commit_unit; build_masks makes the masks from them
// Included by irs_hip.hip (one translation unit).
#pragma once

// (a named namespace: the batch record, at global scope, holds these)
namespace irs_hip {

constexpr uint32_t kDefaultStride = 64;
constexpr uint32_t kPilotMargin = 3;   // estimated threshold: aim at margin * k candidates
constexpr uint32_t kDefaultWgThreads = 512;  // 8 wavefronts share one tile (measured best)

// Tuning and test knobs (environment), read once by irs_hip_batch_create on the caller's thread:
// a batch keeps what was set when it was created.  (IRS_HIP_POOL_MB, IRS_HIP_PINNED_POOL_MB,
// IRS_HIP_STREAM_CACHE_MB, IRS_HIP_TRACE and IRS_HIP_ASYNC_RUN are process-wide settings, not
// batch knobs.)
struct Knobs {
  bool join_off = false;     // IRS_HIP_JOIN=0: no joined streams unless irs_hip_batch_set_path asks
  bool join_counts = true;   // IRS_HIP_JOIN_COUNTS=0: no match counts in joined accumulators
  int join_and = -1;         // IRS_HIP_JOIN_AND: conjunctions joined never (0) / wherever possible (1)
  int join_or = -1;          // IRS_HIP_JOIN_OR: the same for plain disjunctions (-1: by cost)
  int join_half = -1;        // IRS_HIP_JOIN_HALF: paired tiles never (0) / whatever the size (1)
  uint32_t join_chunk = 0;   // IRS_HIP_JOIN_CHUNK: tiles per k_join_score chunk at most (0: by size)
  uint32_t join_split_log2 = ~0u;   // IRS_HIP_JOIN_SPLIT_LOG2: a tile's entries among the first 2^v wavefronts only
  int conj_split_log2 = -1;  // IRS_HIP_CONJ_SPLIT_LOG2: every lead block cut into 2^v pieces
  uint32_t wg_threads = kDefaultWgThreads;   // IRS_HIP_WG_THREADS: threads per k_pilot / k_score workgroup
  uint32_t join_threads = 1024;   // IRS_HIP_JOIN_THREADS: ... per k_join_pilot / k_join_score workgroup
  bool acc64 = false;        // IRS_HIP_ACC=64: 64-bit accumulators whatever the queries
  uint32_t excl_slice = kExclSliceWords;   // IRS_HIP_EXCL_SLICE: mask words per k_excl_mask workgroup (64..8192, a power of two)
  uint32_t match_slice = kMatchSliceWords;   // IRS_HIP_MATCH_SLICE: bitmap words per k_match_slice workgroup (64..8192, a power of two)
  bool tail_stream = true;   // IRS_HIP_TAIL_STREAM=0: k_join_rescore and k_select stay on the caller's stream
  static Knobs from_env() {
    Knobs k;
    int v = 0;
    auto set = [&v](const char* name) {
      const char* e = std::getenv(name);
      if (e) v = std::atoi(e);
      return e != nullptr;
    };
    if (set("IRS_HIP_JOIN")) k.join_off = v == 0;
    if (set("IRS_HIP_JOIN_COUNTS")) k.join_counts = v != 0;
    if (set("IRS_HIP_JOIN_AND")) k.join_and = v != 0;
    if (set("IRS_HIP_JOIN_OR")) k.join_or = v != 0;
    if (set("IRS_HIP_JOIN_HALF") && (v == 0 || v == 1)) k.join_half = v;
    if (set("IRS_HIP_JOIN_CHUNK") && v >= 1 && uint32_t(v) <= kJoinChunkTiles) k.join_chunk = uint32_t(v);
    if (set("IRS_HIP_JOIN_SPLIT_LOG2")) k.join_split_log2 = uint32_t(v);
    if (set("IRS_HIP_CONJ_SPLIT_LOG2") && v >= 0 && v <= int(kConjSplitMax)) k.conj_split_log2 = v;
    if (set("IRS_HIP_WG_THREADS") && (v == 256 || v == 512 || v == 1024)) k.wg_threads = uint32_t(v);
    if (set("IRS_HIP_JOIN_THREADS") && (v == 256 || v == 512 || v == 1024)) k.join_threads = uint32_t(v);
    if (set("IRS_HIP_ACC")) k.acc64 = v == 64;
    if (set("IRS_HIP_EXCL_SLICE") && v >= 64 && uint32_t(v) <= kExclSliceWords && (v & (v - 1)) == 0)
      k.excl_slice = uint32_t(v);
    if (set("IRS_HIP_MATCH_SLICE") && v >= 64 && uint32_t(v) <= kMatchSliceMax && (v & (v - 1)) == 0)
      k.match_slice = uint32_t(v);
    if (set("IRS_HIP_TAIL_STREAM")) k.tail_stream = v != 0;
    return k;
  }
};

// Doc-tile units as work items (score.h): k_plan's tables -> work-item lists -> k_pilot -> k_score
struct TileWork {
  std::vector<uint32_t> units;
  DevBuf d_units;
  // work-item lists of the doc tiles: per-tile item offsets (+ scan scratch) and the 32-byte
  // records themselves
  DevBuf d_off, d_scan_parts, d_items, d_args, d_ub;
  DevBuf d_work;   // k_score's work counter
  ScoreArgs args{}, args_sent{};
  bool args_valid = false;
  uint32_t docs = 0 /* docs per tile, 0 = pick by accumulator width */;
  uint32_t asked = 0;      // irs_hip_batch_configure's tile (0: ensure_scratch picks one per deal)
  bool any_and = false;    // some unit counts matches per doc in the tile kernels (min-match)
  uint32_t n_total = 0;    // doc tiles of all units
  uint32_t n_max = 0;      // ... of the unit with the most (chunk ids per unit)
  uint32_t threads = 0;    // threads per k_pilot / k_score workgroup (power of two x 64)
  uint32_t nw_log2 = 3;    // log2(wavefronts per such workgroup)
};

// Joined posting streams (join.h): every distinct (segment, term) of the batch decoded once per run
// — or not at all, where the device's stream cache holds it
struct JoinWork {
  std::vector<uint32_t> units;
  bool on() const { return !units.empty(); }   // some unit runs on joined streams
  DevBuf d_streams, d_wgs, d_jterms, d_entries, d_bounds, d_args, d_units, d_order;
  uint32_t n_max = 0;   // doc tiles of the unit with the most
  uint32_t n_streams = 0, n_wgs = 0;
  // Decoded streams kept across batches (stream_cache.h).  A stream of the deal is a HIT — it
  // lies in a slab an earlier batch filled: no k_join work —, a FILL — in a slab this deal
  // claimed: decoded by the deal's first plan stage, served to later batches from then on — or
  // PRIVATE — in d_entries / d_bounds, decoded in every run (no cache, the budget full of pinned
  // slabs, a slab another batch has claimed and not queued yet).  d_wgs: the private streams'
  // workgroups (n_wgs), then the fills' (n_wgs_fill), each in doc-position order.
  std::vector<scache::SlabPtr> pinned;   // every slab a stream of the deal lies in, `fills` included
  std::vector<scache::SlabPtr> fills;
  bool fill_pending = false;             // the fills' k_join is not queued yet
  uint32_t n_wgs_fill = 0;
  uint32_t n_private = 0, n_fill = 0;    // streams
  uint32_t decoded_last = 0;             // streams the last plan stage queued k_join work for
  uint32_t threads = 1024, nw_log2 = 4;   // threads per k_join_pilot / k_join_score workgroup
  uint64_t entries = 0;
  bool slack_zeroed = false;   // the readable slack behind d_entries
  JoinArgs args[2]{};   // plain disjunctions / units with match counts
  JoinArgs args_sent[2]{};   // ... as the device last got them
  bool args_valid[2] = {false, false};
  uint32_t n_plain = 0; // units in d_order: the plain ones first
  uint32_t first[2][kJoinQueues + 1]{};   // [launch] the queues' first slots in d_order
  DevBuf d_ctr;                           // [launch][kJoinQueues] work counters
  uint32_t ctr_init[2][kJoinQueues]{};
  bool pairs_allowed = true;   // irs_hip_batch_set_paired_tiles (0: never; 1: by size; 2: whatever the size)
  bool pairs_forced = false;
  bool pairs_used = false;     // ... and whether the last run's plain disjunctions took them
  // Bound images (join.h k_join_bound) of the streams the plain disjunctions read, made where that
  // launch will run paired (join_half_ok at the deal): hits / fills of the stream cache's image
  // map or private (d_img_entries / d_img_bounds, rebuilt behind k_join in every run).  d_jimgs:
  // the per-(unit, term) records of k_join_score<kJKHalf>, parallel to d_jterms; d_bwgs: the
  // private images' k_join_bound workgroups (n_bwgs), then the fills' (n_bwgs_fill).
  DevBuf d_jimgs, d_bwgs, d_img_entries, d_img_bounds;
  bool img_on = false;          // every stream of the plain disjunctions has an image
  uint32_t img_n_max = 0;       // tiles of kJoinBoundTile docs of the plain unit with the most
  uint32_t n_images = 0, n_img_private = 0, n_img_fill = 0;
  uint32_t n_bwgs = 0, n_bwgs_fill = 0;
  uint32_t images_built_last = 0;   // images the last plan stage queued k_join_bound work for
};

// Scored multi-term queries of up to 64 terms (IRS_HIP_OP_MULTITERM; wide.h, plan_wide.h): the units,
// fixed at create — they never change path.  Their terms are streams of JoinWork (build_streams),
// their per-term records lie in join.d_jterms; nothing else of the batch counts them in (acc32,
// count_precise, jt, tiles.any_and, all_tile_units, all_conj_units).
struct WideWork {
  std::vector<uint32_t> units;
  bool on() const { return !units.empty(); }
  DevBuf d_units;
  uint32_t n_max = 0;   // doc tiles of the unit with the most
  uint32_t n_min = 0;   // ... with the fewest, empty units aside (pilot stride)
};

// Ors of clauses (IRS_HIP_CLAUSE_AND; clauses.h, plan_clauses.h): the units, fixed at create, kept
// apart from the rest of the batch exactly as the wide units are — their entries are streams of
// JoinWork behind the joined and the wide units', their per-entry records lie in join.d_jterms, the
// clause table rides in their DevQTerm rows (pad0: the need-mask of the row's clause).
struct ClauseWork {
  std::vector<uint32_t> units;
  bool on() const { return !units.empty(); }
  DevBuf d_units;
  uint32_t n_max = 0;   // doc tiles of the unit with the most
  uint32_t n_min = 0;   // ... with the fewest, empty units aside (pilot stride)
};

// Tree queries (IRS_HIP_TREE_NODE; tree.h, plan_tree.h): the units, fixed at create, kept apart from
// the rest of the batch exactly as the clause units are — their leaves are streams of JoinWork behind
// the joined, the wide and the clause units', their per-row records lie in join.d_jterms, a row's
// DevQTerm::pad0 names its leaf; `nodes`: kTreeMaxNodes records per unit, in the order of `units`.
struct TreeWork {
  std::vector<uint32_t> units;
  std::vector<TreeNode> nodes;
  bool on() const { return !units.empty(); }
  DevBuf d_units, d_nodes;
  uint32_t n_max = 0;   // doc tiles of the unit with the most
  uint32_t n_min = 0;   // ... with the fewest, empty units aside (pilot stride)
};

// Block-driven conjunctions (conj.h) and phrases (phrase.h): a wavefront per block of a unit's lead term
struct BlockWork {
  std::vector<uint32_t> units;
  std::vector<uint32_t> items;   // lead items of every unit
  uint32_t n_items = 0;
  uint32_t n_wgs = 0;          // k_conj workgroups
  uint32_t n_phrase_wgs = 0;   // k_phrase workgroups: kPhraseWaves lead blocks each
  DevBuf d_units, d_items, d_hist;
  DevBuf d_item_base, d_unit_items, d_seek, d_recs;   // k_conj_seek
  DevBuf d_lg;   // [unit] log2 of the pieces a lead block is cut into (ConjItem)
  DevBuf d_item_hits;   // [lead item] matches (ConjArgs::item_hits, k_conj_hits)
  DevBuf d_lead_of;   // by_phrase: slot of every unit's lead term
  // variadic by_phrase (IRS_HIP_PHRASE_ALT in any unit: every phrase unit of the batch runs on
  // k_vphrase): per unit, bit r of `opens` set = row r opens a part; the iteration lead part's rows
  bool variadic = false;
  std::vector<uint32_t> opens;
  DevBuf d_opens, d_lead_rows;   // [unit] opens; lead part's rows lo | hi << 8
  // by_phrase with required terms (IRS_HIP_PHRASE_REQUIRED in any unit: every phrase unit of the
  // batch runs on k_phrase_and): per unit the rows that are phrase words, the required terms' behind
  bool required = false;
  // ... or optional terms (IRS_HIP_PHRASE_OPTIONAL in any unit: every phrase unit of the batch runs
  // on k_phrase_or, the lead among the words only); the term pass: irs_hip_batch::opt
  bool optional = false;
  std::vector<uint32_t> n_phrase;
  DevBuf d_n_phrase;
  // ... or several phrases in one And (IRS_HIP_PHRASE_NEXT in any unit: every phrase unit of the
  // batch runs on k_phrases_and, phrases.h): n_phrase as above (all word rows), and per unit bit r of
  // `phrase_opens` set = row r opens a phrase; they go out in d_opens, which a variadic batch —
  // never one of these — fills with its parts' words
  bool several = false;
  uint32_t n_several = 0;   // units with the flag (irs_hip_batch_phrase_conj_units)
  std::vector<uint32_t> phrase_opens;
  // ... or several phrases in one Or (IRS_HIP_PHRASE_OR in any unit: every phrase unit of the batch
  // runs on k_phrases_or, phrases_or.h): `phrase_opens` over the rows of the PRESENT phrases, in
  // d_opens; every phrase leads with its rarest row, the unit's lead rows as a mask in d_lead_rows
  bool disj = false;
  uint32_t n_disj = 0;      // units with the flag (irs_hip_batch_phrase_disj_units)
  DevBuf d_pilot;             // the lead items the pilot pass samples, {unit, item} each
  uint32_t n_pilot = 0, pilot_stride = 0;
};

// Grouped conjunctions (an And of Ors of by_term, IRS_HIP_GROUP_ALT; conj_any.h): the tables of
// BlockWork, a list of their own — built at create (they never join streams, never change path),
// next to a batch's block-driven or joined flat conjunctions.  `opens` and the lead group's rows as
// for variadic phrases; n_wgs: k_conj_any workgroups.  Of BlockWork the grouped path uses units,
// items, n_items, n_wgs, the lead-item tables (d_units, d_items, d_hist, d_item_base, d_unit_items,
// d_seek, d_recs, d_item_hits), opens / d_opens / d_lead_rows and the pilot list (d_pilot,
// n_pilot, pilot_stride); d_lg, d_lead_of, n_phrase_wgs, `variadic`, `required` and `optional` stay
// unused.
struct AnyWork : BlockWork {};

// Units with excluded terms (IRS_HIP_EXCLUDE) or a doc set (irs_hip_batch_set_doc_sets), excl.h: one
// doc mask per distinct (segment, doc-set row, present excluded terms), built by k_excl_mask in
// every run's plan stage; DevQuery::dead points at it
struct ExclWork {
  std::vector<ExclMask> masks;   // (the `out` pointers lie in d_words)
  std::vector<uint32_t> terms;   // the masks' term ordinals, ExclMask::first / n
  DevBuf d_words, d_masks, d_terms;
  uint32_t slices = 0;           // k_excl_mask workgroups per mask (of the largest segment's)
  bool on() const { return !masks.empty(); }
  // what create found per unit — the masks are made anew when the doc sets change:
  // unit_terms[unit_first[u] .. unit_first[u + 1]) = its present excluded terms, sorted, distinct;
  // unit_live[u]: some doc may match it at all (it has rows)
  std::vector<uint32_t> unit_terms, unit_first;
  std::vector<uint8_t> unit_live;
  // the doc sets: [set_rows][set_words] u64 on the device — the caller's memory, or d_own (the host
  // form's copy); row_of[unit] (IRS_HIP_NO_DOC_SET: unrestricted), empty: no unit is restricted
  const uint64_t* sets = nullptr;
  uint64_t set_rows = 0, set_words = 0;
  std::vector<uint32_t> row_of;
  std::vector<uint8_t> restricted;   // [unit] its mask comes from a doc set
  DevBuf d_own, d_restricted;
  DevBuf d_tile_live;            // [tiles.n_total] k_tile_live's bytes (work-item units)
  DevBuf d_leads;                // 2 x u64: lead pieces of restricted block-driven units / skipped ones
  bool leads_counted = false;    // ... counted by the last run (irs_hip_batch_profile bit 1)
  uint64_t set_bytes = 0;        // irs_hip_batch_work: (num_docs + 7) / 8 per restricted unit
  bool sets_on() const { return !row_of.empty(); }
};

// Unscored execution (match.h, plan_match.h): the units as k_match_slice reads them, built with the
// first irs_hip_batch_match_sets call; the host form's staging of the sets and counts
struct MatchWork {
  bool built = false, sent = false;
  std::vector<MatchUnit> units;
  std::vector<uint32_t> rows;    // the units' term ordinals, MatchUnit::first / n_rows
  DevBuf d_units, d_rows, d_sets, d_counts;
  uint32_t maps = 1;             // LDS bitmaps per workgroup: of the widest op among the units
  uint32_t slice_words = 0;      // 32-bit words of one bitmap (Knobs::match_slice, halved to fit)
  uint32_t max_docs = 0;         // num_docs of the batch's largest segment
};

// Scores of caller-given docs (score_docs.h, plan_score_docs.h): the units as k_score_docs reads
// them, built with the first irs_hip_batch_score_docs call (the rows and node records go out as
// create left them); the host form's staging of the lists and results
struct ScoreDocsWork {
  bool built = false, sent = false;
  std::vector<SdUnit> units;
  std::vector<uint32_t> seg_docs;   // num_docs of every segment of the batch
  DevBuf d_units, d_rows, d_nodes, d_docs, d_chunks, d_scores, d_matched;
};

// One threshold per query for its units on the batch's segments (irs_hip_batch_set_shared_threshold)
// ... across ranks (irs_hip_batch_set_comm): the group histograms and the group sums are summed
// over the communicator's ranks inside every run
struct Groups {
  bool shared = false;
  uint32_t n = 0;       // groups in force this run (0: none)
  DevBuf d_of;          // [unit] group + 1, 0: a threshold of its own
  DevBuf d_members;     // [nq_user][n_segs] unit or 0xFFFFFFFF
  DevBuf d_hist;        // [nq_user][kBins + 2]
  DevBuf d_sums;        // [nq_user][kGroupSumWords] + 2 status counters (k_group_sums)
  DevBuf d_agree;   // one word: the ranks' vote before a collective re-run (all_ranks_can)
  std::vector<double> upper;   // [unit] a score bound that is the same on every segment, 0: none
};

// A run's place on the streams, what waits for it, and where its results land on the host.  Whoever
// touches a batch's buffers asks for its waits by name (the functions at the end of this file); the
// Pendings here are recorded and read by those and by the stages of a run (run.h) only.
struct RunSync {
  // the end of the batch's OWN last run (not whatever else the caller has queued on the stream
  // since), and the status word that run left in page-locked memory.  Pending: a run recorded it —
  // it stays so for the batch's life, a host wait does not clear it (sync_keep: later stream waits
  // for the same run are issued all the same)
  Pending done;
  PinBuf h_status;
  // a run whose score stage is the one paired launch (tail_ok) ends on the device's tail stream:
  // `scored` lies behind k_join_score<kJKHalf> on the caller's stream, the tail waits for it, and
  // `done` is recorded on the tail stream — NOTHING of such a run is ordered by the caller's
  // stream behind `scored`: whoever reads what the run leaves gets behind `done`
  Event scored;
  bool tail_used = false;      // the last run took the tail stream
  // irs_hip_batch_plan: the planning stage of the NEXT run was queued ahead (on another stream).
  // Pending whether or not the next run will use its tables: the kernels it queued keep reading and
  // writing the batch's buffers
  Pending plan;
  bool planned = false;        // ... and the next run may use it (same geometry: deal_is_stale drops it)
  // the last copy OUT of the batch's buffers queued by irs_hip_batch_results_to_device
  Pending used;
  // the last irs_hip_batch_match_sets_to_device queued on some stream: it reads the exclusion masks
  // and the match tables
  Pending matched;
  // the last irs_hip_batch_score_docs_to_device queued on some stream: it reads the exclusion masks
  // and the score-docs tables
  Pending docs_scored;
  Event uploaded;   // the first run's table uploads (the device's copy stream)
  Event prof[2 * IRS_HIP_K_COUNT];   // irs_hip_batch_profile: around every stage of a run
  PinBuf h_pin;                // page-locked staging for irs_hip_batch_results
  // irs_hip_batch_results_to_host: hits, counts and totals in page-locked memory of the batch
  // (`host` pending: the copy may be in flight AND h_res holds the last run's results — the next
  // run settles it, irs_hip_batch_host_results refuses from then on)
  PinBuf h_res;
  Pending host;
  // irs_hip_batch_run hands the host half of a run (units dealt, streams and work lists built,
  // uploads and launches queued: ~1 ms for 1000 queries) to the device's worker thread and returns;
  // every other entry point waits here for it first.  async_rc: what that run returned.
  std::mutex m;
  std::condition_variable cv;
  bool async_pending = false;
  int async_rc = 0;
  int async_pref = -1;   // irs_hip_batch_set_async: -1 the process default (IRS_HIP_ASYNC_RUN), 0 / 1
};

}  // namespace irs_hip

struct irs_hip_comm {
  int device = 0;
  int n_ranks = 1, rank = 0;
  rt::comm::handle_t h = nullptr;
};

struct irs_hip_batch {
  irs_hip_segment* seg = nullptr;          // segs[0]: device, CU count
  std::vector<irs_hip_segment*> segs;      // a batch spans one or more segments of one device
  uint32_t nq_user = 0;                    // queries per segment
  uint32_t nq = 0 /* execution units = segments x queries */, jt = 0, k_max = 0;
  uint32_t stride = kDefaultStride, cand_cap = 0;
  bool estimate = true;  // k_pilot picks an estimated threshold (falls back to the sound one)
  uint32_t reruns = 0;   // recoveries so far (underflow or overflow re-runs)
  uint32_t n_tiles = 0;     // of the segment with the FEWEST tiles (pilot stride, recovery)
  uint32_t stride_eff = 1;  // pilot stride actually used (>= 2 pilot tiles per segment when possible)
  bool wand = false;       // irs_hip_batch_set_wand
  Knobs knobs;             // the environment's tuning / test knobs at create
  // units by the kernels that execute them: doc tiles (Or, min-match) / lead blocks (And)
  // (all_tile_units: every doc-tile unit, fixed at create; ensure_scratch deals them to
  // join.units — plain disjunctions run as joined posting streams, join.h — and tiles.units —
  // the rest, score.h's work items)
  // (all_conj_units: every conjunction, fixed at create; ensure_scratch deals them to
  // join.units — accumulators with match counts, join.h — and blocks.units — block driven, conj.h)
  std::vector<uint32_t> all_tile_units, all_conj_units;
  std::vector<uint8_t> count_precise;   // [unit] match counts may share its 32-bit accumulators
  DevBuf d_min_bin;   // [unit] score bin of the caller's irs::score::Min (irs_hip_batch_set_min_scores)
  DevBuf d_min_score; // [unit] ... and the score itself (k_select's exact filter)
  bool has_min = false;
  // the caller's scores themselves: their bins are worked out when a run's tables go out — AFTER
  // ensure_scratch, which may change a unit's bin_scale (build_groups across ranks)
  std::vector<float> min_scores;   // [unit]
  bool min_dirty = false;
  bool phrase = false;  // a batch of by_phrase queries (k_phrase instead of k_pilot + k_score)
  bool acc32 = true;   // 32-bit fixed-point accumulators are precise enough for every query
  bool scratch_ready = false;
  std::vector<DevQuery> queries;
  std::vector<DevQTerm> qterms;
  DevBuf d_segs, d_queries, d_qterms, d_first, d_tails, d_bstar, d_cands, d_cand_count, d_hits,
    d_out, d_out_count, d_status;
  DevBuf d_pruned;    // [unit] u32: block-max pruning skipped something of the unit in this run
  DevBuf d_zeroed;    // owns d_status, d_bstar, d_cand_count, d_hits, d_touched, d_pruned (views): one fill per run
  DevBuf d_touched;   // [unit][2] u64: bytes decoded / positions read by the block-driven kernels
  uint64_t alg_bytes = 0, postings = 0;
  int path_pref = 0;   // irs_hip_batch_set_path (0 auto, 1 work items, 2 joined streams)
  irs_hip_comm* comm = nullptr;   // irs_hip_batch_set_comm
  bool profile = false;
  bool count_touched = false;   // irs_hip_batch_profile bit 1: the kernels count what they decode
  rt::stream_t stream = nullptr;
  bool ran = false;
  // host -> device tables of the batch: built in page-locked memory, sent with the next run
  Stager up;
  TileWork tiles;
  JoinWork join;
  WideWork wide;
  ClauseWork clause;
  TreeWork tree;
  BlockWork blocks;
  AnyWork any;
  // A batch with optional terms (IRS_HIP_PHRASE_OPTIONAL): this batch is the PHRASE PASS; `opt` — a
  // batch of its own, created and destroyed with this one, the same units — is the TERM PASS: every
  // unit's optional terms as a plain disjunction, restricted to the doc sets in d_taken ([unit]
  // [taken_words] u64, bit = doc id: zeroed at the start of a run, k_phrase_or sets the docs the phrase
  // matched, k_not_words turns the rows into "not taken").  k_union_topk merges the two passes' top k and totals into d_union_*, which is
  // what the result calls hand out.
  irs_hip_batch* opt = nullptr;
  bool term_pass = false;   // this batch IS the term pass of another (the union follows it in stream order)
  DevBuf d_taken, d_union_out, d_union_count, d_union_hits;
  uint64_t taken_words = 0;
  ExclWork excl;
  MatchWork match;
  ScoreDocsWork score_docs;
  Groups groups;
  RunSync sync;
};

namespace {

template<typename K>
bool big_smem(K kernel, size_t bytes) {
  return rt::allow_dynamic_smem(reinterpret_cast<const void*>(kernel), bytes);
}

// Candidate slots per query.  An estimated threshold aims at kPilotMargin * k
// candidates; the sound one admits about k * (pilot stride).
static const uint32_t* min_bins(const irs_hip_batch* b) {
  return b->has_min ? b->d_min_bin.as<uint32_t>() : nullptr;
}

static uint32_t default_cand_cap(const irs_hip_batch* b) {
  const uint64_t per_k = b->estimate ? 16ull : 4ull * b->stride_eff;
  uint64_t learned = 0;   // (block-driven units only: tile units cut ties by their per-tile staging)
  if (b->phrase || !b->all_conj_units.empty() || !b->any.units.empty())
    for (const irs_hip_segment* sg : b->segs) learned = std::max<uint64_t>(learned, sg->cand_cap_hint.load());
  return uint32_t(std::min<uint64_t>(std::max<uint64_t>({per_k * b->k_max, 16384, learned}), 262144));
}

// ---- the waits of a batch, once each, by what the caller is about to touch ----------------------
// (a Pending that was never recorded waits for nothing: none of these asks whether there was a run,
// a plan queued ahead, a copy)

// The host is about to read what the last run left (status word, results, timings, unit masks,
// doc-set tallies): behind that run's own end — not behind the stream, see RunSync::scored.
static bool run_done(const irs_hip_batch* b) { return b->sync.done.sync_keep(); }
// ... AND behind whatever else is queued on that run's stream
static bool after_run(const irs_hip_batch* b) {
  const bool ok = run_done(b);
  return rt::sync(b->stream) && ok;
}
// A copy queued on `st` is about to read what the last run left: `st` behind that run's end
static bool run_done_on(const irs_hip_batch* b, rt::stream_t st) { return b->sync.done.wait(st); }
// The status word of the batch's last run, out of the page-locked word that run copied it to
static bool run_status(const irs_hip_batch* b, uint32_t* status) {
  if (!b->sync.h_status.p || !run_done(b)) return false;
  *status = *b->sync.h_status.as<uint32_t>();
  return true;
}

// The host is about to re-deal the units (buffers are reallocated, tables rewritten): whatever of
// the batch is still queued is through — a plan stage queued ahead, its last run and that run's
// stream, match sets on another stream.
static bool quiesce(irs_hip_batch* b) {
  bool ok = b->sync.plan.sync();
  if (b->ran) ok = after_run(b) && ok;
  ok = b->sync.matched.sync() && ok;
  return b->sync.docs_scored.sync() && ok;
}

// A plan stage is about to rewrite the plan tables and the masks on `st`: behind the batch's last
// run (it reads them), a plan queued earlier and never used (it may run on ANOTHER stream), match
// sets on another stream (they read the masks).
static bool plan_get_behind(const irs_hip_batch* b, rt::stream_t st) {
  return b->sync.done.wait(st) && b->sync.plan.wait(st) && b->sync.matched.wait(st) &&
         b->sync.docs_scored.wait(st);
}

// Match sets are about to read the masks and the tables on `st`, and to rewrite the masks: behind a
// plan stage and a run (they write the masks and may have the tables in flight) and an earlier
// call's kernels on another stream.
static bool match_get_behind(const irs_hip_batch* b, rt::stream_t st) {
  return b->sync.plan.wait(st) && b->sync.done.wait(st) && b->sync.matched.wait(st) &&
         b->sync.docs_scored.wait(st);
}

// A run is about to rewrite the batch's tables and outputs on `st`, and — a first run with tables
// staged since create — to upload on the device's copy stream (*up_st, else null).  Behind:
//   host      a copy of the PREVIOUS run's results to host memory may still read d_out / d_hits
//             (those host results are stale from here on: irs_hip_batch_host_results refuses them)
//   done      the batch's own last run, if it ended on the tail stream (a replay, a recovery
//             re-run): stream order on `st` does not cover that tail
//   plan      a plan stage still queued — used by this run or made stale by a setter — reads and
//             writes the tables this run uploads and rewrites: both streams
//   matched   match sets on another stream read the masks and the tables: both streams
//   docs_scored  irs_hip_batch_score_docs_to_device on another stream reads the masks and the
//             score-docs tables: both streams
// `host`, `matched` and `docs_scored` are settled here though only a stream waited: whatever
// touches these buffers later — a run, a plan stage, match sets, a score-docs call, a setter,
// destroy — gets behind this run's `done`, which is recorded behind everything `st` has waited for.
static bool run_get_behind(irs_hip_batch* b, rt::stream_t st, rt::stream_t* up_st) {
  RunSync& s = b->sync;
  if (!s.host.wait(st)) return false;
  s.host.settle();
  if (s.tail_used && !s.done.wait(st)) return false;
  if (!s.plan.wait(st)) return false;
  *up_st = (!b->ran && !b->up.pending.empty()) ? upload_stream(b->seg->device) : nullptr;
  if (*up_st && !s.plan.wait(*up_st)) return false;
  if (!s.matched.wait(st) || (*up_st && !s.matched.wait(*up_st))) return false;
  s.matched.settle();
  if (!s.docs_scored.wait(st) || (*up_st && !s.docs_scored.wait(*up_st))) return false;
  s.docs_scored.settle();
  return true;
}

// The batch is about to go away, its buffers back to the pool: every piece of queued work that
// touches them is through — its own last run, a plan queued ahead, copies out of d_out, match sets.
// Not the caller's stream, which may hold the NEXT batch.  false: a wait failed, or a run ended
// without recording its end (the caller falls back to the streams themselves).
static bool quiet_for_destroy(irs_hip_batch* b) {
  RunSync& s = b->sync;
  const bool ended = !b->ran || s.done.pending();
  return s.done.sync() && s.plan.sync() && s.used.sync() && s.host.sync() && s.matched.sync() && s.docs_scored.sync() && ended;
}

// A setter is about to change what the deal of the units depends on: the batch's device, and the
// batch quiet ...
static bool quiet_for_setter(irs_hip_batch* b) { return rt::set_device(b->seg->device) && quiesce(b); }
// ... and afterwards the deal is made anew, and a plan queued ahead — made for the old geometry,
// path, masks — is not used: the next run plans inline
static void deal_is_stale(irs_hip_batch* b) {
  b->scratch_ready = false;
  b->sync.planned = false;
}

}  // namespace
