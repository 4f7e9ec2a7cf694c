// units.h — the query -> unit step of irs_hip_batch_create: one query in one segment becomes one
// unit (a DevQuery, its DevQTerm rows, its entries in the per-path side tables).  The steps stand here
// in the order create runs them, which decides the status a bad query gets.  Only the two *_rule
// functions read the batch, only commit_unit writes it; the others work on the query, the segment's
// term table, the Unit record and the scratch rows.  Included by irs_hip.hip (one translation unit).
#pragma once

extern "C" {   // (irs_hip.hip, next to the entry points)
static int batch_create_multi_impl(irs_hip_segment* const* segs, uint32_t n_segs,
                                   const irs_hip_query* queries, uint32_t nq_user,
                                   const irs_hip_term_scorer* all_terms, uint32_t n_entries,
                                   irs_hip_batch** out);
static int batch_set_doc_sets_impl(irs_hip_batch* b, const void* sets, bool host, uint64_t n_rows,
                                   uint64_t n_words, const uint32_t* row_of_unit);
}

namespace {

constexpr uint32_t kEmptyUnit = 0xFFu;   // `need` of a unit no doc of its segment can match

enum class OpClass : int32_t {   // (the API's values)
  kOr = IRS_HIP_OP_OR, kAnd = IRS_HIP_OP_AND, kMinMatch = IRS_HIP_OP_MINMATCH, kPhrase = IRS_HIP_OP_PHRASE,
  kWide = IRS_HIP_OP_MULTITERM
};
// the entries behind a phrase's words: by_term children of the And (IRS_HIP_PHRASE_REQUIRED) or of
// the Or (IRS_HIP_PHRASE_OPTIONAL) that holds the phrase
enum class Behind { kNone, kRequired, kOptional };

// What unit_shape finds: the included entries, then the excluded ones (IRS_HIP_EXCLUDE)
struct UnitShape {
  uint32_t n_incl = 0, n_excl = 0;
  uint32_t n_words = 0;    // a phrase: its words, the entries `behind` follow; else n_incl
  OpClass op = OpClass::kOr;
  bool variadic = false;   // a phrase with IRS_HIP_PHRASE_ALT members
  bool grouped = false;    // an And with IRS_HIP_GROUP_ALT members
  bool clause = false;     // an Or / min-match Or with IRS_HIP_CLAUSE_AND members (clauses.h)
  // a tree query (IRS_HIP_TREE_NODE entries, tree.h): n_incl counts its LEAVES, positive and negated
  // (entry leaf_at[l] of UnitScratch::tab is leaf l), n_excl is 0 — the negated leaves are rows, no mask
  bool tree = false;
  Behind behind = Behind::kNone;
  // an And of several phrases (IRS_HIP_PHRASE_NEXT, phrases.h): bit j of `opens` = entry j opens a
  // phrase (bit 0 always); a unit with rows has a row per entry, so these are its rows too
  bool several = false;
  uint32_t n_phrases = 1, opens = 1;
  // an Or of several phrases (IRS_HIP_PHRASE_OR, phrases_or.h): n_phrases and `opens` as above, over
  // the ENTRIES — a phrase with an absent word has no rows (unit_rows: Unit::disj_opens)
  bool disj = false;
  bool phrase() const { return op == OpClass::kPhrase; }
  bool wide() const { return op == OpClass::kWide; }
};

// The parts of a phrase while unit_rows walks its entries: a plain word or a required term opens a
// part, an IRS_HIP_PHRASE_ALT entry is one more member of it, optional terms are no parts
struct PhraseParts {
  uint32_t n = 0;           // parts so far
  uint32_t first = 0;       // the current part's first entry
  bool open = false;        // ... has a present member
  uint32_t opens = 0;       // bit r: row r is the first present member of its part
  uint32_t found = 0;       // bit p: part p has a present member
  uint32_t word_rows = 0;   // present rows that are phrase words (the rows behind them follow)
  int enter(const irs_hip_term_scorer* ents, uint32_t j, bool member, bool optional) {
    if (member) {   // at the part's offset, a term not yet in it
      if (ents[j].phrase_offset != ents[first].phrase_offset) return IRS_HIP_EINVAL;
      for (uint32_t x = first; x < j && ents[j].term != IRS_HIP_NO_TERM; ++x)
        if (ents[x].term == ents[j].term) return IRS_HIP_EINVAL;
    } else if (!optional) {
      ++n;
      first = j;
      open = false;
    }
    return IRS_HIP_OK;
  }
  void present(size_t row) {
    if (!open) opens |= 1u << row;
    open = true;
    found |= 1u << (n - 1u);
  }
  bool complete() const { return found == (1u << n) - 1u; }
};

// One unit on its way through the steps; its present rows are UnitScratch::row
struct Unit {
  UnitShape shape;
  // unit_rows
  bool absent = false;       // a flat query: some included term is not in the segment
  bool same_bound = true;    // every scorer's bound is its boost, whatever the segment holds
  double upper = 0.0, min_score = 1e300, upper_all = 0.0;
  uint64_t postings = 0, alg_bytes = 0;
  PhraseParts parts;
  // a grouped And: an entry without IRS_HIP_GROUP_ALT opens a group; bit g: group g has a present member
  // (an Or of clauses: an entry without IRS_HIP_CLAUSE_AND opens a clause; bit g: every member of
  // clause g is present)
  uint32_t n_groups = 0, groups_found = 0;
  uint32_t disj_opens = 0;   // an Or of phrases: bit r = row r opens a (present) phrase
  uint32_t need = 1;         // unit_need: the present terms a doc must match, or kEmptyUnit
  // unit_run
  int32_t op = 0;
  bool any_and = false;      // the tile kernels count its matches per doc
  bool count_precise = false;
  uint32_t group_opens = 0;  // a grouped And: bit r = row r opens its group, the groups by cost
  uint32_t n_caches = 0;     // assign_table_slots
  // unit_scale
  float bin_scale = 0.f;
  double shared_upper = 0.0; // Groups::upper
  int exp = 0;               // upper < 2^exp
  bool acc64 = false;        // 32-bit accumulators would not be precise enough
};

// Allocated once per batch: 8000 units otherwise pay 16000 allocations
struct UnitScratch {
  std::vector<DevQTerm> row;          // the unit's present terms
  std::vector<double> smins;          // per present term: the smallest score of one posting
  std::vector<uint32_t> excl;         // the unit's present excluded terms
  std::vector<uint32_t> row_group;    // per row of a grouped And: its group; of an Or of clauses: its clause
  TreeTable tab;                      // a tree query's compiled node table and leaves (tree_shape.h)
};

// A scored multi-term query (IRS_HIP_OP_MULTITERM, wide.h): up to IRS_HIP_MAX_WIDE_TERMS entries
// (by_terms_options::min_match is 1..#terms for a posting-list query: 0 is the all-docs filter,
// terms_filter.cpp:119-123, more than the terms nothing, :125-128)
int wide_shape_ok(const irs_hip_query& in, const UnitShape& sh) {
  if (sh.n_incl <= IRS_HIP_MAX_WIDE_TERMS && (in.min_match == 0 || in.min_match > sh.n_incl)) return IRS_HIP_EINVAL;
  if (sh.n_incl > IRS_HIP_MAX_WIDE_TERMS || sh.n_excl || in.merge != IRS_HIP_MERGE_SUM) return IRS_HIP_EUNSUPPORTED;
  return IRS_HIP_OK;
}

// A phrase with required terms (IRS_HIP_PHRASE_REQUIRED): the phrase's words (n_words, at least 2),
// then the by_term children of the And that holds it, nothing else behind them ... or with optional
// terms (IRS_HIP_PHRASE_OPTIONAL): the by_term children of the Or that holds it, in the same place;
// one query takes one of the two flags.  This is where the two flags are interpreted.
int phrase_behind(const irs_hip_term_scorer* ents, UnitShape& sh) {
  constexpr int32_t kBehind = IRS_HIP_PHRASE_REQUIRED | IRS_HIP_PHRASE_OPTIONAL;
  sh.n_words = 0;
  while (sh.n_words < sh.n_incl && !(ents[sh.n_words].kind & kBehind)) ++sh.n_words;
  if (sh.n_words == sh.n_incl) return IRS_HIP_OK;
  int32_t flags = 0;
  for (uint32_t j = sh.n_words; j < sh.n_incl; ++j) {
    if (!(ents[j].kind & kBehind)) return IRS_HIP_EINVAL;
    flags |= ents[j].kind & kBehind;
  }
  uint32_t plain = 0;   // (members of a variadic part are no words of their own)
  for (uint32_t j = 0; j < sh.n_words; ++j) plain += (ents[j].kind & IRS_HIP_PHRASE_ALT) ? 0u : 1u;
  if (plain < 2) return IRS_HIP_EINVAL;
  if (sh.variadic || flags == kBehind || sh.n_incl > IRS_HIP_MAX_PHRASE_TERMS) return IRS_HIP_EUNSUPPORTED;
  sh.behind = flags == IRS_HIP_PHRASE_REQUIRED ? Behind::kRequired : Behind::kOptional;
  return IRS_HIP_OK;
}

// A chain of phrases (IRS_HIP_PHRASE_NEXT on the first word of every phrase but the first): the
// words of phrase 1, of phrase 2, ..., then required terms.  This is where the flag is interpreted;
// phrase_behind, which follows, sees the words of all phrases as the words in front of the
// required terms.  A query without the flag passes untouched.
int phrase_chain(const irs_hip_term_scorer* ents, UnitShape& sh) {
  constexpr int32_t kBehind = IRS_HIP_PHRASE_REQUIRED | IRS_HIP_PHRASE_OPTIONAL;
  constexpr int32_t kFlags = kBehind | IRS_HIP_PHRASE_ALT | IRS_HIP_PHRASE_NEXT;
  sh.opens = 1;
  sh.n_phrases = 1;
  int32_t kinds = 0;
  for (uint32_t j = 0; j < sh.n_incl; ++j) kinds |= ents[j].kind;
  sh.several = (kinds & IRS_HIP_PHRASE_NEXT) != 0;
  if (!sh.several) return IRS_HIP_OK;
  uint32_t first = 0;       // the current phrase's first entry
  bool behind = false;      // a required / optional entry has been seen
  for (uint32_t j = 0; j <= sh.n_incl; ++j) {
    const bool end = j == sh.n_incl;
    const int32_t kind = end ? 0 : ents[j].kind;
    const bool next = (kind & IRS_HIP_PHRASE_NEXT) != 0;
    if (next && (j == 0 || behind || (kind & (kBehind | IRS_HIP_PHRASE_ALT)) ||
                 (kind & ~kFlags) == IRS_HIP_EXCLUDE || ents[j].phrase_offset != 0))
      return IRS_HIP_EINVAL;
    // the current phrase ends in front of the next one, of the first entry behind the words, of
    // the end: a phrase of one word is none
    if (!behind && (end || next || (kind & kBehind))) {
      if (j - first < 2) return IRS_HIP_EINVAL;
      // its words carry ONE scorer: the phrase's stats blob
      for (uint32_t x = first + 1; x < j; ++x) {
        const irs_hip_term_scorer &a = ents[first], &w = ents[x];
        if ((a.kind & ~kFlags) != (w.kind & ~kFlags) || a.c0 != w.c0 || a.norm_const != w.norm_const ||
            a.norm_length != w.norm_length)
          return IRS_HIP_EINVAL;
      }
    }
    if (next) {
      sh.opens |= 1u << j;
      ++sh.n_phrases;
      first = j;
    }
    behind = behind || (kind & kBehind) != 0;
  }
  if (sh.n_incl > IRS_HIP_MAX_PHRASE_TERMS || (kinds & (IRS_HIP_PHRASE_ALT | IRS_HIP_PHRASE_OPTIONAL)))
    return IRS_HIP_EUNSUPPORTED;
  return IRS_HIP_OK;
}

// Alternative phrases (IRS_HIP_PHRASE_OR on the first word of every phrase but the first): the words
// of phrase 1, of phrase 2, ..., nothing behind them but excluded terms.  This is where the flag is
// interpreted; a query without it passes untouched.
int phrase_alternatives(const irs_hip_term_scorer* ents, UnitShape& sh) {
  constexpr int32_t kOthers = IRS_HIP_PHRASE_REQUIRED | IRS_HIP_PHRASE_OPTIONAL | IRS_HIP_PHRASE_ALT | IRS_HIP_PHRASE_NEXT;
  constexpr int32_t kFlags = kOthers | IRS_HIP_PHRASE_OR;
  int32_t kinds = 0;
  for (uint32_t j = 0; j < sh.n_incl; ++j) kinds |= ents[j].kind;
  sh.disj = (kinds & IRS_HIP_PHRASE_OR) != 0;
  if (!sh.disj) return IRS_HIP_OK;
  sh.opens = 1;
  sh.n_phrases = 1;
  uint32_t first = 0;       // the current phrase's first entry
  for (uint32_t j = 0; j <= sh.n_incl; ++j) {
    const bool end = j == sh.n_incl;
    const bool next = !end && (ents[j].kind & IRS_HIP_PHRASE_OR) != 0;
    if (next && (j == 0 || (ents[j].kind & ~kFlags) == IRS_HIP_EXCLUDE || ents[j].phrase_offset != 0))
      return IRS_HIP_EINVAL;
    if (end || next) {   // the current phrase ends here: a phrase of one word is none
      if (j - first < 2) return IRS_HIP_EINVAL;
      // its words carry ONE scorer: the phrase's stats blob
      for (uint32_t x = first + 1; x < j; ++x) {
        const irs_hip_term_scorer &a = ents[first], &w = ents[x];
        if ((a.kind & ~kFlags) != (w.kind & ~kFlags) || a.c0 != w.c0 || a.norm_const != w.norm_const ||
            a.norm_length != w.norm_length)
          return IRS_HIP_EINVAL;
      }
    }
    if (next) {
      sh.opens |= 1u << j;
      ++sh.n_phrases;
      first = j;
    }
  }
  if (sh.n_incl > IRS_HIP_MAX_PHRASE_TERMS || (kinds & kOthers)) return IRS_HIP_EUNSUPPORTED;
  return IRS_HIP_OK;
}

// A tree query (some entry carries IRS_HIP_TREE_NODE): tree_compile states what create takes
int tree_unit_shape(const irs_hip_query& in, const irs_hip_term_scorer* ents, UnitShape& sh,
                    std::vector<uint32_t>& excl, TreeTable& tab) {
  excl.clear();
  sh = UnitShape{};
  sh.tree = true;
  if (in.k == 0 || in.k > IRS_HIP_MAX_K || in.merge > IRS_HIP_MERGE_MIN) return IRS_HIP_EINVAL;
  if (const int rc = tree_compile(in, ents, tab)) return rc;
  sh.op = OpClass(in.op);
  sh.n_incl = sh.n_words = tab.n_leaves;
  return IRS_HIP_OK;
}

// Shape of query `in` in one segment.  Reads the query, the segment's entries `terms` and its term
// table; fills `sh` and `excl` (the present excluded terms; a tree query: `tab`); writes nothing of
// the batch.
int unit_shape(const irs_hip_query& in, const irs_hip_term_scorer* terms, uint32_t n_entries,
               const irs_hip_segment* seg, UnitShape& sh, std::vector<uint32_t>& excl, TreeTable& tab) {
  if (uint64_t(in.first_term) + in.n_terms > n_entries) return IRS_HIP_EINVAL;
  const irs_hip_term_scorer* ents = terms + in.first_term;
  sh = UnitShape{};
  int32_t kinds = 0;   // every included entry's kind OR-ed together: the flags some entry carries
  while (sh.n_incl < in.n_terms && ents[sh.n_incl].kind != IRS_HIP_EXCLUDE) kinds |= ents[sh.n_incl++].kind;
  // a node entry, among the included entries or behind the first IRS_HIP_EXCLUDE one: a tree query
  int32_t behind = 0;
  for (uint32_t j = sh.n_incl; j < in.n_terms; ++j) behind |= ents[j].kind;
  if ((kinds | behind) & IRS_HIP_TREE_NODE) return tree_unit_shape(in, ents, sh, excl, tab);
  sh.n_excl = in.n_terms - sh.n_incl;
  auto flagged = [&](int32_t flag) {
    bool any = false;
    for (uint32_t j = 0; j < sh.n_incl; ++j) any = any || (ents[j].kind & flag) != 0;
    return any;
  };
  // a variadic phrase (IRS_HIP_PHRASE_ALT members): up to IRS_HIP_MAX_PHRASE_ENTRIES entries
  sh.variadic = in.op == IRS_HIP_OP_PHRASE && flagged(IRS_HIP_PHRASE_ALT);
  if (sh.variadic && sh.n_incl > IRS_HIP_MAX_PHRASE_ENTRIES) return IRS_HIP_EUNSUPPORTED;
  sh.op = OpClass(in.op);
  // an Or of clauses (IRS_HIP_CLAUSE_AND members): clause_shape_ok states what create takes
  sh.clause = (kinds & IRS_HIP_CLAUSE_AND) != 0;
  if (sh.clause && clause_shape_ok(in, ents, sh.n_incl, sh.n_excl) == IRS_HIP_EINVAL) return IRS_HIP_EINVAL;
  if ((in.op != IRS_HIP_OP_OR && in.op != IRS_HIP_OP_AND && in.op != IRS_HIP_OP_MINMATCH && !sh.phrase() && !sh.wide()) ||
      sh.n_incl == 0 || in.merge > IRS_HIP_MERGE_MIN || (sh.phrase() && in.merge != IRS_HIP_MERGE_SUM) ||
      (!sh.phrase() && (kinds & (IRS_HIP_PHRASE_NEXT | IRS_HIP_PHRASE_OR))) ||
      (!sh.wide() && !sh.clause && sh.n_incl > IRS_HIP_MAX_TERMS) || sh.n_excl > IRS_HIP_MAX_EXCLUDED || in.k == 0 ||
      in.k > IRS_HIP_MAX_K)
    return IRS_HIP_EINVAL;
  sh.n_words = sh.n_incl;
  if (sh.clause)
    if (const int rc = clause_shape_ok(in, ents, sh.n_incl, sh.n_excl)) return rc;
  if (sh.wide())
    if (const int rc = wide_shape_ok(in, sh)) return rc;
  if (sh.phrase())
    if (const int rc = phrase_alternatives(ents, sh)) return rc;
  if (sh.phrase() && !sh.disj)
    if (const int rc = phrase_chain(ents, sh)) return rc;
  if (sh.phrase())
    if (const int rc = phrase_behind(ents, sh)) return rc;
  // a grouped conjunction: an And whose entries with IRS_HIP_GROUP_ALT are more members of the
  // group (an Or of by_term) opened by the nearest entry before them without it
  sh.grouped = in.op == IRS_HIP_OP_AND && flagged(IRS_HIP_GROUP_ALT);
  if (sh.grouped && (ents[0].kind & IRS_HIP_GROUP_ALT)) return IRS_HIP_EINVAL;
  // excluded terms: the docs of those present here leave the unit's matches (exclusion.hpp); an
  // absent one has no effect (boolean_query.cpp:131-134)
  excl.clear();
  for (uint32_t j = sh.n_incl; j < in.n_terms; ++j) {
    const irs_hip_term_scorer& ts = ents[j];
    if (ts.kind != IRS_HIP_EXCLUDE || (ts.term != IRS_HIP_NO_TERM && ts.term >= seg->dev.num_terms))
      return IRS_HIP_EINVAL;
    if (ts.term != IRS_HIP_NO_TERM && seg->terms[ts.term].docs_count) excl.push_back(ts.term);
  }
  return IRS_HIP_OK;
}

// A batch holds phrase queries only, or none: its first unit decides (commit_unit: b->phrase)
int phrase_only_rule(const irs_hip_batch* b, uint32_t q, const UnitShape& sh) {
  return q == 0 || sh.phrase() == b->phrase ? IRS_HIP_OK : IRS_HIP_EUNSUPPORTED;
}

// A phrase's parts and what its segment must hold
int phrase_parts_ok(const irs_hip_term_scorer* ents, const UnitShape& sh, const irs_hip_segment* seg) {
  uint32_t n_parts = 0;
  for (uint32_t j = 0; j < sh.n_incl; ++j) n_parts += (ents[j].kind & IRS_HIP_PHRASE_ALT) ? 0u : 1u;
  if (n_parts > IRS_HIP_MAX_PHRASE_TERMS || (ents[0].kind & IRS_HIP_PHRASE_ALT) || ents[0].phrase_offset != 0)
    return IRS_HIP_EINVAL;
  // FixedPhraseQuery needs FREQ | POS (phrase_query.cpp:63-66)
  return seg->dev.pos ? IRS_HIP_OK : IRS_HIP_EUNSUPPORTED;
}

// API scorer kind -> device Kind on a segment's norm column, with the scorer's argument checks
int device_kind(int32_t kind, const irs_hip_term_scorer& ts, const DevSegment& dev, int32_t* out) {
  const bool norms = dev.norms != nullptr;
  const bool legacy = norms && dev.norm_legacy;
  switch (kind) {
    case IRS_HIP_SCORE_BM25:
      *out = !norms ? kBM25One : legacy ? kBM25Legacy : (dev.norm_width == 1 ? kBM25Tiny : kBM25Wide);
      return ts.norm_const + ts.norm_length > 0.f ? IRS_HIP_OK : IRS_HIP_EINVAL;
    case IRS_HIP_SCORE_BM15:
      *out = kBM15;
      return ts.norm_const > 0.f ? IRS_HIP_OK : IRS_HIP_EINVAL;
    case IRS_HIP_SCORE_BM1: *out = kBM1; return IRS_HIP_OK;
    case IRS_HIP_SCORE_TFIDF: *out = kTfidf; return IRS_HIP_OK;
    case IRS_HIP_SCORE_TFIDF_NORM:
      *out = !norms ? kTfidf : legacy ? kTfidfLegacy : (dev.norm_width == 1 ? kTfidfTiny : kTfidfWide);
      return IRS_HIP_OK;
    default: return IRS_HIP_EINVAL;
  }
}

// The smallest score one posting of the term can have (tf = 1, longest doc)
double posting_smin(const DevQTerm& qt) {
  const double c0 = qt.c0, nc = qt.norm_const, nl = qt.norm_length;
  switch (qt.kind) {
    case kBM1: return c0;
    case kBM15: return c0 - c0 / (1.0 + 1.0 / nc);
    case kBM25Tiny: return c0 - c0 / (1.0 + 1.0 / (nc + nl * 255.0));
    case kBM25One: return c0 - c0 / (1.0 + 1.0 / (nc + nl));
    case kTfidf: return c0;
    case kTfidfTiny: return c0 / std::sqrt(255.0);
    default: return 0.0;  // wide norms: unbounded below
  }
}

// Rows of the unit: its included entries checked, those present in the segment as DevQTerm rows in
// s.row (table slots not assigned yet), the score bounds and the work they stand for in `u`
int unit_rows(const irs_hip_term_scorer* ents, const irs_hip_segment* seg, Unit& u, UnitScratch& s) {
  const UnitShape& sh = u.shape;
  s.row.clear();
  s.smins.clear();
  s.row_group.clear();
  // an Or of clauses: a clause with an absent member is empty in this segment — none of its entries
  // is a row (bit c of `dead`)
  uint32_t clause_of[IRS_HIP_MAX_TERMS];   // (written and read for such a unit only)
  uint32_t dead = 0;
  if (sh.clause) {
    u.n_groups = clause_of_entries(ents, sh.n_incl, clause_of);
    for (uint32_t j = 0; j < sh.n_incl; ++j) {
      const uint32_t t = ents[j].term;
      if (t == IRS_HIP_NO_TERM || (t < seg->dev.num_terms && seg->terms[t].docs_count == 0)) dead |= 1u << clause_of[j];
    }
    u.groups_found = ((1u << u.n_groups) - 1u) & ~dead;
  }
  // an Or of phrases: a phrase with an absent word is dropped in this segment the same way — none of
  // its entries is a row (bit j of `gone`: entry j belongs to such a phrase)
  uint32_t gone = 0;
  if (sh.disj) {
    for (uint32_t lo = 0; lo < sh.n_incl;) {
      uint32_t end = lo + 1;
      while (end < sh.n_incl && !((sh.opens >> end) & 1u)) ++end;
      bool absent = false;
      for (uint32_t j = lo; j < end; ++j) {
        const uint32_t t = ents[j].term;
        absent = absent || t == IRS_HIP_NO_TERM || (t < seg->dev.num_terms && seg->terms[t].docs_count == 0);
      }
      if (absent) gone |= ((1u << end) - 1u) & ~((1u << lo) - 1u);
      lo = end;
    }
  }
  // a tree query: its leaves, wherever they stand; a negated leaf is a row without a scorer of its
  // own — it carries the scorer values of the tree's first positive leaf (one signature, one stream
  // per term: plan_join.h build_streams) and a boost of 0
  uint32_t tree_ref = 0;
  while (sh.tree && tree_ref + 1u < sh.n_incl && ((s.tab.negated >> tree_ref) & 1u)) ++tree_ref;
  for (uint32_t j = 0; j < sh.n_incl; ++j) {
    const bool negated = sh.tree && ((s.tab.negated >> j) & 1u);
    irs_hip_term_scorer leaf{};
    if (negated) {
      leaf = ents[s.tab.leaf_at[tree_ref]];
      leaf.term = ents[s.tab.leaf_at[j]].term;
      leaf.c0 = 0.f;
    }
    const irs_hip_term_scorer& ts = negated ? leaf : sh.tree ? ents[s.tab.leaf_at[j]] : ents[j];
    const bool behind = sh.phrase() && j >= sh.n_words;   // (a required or an optional term)
    const bool optional = behind && sh.behind == Behind::kOptional;   // (no part of the phrase: absent, it is dropped)
    const int32_t kind = sh.phrase() ? (ts.kind & ~(IRS_HIP_PHRASE_ALT | IRS_HIP_PHRASE_REQUIRED | IRS_HIP_PHRASE_OPTIONAL |
                                                  IRS_HIP_PHRASE_NEXT | IRS_HIP_PHRASE_OR))
                         : sh.grouped ? (ts.kind & ~IRS_HIP_GROUP_ALT)
                         : sh.clause ? (ts.kind & ~IRS_HIP_CLAUSE_AND) : ts.kind;
    if (sh.grouped && !(ts.kind & IRS_HIP_GROUP_ALT)) ++u.n_groups;
    if (sh.phrase())
      if (const int rc = u.parts.enter(ents, j, (ts.kind & IRS_HIP_PHRASE_ALT) != 0, optional)) return rc;
    DevQTerm qt{};
    qt.term = ts.term;
    qt.c0 = ts.c0;
    qt.norm_const = ts.norm_const;
    qt.norm_length = ts.norm_length;
    qt.cache_id = kMaxCaches;
    qt.pad0 = (sh.phrase() && !behind) ? ts.phrase_offset : 0u;
    if (sh.tree) qt.pad0 = j | (negated ? kTreeNegated : 0u);   // (the leaf's bit: an absent leaf keeps it and never sets it)
    if (ts.term != IRS_HIP_NO_TERM && ts.term >= seg->dev.num_terms) return IRS_HIP_EINVAL;
    // (a zero boost is legal: every posting then scores 0 — the fixed-point accumulators
    // still mark the doc as matched, and sums below kMaxTerms units come back as 0)
    if (!(ts.c0 >= 0.f) || !std::isfinite(ts.c0)) return IRS_HIP_EINVAL;
    if (const int rc = device_kind(kind, ts, seg->dev, &qt.kind)) return rc;
    // (BM25 family: a posting scores below its boost c0 whatever the segment holds; the
    // TF-IDF bound grows with the segment's largest frequency)
    u.same_bound = u.same_bound && (kind == IRS_HIP_SCORE_BM25 || kind == IRS_HIP_SCORE_BM15 || kind == IRS_HIP_SCORE_BM1);
    u.upper_all += double(ts.c0);
    // TermQuery::execute: no term state in this segment -> empty iterator (term_query.cpp:41-43)
    if (qt.term == IRS_HIP_NO_TERM || seg->terms[qt.term].docs_count == 0) {
      // (a phrase / grouped conjunction: an absent member is dropped; a part / group without
      // a present one empties the unit, unit_need)
      if (!sh.phrase() && !sh.grouped && !sh.clause && !sh.tree) u.absent = true;
      continue;
    }
    if (sh.clause) {
      if ((dead >> clause_of[j]) & 1u) continue;
      s.row_group.push_back(clause_of[j]);
    }
    if (sh.disj) {
      if ((gone >> j) & 1u) continue;
      if ((sh.opens >> j) & 1u) u.disj_opens |= 1u << s.row.size();
    }
    if (sh.grouped) {
      u.groups_found |= 1u << (u.n_groups - 1u);
      s.row_group.push_back(u.n_groups - 1u);
    }
    if (sh.phrase() && !optional) u.parts.present(s.row.size());
    const DevTerm& t = seg->terms[qt.term];
    qt.pad1 = t.tf_bound;
    s.smins.push_back(posting_smin(qt));
    if (!negated) u.min_score = std::min(u.min_score, s.smins.back());
    const bool tfidf = qt.kind == kTfidf || qt.kind == kTfidfTiny || qt.kind == kTfidfWide || qt.kind == kTfidfLegacy;
    // (a phrase's frequency is at most the sum of the tf_bound of its first part's members; the
    // sum over every row of sqrt(tf_bound) bounds the square root of that, sqrt being subadditive)
    u.upper += tfidf ? double(qt.c0) * std::sqrt(double(t.tf_bound)) : double(qt.c0);
    u.postings += t.docs_count;
    u.alg_bytes += uint64_t(t.blocks_bytes) + t.tail_bytes;
    if (needs_norm(qt.kind)) u.alg_bytes += uint64_t(t.docs_count) * seg->dev.norm_width;
    s.row.push_back(qt);
    if (!behind) ++u.parts.word_rows;
  }
  return IRS_HIP_OK;
}

// k_vphrase takes no required or optional terms, k_phrase_and no variadic parts, a batch runs on
// k_phrase_and or on k_phrase_or; k_phrases_and (several phrases in one And) takes plain phrases
// and required terms, no variadic parts, no optional terms; k_phrases_or (several phrases in one Or)
// plain phrases only: the units so far (BlockWork's flags,
// commit_unit) and this one
int phrase_kernel_rule(const irs_hip_batch* b, const UnitShape& sh) {
  if (!sh.phrase()) return IRS_HIP_OK;
  const bool variadic = b->blocks.variadic || sh.variadic;
  const bool required = b->blocks.required || sh.behind == Behind::kRequired;
  const bool optional = b->blocks.optional || sh.behind == Behind::kOptional;
  const bool several = b->blocks.several || sh.several;
  // (k_phrases_or — several phrases in one Or — takes plain phrases and nothing else)
  const bool disj = b->blocks.disj || sh.disj;
  return (variadic && (required || optional || several)) || (optional && (required || several)) ||
                 (disj && (variadic || required || optional || several))
             ? IRS_HIP_EUNSUPPORTED : IRS_HIP_OK;
}

// How many of the (present) terms a doc must match.  Or: 1.  And: all, and one absent term empties
// it (MakeScoreAdapters<true>, boolean_query.cpp:50-53); a grouped one: a group without a present
// member does.  MinMatch(m) (MinMatchQuery::execute, boolean_query.cpp:212-247): m > #sub-queries
// or m > #present -> empty; m == #present -> conjunction; m <= 1 -> disjunction; otherwise the
// min-match block disjunction: every matching term scores, docs with < m matches drop.  A wide
// query: fewer than min_match present entries empty it in this segment (MultiTermQuery::execute,
// multiterm_query.cpp:163-167).  A phrase: no phrase state for a segment lacking one of the terms
// (phrase_filter.cpp:254-258), or a part with none of its members (:370-379); its scorer is one
// stats blob: every word's entry must carry the same values (a required term carries its own).
// An empty unit loses its rows.
int unit_need(const irs_hip_query& in, Unit& u, UnitScratch& s) {
  const UnitShape& sh = u.shape;
  const uint32_t n_rows = uint32_t(s.row.size());
  u.need = 1;
  // a tree query: what a doc needs is its node table's to say (an And with an absent member, a
  // min-match with too few present children: no doc's mask satisfies them)
  if (sh.tree) return IRS_HIP_OK;
  // an Or of clauses: min_match counts the clauses (MinMatchQuery::execute over the children)
  const uint32_t n_live = sh.clause ? uint32_t(__builtin_popcount(u.groups_found)) : n_rows;
  const uint32_t n_subs = sh.clause ? u.n_groups : sh.n_incl;
  switch (sh.op) {
    case OpClass::kOr: break;
    case OpClass::kAnd:
      u.need = (sh.grouped ? u.groups_found != (1u << u.n_groups) - 1u : u.absent) ? kEmptyUnit : n_rows;
      break;
    case OpClass::kMinMatch:
      // Or::prepare turns min_match_count == 0 into the all-docs filter
      // (boolean_filter.cpp:213): not a posting-list query, not on this path
      if (in.min_match == 0) return IRS_HIP_EUNSUPPORTED;
      u.need = (in.min_match > n_subs || in.min_match > n_live) ? kEmptyUnit : in.min_match;
      break;
    case OpClass::kWide: u.need = in.min_match > n_rows ? kEmptyUnit : in.min_match; break;
    case OpClass::kPhrase:
      // (several phrases: every word is a part, so an absent word of any phrase empties the unit;
      // one scorer per PHRASE was checked on the entries, phrase_chain)
      // (an Or of phrases: the rows of its present phrases; none present empties it)
      u.need = (sh.disj ? !s.row.empty() : u.parts.complete()) ? 1u : kEmptyUnit;
      for (uint32_t r = 0; r < u.parts.word_rows && !sh.several && !sh.disj; ++r) {
        const DevQTerm& qt = s.row[r];
        if (qt.kind != s.row[0].kind || qt.c0 != s.row[0].c0 || qt.norm_const != s.row[0].norm_const ||
            qt.norm_length != s.row[0].norm_length)
          return IRS_HIP_EINVAL;
      }
      break;
  }
  if (u.need == kEmptyUnit) s.row.clear();
  return IRS_HIP_OK;
}

// MakeConjunction sorts its children by cost (conjunction.hpp:450-453): the groups of a grouped And,
// by the sum of their members' docs_count (the cheapest leads; the members keep their order).
// Returns `opens` of the sorted rows.
uint32_t sort_groups(const irs_hip_segment* seg, uint32_t n_groups, UnitScratch& s) {
  std::vector<uint64_t> cost(n_groups, 0);
  for (size_t r = 0; r < s.row.size(); ++r) cost[s.row_group[r]] += seg->terms[s.row[r].term].docs_count;
  std::vector<uint32_t> order(n_groups);
  for (uint32_t g = 0; g < n_groups; ++g) order[g] = g;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cost[x] < cost[y]; });
  std::vector<DevQTerm> sorted;
  uint32_t opens = 0;
  for (uint32_t g : order) {
    bool first = true;
    for (size_t r = 0; r < s.row.size(); ++r) {
      if (s.row_group[r] != g) continue;
      if (first) opens |= 1u << sorted.size();
      first = false;
      sorted.push_back(s.row[r]);
    }
  }
  s.row.swap(sorted);
  return opens;
}

// How the unit runs: its op word (score.h "DevQuery::op"), its rows in the order the kernels want
// them, and whether match counts may ride in its 32-bit accumulators
void unit_run(const irs_hip_query& in, const irs_hip_segment* seg, Unit& u, UnitScratch& s) {
  const UnitShape& sh = u.shape;
  std::vector<DevQTerm>& row = s.row;
  // A doc that exists matches at least `need` terms: c matched postings score at least
  // c times the mean of the `need` smallest per-term minima — the score below which no
  // posting of a matching doc falls ON AVERAGE, which is what bounds the relative error of
  // a fixed-point sum that loses a constant per posting
  if (u.need > 1 && u.need != kEmptyUnit && !s.smins.empty() && !sh.phrase()) {
    std::sort(s.smins.begin(), s.smins.end());
    double sm = 0.0;
    for (uint32_t i = 0; i < u.need && i < s.smins.size(); ++i) sm += s.smins[i];
    u.min_score = sm / double(u.need);
  }
  uint32_t run = kRunTiles, op_need = 0;
  if (sh.wide()) {
    // lane j = term j of k_wide_pilot / k_wide_score; the match count rides in the low bits of
    // the unit's own 64-bit sums whatever min_match is
    run = kRunWide;
    op_need = u.need;
  } else if (sh.clause) {
    // lane j = row j of k_clause_pilot / k_clause_score; every row carries the need-mask of its
    // clause (DevQTerm::pad0), `need` counts clauses
    run = kRunClause;
    op_need = u.need;
    uint32_t masks[IRS_HIP_MAX_TERMS] = {};
    clause_masks(s.row_group.data(), row.size(), masks);
    for (size_t r = 0; r < row.size(); ++r) row[r].pad0 = masks[r];
  } else if (sh.tree) {
    // lane j = row j of k_tree_pilot / k_tree_score; every row carries its leaf's bit
    // (DevQTerm::pad0, unit_rows), `need` counts the records of the unit's node table
    run = kRunTree;
    op_need = s.tab.n_nodes;
  } else if (sh.grouped) {   // always block driven (conj_any.h), whatever the number of rows
    if (!row.empty()) u.group_opens = sort_groups(seg, u.n_groups, s);
    run = kRunConj;
    op_need = uint32_t(row.size());
  } else if (u.need > 1 && !row.empty() && !sh.phrase()) {
    op_need = u.need;
    if (u.need == row.size()) {
      // MakeConjunction sorts by cost (conjunction.hpp:450-453): the cheapest leads, and
      // the scores are summed in that order
      std::stable_sort(row.begin(), row.end(), [&](const DevQTerm& x, const DevQTerm& y) {
        return seg->terms[x.term].docs_count < seg->terms[y.term].docs_count;
      });
      run = kRunConj;
    } else {
      run = kRunCount;
      u.any_and = true;
    }
  }
  // The filter's ScoreMergeType (boolean_filter.hpp:39-43).  One sub-iterator: its score as
  // it is (MakeDisjunction :1422-1426, MakeConjunction :444).  kMin in a disjunction merges
  // with the 0 of every sub-iterator that is not on the doc (basic_disjunction,
  // disjunction.hpp:338-351) resp. with the zeroed score buffer (block_disjunction
  // :1308-1351): two sub-iterators -> min where both match, else 0; more (or the
  // min-match block disjunction) -> 0 for every doc.
  uint32_t merge = row.size() > 1 && !sh.clause && !sh.tree ? in.merge : uint32_t(IRS_HIP_MERGE_SUM);
  bool min_both = false;
  if (merge == IRS_HIP_MERGE_MIN && run != kRunConj) {
    if (run == kRunTiles && row.size() == 2) {
      min_both = true;
      u.any_and = true;   // (the per-doc match counters tell "both")
    } else {
      for (DevQTerm& qt : row) qt.c0 = 0.f;
      u.upper = 0.0;
      u.min_score = 0.0;
      merge = IRS_HIP_MERGE_SUM;
    }
  }
  u.op = make_op(run, op_need, merge, min_both);
  // match counts in the low bits of a 32-bit accumulator (join.h COUNT) round every posting
  // to 16 fixed-point units (+-8): relative to any doc's score that is at most
  // 8 * upper / (2^29 * min_score) — allowed while it stays below 2e-6
  u.count_precise = !sh.wide() && !sh.clause && !sh.tree && row.size() <= kJoinCountTerms && u.min_score > 0.0 && u.upper > 0.0 &&
                    u.upper / u.min_score <= 125.0;
}

// Table slots (kernels.h "table_kind"): one per distinct (kind, norm_const, norm_length).  Returns
// the slots in use.
uint32_t assign_table_slots(std::vector<DevQTerm>& row) {
  uint32_t n_caches = 0;
  float cnc[kMaxCaches], cnl[kMaxCaches];
  int32_t ckind[kMaxCaches];
  for (DevQTerm& qt : row) {
    if (!table_kind(qt.kind)) continue;
    uint32_t c = 0;
    for (; c < n_caches; ++c)
      if (ckind[c] == qt.kind && cnc[c] == qt.norm_const && cnl[c] == qt.norm_length) break;
    if (c == n_caches && n_caches < kMaxCaches) {
      ckind[c] = qt.kind;
      cnc[c] = qt.norm_const;
      cnl[c] = qt.norm_length;
      ++n_caches;
    }
    qt.cache_id = c < kMaxCaches ? c : kMaxCaches;
  }
  return n_caches;
}

// Fixed-point scale of the unit's scores: upper < 2^exp.  32-bit accumulators (2^(30-exp) units)
// lose at most one unit per posting, i.e. <= upper / (2^29 * min_score) relative to any doc's
// score: used only while that stays below 2e-6 for every query of the batch (Unit::acc64).
int unit_scale(Unit& u, bool has_rows) {
  const UnitShape& sh = u.shape;
  u.upper *= 1.0 + 1e-6;
  if (!has_rows) return IRS_HIP_OK;   // (bin_scale 0, no shared bound, exp 0)
  if (u.upper == 0.0) u.upper = 1.0;   // every boost is 0: all scores are 0
  if (!(u.upper > 0.0 && std::isfinite(u.upper))) return IRS_HIP_EUNSUPPORTED;
  u.bin_scale = float(double(kBins) / u.upper);
  // (irs_hip_batch_set_comm) the bound every segment of the index computes alike
  if (u.same_bound && !sh.phrase() && !sh.wide() && !sh.clause && !sh.tree && u.upper_all > 0.0 &&
      u.upper_all * (1.0 + 1e-6) >= u.upper && std::isfinite(u.upper_all))
    u.shared_upper = u.upper_all * (1.0 + 1e-6);
  (void)std::frexp(u.upper, &u.exp);
  if (u.exp < -60 || u.exp > 60) return IRS_HIP_EUNSUPPORTED;
  // (grouped units score in floats, block driven: the flat units' accumulators are theirs)
  // (wide units, Ors of clauses and tree queries carry 64-bit sums of their own and never ask)
  u.acc64 = !sh.grouped && !sh.wide() && !sh.clause && !sh.tree && (!(u.min_score > 0.0) || u.upper / u.min_score > 1000.0);
  return IRS_HIP_OK;
}

// The finished unit q into the batch: its DevQuery and rows, its entries in the side tables of its
// path, and the batch-wide facts it bears on (phrase, blocks.variadic / required / optional, acc32,
// jt, k_max, tiles.any_and, postings, alg_bytes).  Nothing else of create writes these per unit.
void commit_unit(irs_hip_batch* b, uint32_t q, const irs_hip_query& in, const irs_hip_segment* seg,
                 const Unit& u, UnitScratch& s, std::vector<uint32_t>& grouped_units) {
  const UnitShape& sh = u.shape;
  const bool has_rows = !s.row.empty();
  DevQuery& dq = b->queries[q];
  dq.k = in.k;
  dq.seg = q / b->nq_user;
  dq.op = u.op;
  dq.n_caches = u.n_caches;
  dq.n_terms = uint32_t(s.row.size());
  dq.first_term = uint32_t(b->qterms.size());
  dq.bin_scale = u.bin_scale;
  // (64-bit accumulators; widen_fixed_point, once the whole batch is known)
  dq.fx_mul = std::ldexp(1.f, 29 - u.exp);
  dq.fx_inv = std::ldexp(1.f, u.exp - 61);
  // the unit's masked docs: its segment's deleted ones, and for a unit with present excluded
  // terms a mask of its own (dead | their docs), shared by the units with the same terms
  // (build_masks, behind the loop — and again when the batch gets doc sets)
  dq.dead = seg->dev.dead;
  b->excl.unit_live[q] = has_rows;
  b->alg_bytes += u.alg_bytes + 8ull * in.k;
  if (has_rows && !s.excl.empty()) {
    std::sort(s.excl.begin(), s.excl.end());
    s.excl.erase(std::unique(s.excl.begin(), s.excl.end()), s.excl.end());
    b->excl.unit_terms.insert(b->excl.unit_terms.end(), s.excl.begin(), s.excl.end());
    // (what k_excl_mask reads for the unit: the excluded terms' doc blocks)
    for (uint32_t t : s.excl) b->alg_bytes += uint64_t(seg->terms[t].blocks_bytes) + seg->terms[t].tail_bytes;
  }
  b->excl.unit_first.push_back(uint32_t(b->excl.unit_terms.size()));
  if (q == 0) b->phrase = sh.phrase();
  if (sh.phrase()) {
    b->blocks.variadic = b->blocks.variadic || sh.variadic;
    b->blocks.required = b->blocks.required || sh.behind == Behind::kRequired;
    b->blocks.optional = b->blocks.optional || sh.behind == Behind::kOptional;
    b->blocks.n_phrase[q] = u.parts.word_rows;
    if (has_rows) b->blocks.opens[q] = u.parts.opens;
    b->blocks.several = b->blocks.several || sh.several;
    if (sh.several) ++b->blocks.n_several;
    if (has_rows) b->blocks.phrase_opens[q] = sh.disj ? u.disj_opens : sh.opens;   // (one phrase: bit 0)
    b->blocks.disj = b->blocks.disj || sh.disj;
    if (sh.disj) ++b->blocks.n_disj;
  } else if (sh.wide()) {
    b->wide.units.push_back(q);
  } else if (sh.clause) {
    b->clause.units.push_back(q);
  } else if (sh.tree) {
    b->tree.units.push_back(q);
    b->tree.nodes.insert(b->tree.nodes.end(), s.tab.node, s.tab.node + kTreeMaxNodes);
  } else if (sh.grouped) {
    if (has_rows) {
      b->any.opens[q] = u.group_opens;
      grouped_units.push_back(q);
    }
  } else {
    (query_run(u.op) == kRunConj ? b->all_conj_units : b->all_tile_units).push_back(q);
  }
  b->count_precise[q] = u.count_precise;
  b->groups.upper[q] = u.shared_upper;
  b->tiles.any_and = b->tiles.any_and || u.any_and;
  if (u.acc64) b->acc32 = false;
  b->postings += u.postings;
  b->qterms.insert(b->qterms.end(), s.row.begin(), s.row.end());
  if (!sh.wide() && !sh.clause && !sh.tree) b->jt = std::max(b->jt, dq.n_terms);   // (the plan table's term slots)
  b->k_max = std::max(b->k_max, in.k);
}

// Where every flat unit allows 32-bit accumulators (b->acc32, final behind the loop): 2^(30-exp)
// units instead of commit_unit's 2^(29-exp) high words.  Wide units, Ors of clauses and tree
// queries keep their 64-bit sums.
void widen_fixed_point(irs_hip_batch* b) {
  if (!b->acc32) return;
  for (DevQuery& dq : b->queries) {
    if (unit_is_wide(dq) || unit_is_clause(dq) || unit_is_tree(dq)) continue;
    dq.fx_mul = std::ldexp(dq.fx_mul, 1);
    dq.fx_inv = std::ldexp(dq.fx_inv, 31);
  }
}

// The TERM PASS of a batch with optional terms (IRS_HIP_PHRASE_OPTIONAL; batch.h irs_hip_batch::opt):
// a batch of its own over the same segments and queries — per query its optional entries as a plain
// Or (the flag taken off, the IRS_HIP_EXCLUDE entries behind them; a query without optional entries:
// one absent term, an empty unit) — whose units are restricted to the rows of b->d_taken, the doc
// sets k_phrase_or takes the phrase's matches out of.  Masked units run as work items (k_items_*,
// k_pilot, k_score) and never join streams.
int create_term_pass(irs_hip_batch* b, irs_hip_segment* const* segs, uint32_t n_segs,
                     const irs_hip_query* queries, const irs_hip_term_scorer* all_terms,
                     uint32_t n_entries) {
  std::vector<irs_hip_query> cq(b->nq_user);
  std::vector<uint32_t> from;   // the term pass's entries: their indices in the caller's, ~0u: the absent one
  for (uint32_t q = 0; q < b->nq_user; ++q) {
    const irs_hip_query& in = queries[q];
    cq[q] = in;
    cq[q].op = IRS_HIP_OP_OR;
    cq[q].min_match = 1;
    cq[q].first_term = uint32_t(from.size());
    bool any = false;
    for (uint32_t j = 0; j < in.n_terms; ++j) {
      const int32_t kind = all_terms[in.first_term + j].kind;
      const bool optional = kind != IRS_HIP_EXCLUDE && (kind & IRS_HIP_PHRASE_OPTIONAL) != 0;
      if (optional || (any && kind == IRS_HIP_EXCLUDE)) from.push_back(in.first_term + j);
      any = any || optional;
    }
    if (!any) from.push_back(~0u);
    cq[q].n_terms = uint32_t(from.size()) - cq[q].first_term;
  }
  std::vector<irs_hip_term_scorer> ct(from.size() * n_segs);
  for (uint32_t s = 0; s < n_segs; ++s) {
    for (size_t i = 0; i < from.size(); ++i) {
      irs_hip_term_scorer& t = ct[s * from.size() + i];
      if (from[i] == ~0u) {
        t = irs_hip_term_scorer{};
        t.term = IRS_HIP_NO_TERM;
        t.kind = IRS_HIP_SCORE_BM1;
      } else {
        t = all_terms[size_t(s) * n_entries + from[i]];
        if (t.kind != IRS_HIP_EXCLUDE) t.kind &= ~IRS_HIP_PHRASE_OPTIONAL;
        t.phrase_offset = 0;
      }
    }
  }
  if (const int rc = batch_create_multi_impl(segs, n_segs, cq.data(), b->nq_user, ct.data(),
                                             uint32_t(from.size()), &b->opt))
    return rc;
  b->opt->term_pass = true;
  uint32_t max_docs = 0;
  for (uint32_t s = 0; s < n_segs; ++s) max_docs = std::max(max_docs, segs[s]->dev.num_docs);
  b->taken_words = uint64_t(max_docs) / 64u + 1u;
  std::vector<uint32_t> row_of(b->nq);
  for (uint32_t u = 0; u < b->nq; ++u) row_of[u] = u;
  if (!b->d_taken.alloc(uint64_t(b->nq) * b->taken_words * 8u) ||
      !b->d_union_out.alloc(uint64_t(b->nq) * b->k_max * sizeof(Hit)) ||
      !b->d_union_count.alloc(uint64_t(b->nq) * 4u) || !b->d_union_hits.alloc(uint64_t(b->nq) * 8u))
    return IRS_HIP_ENOMEM;
  return batch_set_doc_sets_impl(b->opt, b->d_taken.p, false, b->nq, b->taken_words, row_of.data());
}

}  // namespace
