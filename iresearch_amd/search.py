"""Host-side mirror of the reference interfaces on the hot path, above the C ABI.

Names follow IResearch: a *segment* holds posting lists of *terms*; a *filter*
(`by_term`, `Or`, `And`) is `prepare`d against an *index* (all segments) to
collect statistics, then executed per segment; a *scorer* (`BM25`, `TFIDF`)
turns statistics into per-term score functions.

  irs::BM25::collect          core/search/bm25.cpp:366-410     -> BM25.collect
  irs::TFIDF::collect         core/search/tfidf.cpp:263-278    -> TFIDF.collect
  by_term::prepare            core/search/term_filter.cpp:92-129 -> prepare()
  by_phrase (FixedPrepareCollect) core/search/phrase_filter.cpp:212-293 -> prepare()
  by_terms::prepare           core/search/terms_filter.cpp:110-153 -> prepare()
  filter::prepared::execute   core/search/filter.hpp:52-78     -> SegmentReader.execute()
  utils/index-search.cpp:719-787 (heap over all segments)     -> Index.search()

This module holds no posting decode or scoring arithmetic of its own beyond the
per-term statistics (which the reference also computes on the CPU once per
query): everything per posting happens in libirs_hip.so on the GPU.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field, replace

import numpy as np

from . import _lib
from ._lib import (EXCLUDE, HIT, NO_TERM, OP_AND, OP_MINMATCH, OP_MULTITERM, OP_OR, OP_PHRASE, PHRASE_ALT, PHRASE_NEXT, PHRASE_OPTIONAL, PHRASE_OR, PHRASE_REQUIRED, CLAUSE_AND, TREE_NODE, QUERY, SCORE_BM1, SCORE_BM15, SCORE_BM25,
                   SCORE_TFIDF, SCORE_TFIDF_NORM, TERM_META, TERM_SCORER, SegmentDesc)

f32 = np.float32


# ------------------------------------------------------------------ scorers --

@dataclass(frozen=True)
class TermStats:
    """BM25Stats minus the cache (bm25.hpp:48-57) / TFIDFStats."""
    idf: np.float32
    norm_const: np.float32 = f32(0)
    norm_length: np.float32 = f32(0)


class BM25:
    """irs::BM25 (bm25.hpp:59-117): k = 1.2, b = 0.75 by default."""

    def __init__(self, k: float = 1.2, b: float = 0.75):
        self.k, self.b = f32(k), f32(b)

    def collect(self, docs_with_field: int, docs_with_term: int, total_term_freq: int):
        # bm25.cpp:381-383 — double log1p, then cast
        idf = f32(math.log1p((float(docs_with_field - docs_with_term) + 0.5) /
                             (float(docs_with_term) + 0.5)))
        if self.k == 0 or self.b == 0:  # !NeedsNorm() bm25.cpp:387-390
            return TermStats(idf, self.k, f32(0))
        kb = f32(self.k * self.b)
        norm_const = f32(self.k - kb)
        if total_term_freq and docs_with_field:
            avg_dl = f32(f32(total_term_freq) / f32(docs_with_field))
            norm_length = f32(kb / avg_dl)
        else:
            norm_length = kb
        return TermStats(idf, norm_const, norm_length)

    def term_scorer(self, st: TermStats, boost: float = 1.0):
        # BM1Context: num = boost * (k + 1) * idf (bm25.cpp:201)
        c0 = f32(f32(f32(boost) * f32(self.k + f32(1))) * st.idf)
        if self.k == 0:
            kind = SCORE_BM1
        elif self.b == 0:
            kind = SCORE_BM15
        else:
            kind = SCORE_BM25
        return kind, c0, st.norm_const, st.norm_length


class TFIDF:
    """irs::TFIDF (tfidf.hpp): with_norms == normalize()."""

    def __init__(self, with_norms: bool = False):
        self.with_norms = bool(with_norms)

    def collect(self, docs_with_field: int, docs_with_term: int, total_term_freq: int):
        return TermStats(f32(math.log1p((docs_with_field + 1.0) / (docs_with_term + 1.0))))

    def term_scorer(self, st: TermStats, boost: float = 1.0):
        c0 = f32(f32(boost) * st.idf)  # TFIDFContext: idf = boost * idf.value
        return (SCORE_TFIDF_NORM if self.with_norms else SCORE_TFIDF), c0, f32(0), f32(0)


# ------------------------------------------------------------------ filters --

@dataclass
class by_term:
    """irs::by_term on the benchmark field; `term` is the ordinal in the term table."""
    term: int
    boost: float = 1.0


# irs::ScoreMergeType (scorer.hpp:224-236) of a boolean filter: boolean_filter::merge_type()
MERGE_SUM, MERGE_MAX, MERGE_MIN = 0, 1, 2


@dataclass
class Or:
    """irs::Or; min_match > 1 is Or::min_match_count() (boolean_filter.hpp); `merge` its
    merge_type(); `boost` multiplies into the boosts of its terms (boolean_filter.cpp:153-154, 204).
    An Or of by_term and And-of-by_term children — a disjunction of clauses, `(a AND b) OR c`
    (IRS_HIP_CLAUSE_AND; min_match counts the children, merge SUM, at most 16 terms in all) — is
    taken by prepare(..., and_clauses=True).
    An Or of ONE by_phrase of plain terms and by_term children — a phrase or optional terms,
    `"new york" hotel cheap` (IRS_HIP_PHRASE_OPTIONAL; min_match <= 1, merge SUM, at most 8 words
    and terms in all) — is taken by prepare(..., optional_terms=True)."""
    subs: list
    min_match: int = 1
    merge: int = MERGE_SUM
    boost: float = 1.0

    @property
    def op(self):
        return OP_MINMATCH if self.min_match > 1 else OP_OR


@dataclass
class And:
    """irs::And of by_term and Or-of-by_term children (the Ors are groups: IRS_HIP_GROUP_ALT), or of
    ONE by_phrase of plain terms and by_term children — a phrase plus required terms,
    `+"new york" +hotel` (IRS_HIP_PHRASE_REQUIRED; merge SUM, at most 8 words and terms in all;
    prepare(..., required_terms=True)), or of two to four such phrases and by_term children —
    `+"new york" +"real estate"` (IRS_HIP_PHRASE_NEXT; merge SUM, at most 8 words and terms in all;
    prepare(..., phrase_conjunctions=True));
    Not children exclude docs either way; `boost` multiplies into the boosts of its children."""
    subs: list
    op: int = OP_AND
    min_match: int = 0
    merge: int = MERGE_SUM
    boost: float = 1.0


@dataclass
class by_terms:
    """irs::by_terms (by_terms_options, terms_filter.cpp:110-153): a set of (term, boost) and
    min_match, scored as MultiTermQuery::execute does (multiterm_query.cpp:114-181) — a doc matches
    when at least `min_match` of the terms present in its segment hold it, its score is the sum of
    the scores of the terms holding it.  `terms`: ordinals or (ordinal, boost) pairs, 1..64 of them
    (IRS_HIP_OP_MULTITERM); `boost` multiplies into every term's.  The same term twice scores
    twice."""
    terms: list
    min_match: int = 1
    boost: float = 1.0

    def pairs(self):
        """[(ordinal, boost)]"""
        return [(int(t[0]), float(t[1])) if isinstance(t, (tuple, list)) else (int(t), 1.0)
                for t in self.terms]

    def check(self):
        n = len(self.terms)
        if not 1 <= n <= _lib.MAX_WIDE_TERMS:
            raise ValueError("by_terms takes 1..%d terms, not %d" % (_lib.MAX_WIDE_TERMS, n))
        if not 1 <= int(self.min_match) <= n:
            raise ValueError("by_terms: min_match is 1..%d (the number of terms), not %d" %
                             (n, int(self.min_match)))


@dataclass
class by_phrase:
    """irs::by_phrase (by_phrase_options): `terms[i]` is part i — a term ordinal
    (push_back<by_term_options>) or a list of them: a part that stands for a set of terms, what a
    by_terms / by_prefix / by_wildcard / by_range visitor yields, in dictionary order (a variadic
    phrase, VariadicPrepareCollect); `offsets[i]` = position of part i relative to the first
    (default: consecutive words).  A phrase of plain terms may also be a child of an And, next to
    by_term children (required terms) and Nots (prepare(..., required_terms=True)), or of an Or
    next to by_term children (optional terms, prepare(..., optional_terms=True)).  Up to four
    phrases of plain terms may stand in one And (prepare(..., phrase_conjunctions=True)) or in
    one Or (prepare(..., phrase_disjunctions=True))."""
    terms: list
    offsets: list | None = None
    boost: float = 1.0

    def __post_init__(self):
        if self.offsets is None:
            self.offsets = list(range(len(self.terms)))
        if len(self.offsets) != len(self.terms) or (self.offsets and self.offsets[0] != 0):
            raise ValueError("offsets are relative to the first term")

    @property
    def variadic(self):
        return any(isinstance(t, (list, tuple)) for t in self.terms)

    def parts(self):
        """The member lists of the parts, checked: what the GPU path takes of a variadic phrase."""
        parts = [list(t) if isinstance(t, (list, tuple)) else [t] for t in self.terms]
        if len(parts) < 2:
            raise ValueError("a by_phrase of one part is that part's own filter (by_phrase::Prepare, "
                             "phrase_filter.cpp:442-449): send it as an Or of by_term, or through "
                             "prepare_expansions")
        if len(parts) > _lib.MAX_PHRASE_TERMS:
            raise ValueError("a by_phrase has at most %d parts" % _lib.MAX_PHRASE_TERMS)
        for part in parts:
            if not part:
                raise ValueError("a by_phrase part without terms")
            if any(isinstance(t, (bool, float)) or not isinstance(t, (int, np.integer)) for t in part):
                raise ValueError("per-member boosts (the reference's VolatileBoost path) are not on "
                                 "the GPU path: a part's members are plain term ordinals")
            if len(set(int(t) for t in part)) != len(part):
                raise ValueError("a term twice in one by_phrase part")
        if sum(len(p) for p in parts) > _lib.MAX_PHRASE_ENTRIES:
            raise ValueError("a variadic by_phrase has at most %d members in all"
                             % _lib.MAX_PHRASE_ENTRIES)
        return [[int(t) for t in part] for part in parts]


@dataclass
class Not:
    """irs::Not (boolean_filter.hpp): as a child of an And, the docs its filter matches leave the
    And's matches (boolean_query.cpp:121-141: exclusion(included, disjunction(excluded)),
    exclusion.hpp) — scoring nothing and changing no statistic.  `filter`: a by_term, an Or of
    by_term (several excluded terms) or another Not (Not(Not(f)) is f, optimize_not,
    boolean_filter.cpp:35-48)."""
    filter: object


@dataclass
class by_doc_set:
    """A doc set as a child of an And: row `row` of the bitsets the batch is given
    (SegmentReader.batch(..., doc_sets=...), QueryBatch.set_doc_sets) — the reference's unscored
    child of a conjunction: the bitset_doc_iterator of a multi-term query's unscored terms, a
    column-existence filter, proxy_filter's cached bitset.  It only decides which docs match
    (MakeConjunction leaves an iterator with the default score out of the score,
    conjunction.hpp:461-467).  Taken as a direct child of the outermost And only, next to Not
    children; one per And."""
    row: int


def split_doc_set(flt):
    """(filter without its by_doc_set child, row or None): And([f..., by_doc_set(r)]) is the And of
    its other children restricted to row r; a single other child that is not a Not stands for
    itself (boolean_filter.cpp:200-208).  An And of only by_doc_set / Not children has nothing that
    scores: ValueError, as for an And of only Nots."""
    if isinstance(flt, by_doc_set):
        raise ValueError("a by_doc_set alone has no scored part: it is a child of an And")
    if type(flt) is not And or not any(isinstance(s, by_doc_set) for s in flt.subs):
        return flt, None
    rows = [s.row for s in flt.subs if isinstance(s, by_doc_set)]
    if len(rows) > 1:
        raise ValueError("an And takes ONE by_doc_set child: intersect the rows first")
    row = int(rows[0])
    if row < 0 or row >= _lib.NO_DOC_SET:
        raise ValueError("by_doc_set: a row index")
    rest = [s for s in flt.subs if not isinstance(s, by_doc_set)]
    if all(_unwrap_not(s)[1] for s in rest):
        raise ValueError("an And of only by_doc_set / Not children has no scored part "
                         "(only Not / doc set): not on the GPU path")
    if len(rest) == 1:
        inner = rest[0]
        if flt.boost != 1.0:   # (the And's boost multiplies into its one child's)
            inner = replace(inner, boost=float(f32(f32(flt.boost) * f32(inner.boost))))
        return inner, row
    return replace(flt, subs=rest), row


def _unwrap_not(flt):
    """optimize_not (boolean_filter.cpp:35-48): (filter, negated) with double negations removed."""
    neg = False
    while isinstance(flt, Not):
        flt, neg = flt.filter, not neg
    return flt, neg


def _excluded_terms(flt):
    """Term ordinals of the filter under a Not: a by_term, or a plain Or of by_term."""
    if isinstance(flt, by_term):
        return [flt.term]
    if type(flt) is Or and flt.min_match <= 1 and flt.subs and all(type(s) is by_term for s in flt.subs):
        return [s.term for s in flt.subs]
    raise ValueError("Not of %s is not on the GPU path: only Not(by_term) and Not(Or([by_term...])) "
                     "exclude docs" % type(flt).__name__)


def split_exclusions(flt):
    """(included filter, excluded term ordinals) of a filter: And([..., Not(...), ...]) is the And
    of its other children minus the docs of the negated terms; a single included Or / And /
    by_phrase child keeps its own op, min_match and merge (boolean_filter.cpp:200-208,
    boolean_query.cpp:104-109).  Filters without Not come back as they are.  Refused (ValueError):
    what the reference gives other semantics — an Or with a Not child (all docs but ..., with a
    zero-score fill, boolean_filter.cpp:120-127), a filter of only Nots, Not of a phrase or an And."""
    flt, neg = _unwrap_not(flt)
    if neg:
        raise ValueError("a filter of only Not matches all docs but some (zero-score fill): "
                         "not on the GPU path")
    if isinstance(flt, (Or, And)) and any(isinstance(s, Not) for s in flt.subs):
        if type(flt) is not And:
            raise ValueError("an Or with a Not child matches all docs but some (zero-score fill, "
                             "boolean_filter.cpp:120-127): not on the GPU path")
        incl, excl = [], []
        for s in flt.subs:
            f, n = _unwrap_not(s)
            if n:
                excl += _excluded_terms(f)
            else:
                incl.append(f)
        if not incl:
            raise ValueError("an And of only Not children matches all docs but some "
                             "(zero-score fill): not on the GPU path")
        if len(incl) == 1 and not isinstance(incl[0], by_term):
            inner = incl[0]
            if isinstance(inner, (Or, And)) and any(isinstance(s, Not) for s in inner.subs):
                raise ValueError("Not is taken in the outermost And only")
            if flt.boost != 1.0:   # (the And's boost multiplies into its one child's)
                inner = replace(inner, boost=float(f32(f32(flt.boost) * f32(inner.boost))))
            return inner, excl
        if any(isinstance(s, by_phrase) for s in incl):
            # a phrase plus required terms (checked by prepare(): _prepare_phrase_and)
            return And(incl, op=flt.op, merge=flt.merge, boost=flt.boost), excl
        if any(type(s) is not by_term for s in incl):
            raise ValueError("an And with Not children takes by_term children, ONE by_phrase plus "
                             "by_term children, or ONE Or / And / by_phrase child (groups minus some "
                             "terms: And([And([...]), Not(...)]))")
        return And(incl, merge=flt.merge, boost=flt.boost), excl
    return flt, []


def _or_members(flt, mult):
    """(term, boost product) of every by_term under a SUM Or (nested SUM Ors flattened)."""
    out = []
    for s in flt.subs:
        if type(s) is by_term:
            out.append((s.term, f32(f32(mult) * f32(s.boost))))
        elif type(s) is Or and s.min_match <= 1 and (s.merge == MERGE_SUM or len(s.subs) == 1):
            out += _or_members(s, f32(f32(mult) * f32(s.boost)))
        elif isinstance(s, And):
            raise ValueError("an Or with And children (a OR (b AND c)) is not on the GPU path")
        elif isinstance(s, Not):
            raise ValueError("an Or with a Not child matches all docs but some (zero-score fill, "
                             "boolean_filter.cpp:120-127): not on the GPU path")
        elif isinstance(s, by_phrase):
            raise ValueError("a by_phrase inside an Or is not on the GPU path: a phrase is taken alone, "
                             "or as a child of an And next to by_term children")
        elif type(s) is Or:
            raise ValueError("an Or group takes by_term children and SUM Ors of them: min_match > 1 "
                             "and non-SUM merges are not on the GPU path")
        else:
            raise ValueError("%s inside an Or is not on the GPU path" % type(s).__name__)
    return out


def and_groups(flt, mult=1.0):
    """The groups of an And of by_term / Or-of-by_term children, normalised: a by_term child is a
    group of one, so is a one-term Or (the single node case, boolean_filter.cpp:152-155); an And
    child with the same merge is flattened into it; a SUM Or inside a group is flattened into the
    group.  Each member is (term, boost): term boost x Or boosts x And boosts, multiplied from the
    top in float32 as prepare() hands ctx.boost down (boolean_filter.cpp:153-154, 204).  Anything
    else raises ValueError."""
    mult = f32(f32(mult) * f32(flt.boost))
    if flt.op != OP_AND:
        raise ValueError("an And child with op %d is not on the GPU path" % flt.op)
    if not flt.subs:
        raise ValueError("an And without children")
    groups = []
    for s in flt.subs:
        if type(s) is by_term:
            groups.append([(s.term, f32(mult * f32(s.boost)))])
        elif type(s) is And:
            if s.merge != flt.merge:
                raise ValueError("an And child with another merge type is not on the GPU path")
            groups += and_groups(s, mult)
        elif type(s) is Or:
            if s.min_match > 1:
                raise ValueError("an Or group with min_match > 1 is not on the GPU path")
            if len(s.subs) != 1 and s.merge != MERGE_SUM:
                raise ValueError("an Or group merges with SUM on the GPU path")
            members = _or_members(s, f32(mult * f32(s.boost)))
            if not members:
                raise ValueError("an Or group without terms")
            groups.append(members)
        elif isinstance(s, Not):
            raise ValueError("Not is taken by prepare() only (as a child of the outermost And)")
        elif isinstance(s, by_phrase):
            raise ValueError("a by_phrase inside a nested And is not on the GPU path: a phrase is "
                             "taken as a child of the outermost And, next to by_term children")
        else:
            raise ValueError("%s inside an And is not on the GPU path" % type(s).__name__)
    if sum(len(g) for g in groups) > _lib.MAX_TERMS:
        raise ValueError("an And has at most %d terms in all its groups" % _lib.MAX_TERMS)
    return groups


def _and_members(flt, mult):
    """(term, boost product) of every by_term under an And that is a clause of an Or (nested SUM Ands
    flattened; a one-term And is its term)."""
    if flt.op != OP_AND:
        raise ValueError("an And child with op %d inside an Or is not on the GPU path" % flt.op)
    if not flt.subs:
        raise ValueError("an And without children inside an Or")
    if flt.merge != MERGE_SUM and len(flt.subs) > 1:
        raise ValueError("an And inside an Or merges with SUM on the GPU path (MAX / MIN clauses are "
                         "not built)")
    mult = f32(f32(mult) * f32(flt.boost))
    out = []
    for s in flt.subs:
        if type(s) is by_term:
            out.append((s.term, f32(mult * f32(s.boost))))
        elif type(s) is And:
            out += _and_members(s, mult)
        elif isinstance(s, Or):
            raise ValueError("an And child of an Or with an Or inside ((a AND (b OR c)) OR d) is not on "
                             "the GPU path: a clause is an And of by_term")
        elif isinstance(s, Not):
            raise ValueError("an And child of an Or with a Not inside ((a AND NOT b) OR c) is not on "
                             "the GPU path: a clause is an And of by_term")
        elif isinstance(s, by_phrase):
            raise ValueError("an And child of an Or with a by_phrase inside is not on the GPU path: a "
                             "clause is an And of by_term")
        else:
            raise ValueError("%s inside an And child of an Or is not on the GPU path" % type(s).__name__)
    return out


def or_clauses(flt, mult=1.0):
    """The clauses of an Or whose children are by_term, And of by_term and SUM Ors of those,
    normalised: a by_term child is a clause of one, so is a one-term And (the single node case,
    boolean_filter.cpp:152-155); nested SUM Ands are flattened into their clause; an Or child with
    min_match <= 1 that merges with SUM is flattened into its parent where that parent's min_match
    is <= 1 too (an Or of ONE child is that child under any parent).  Each member is (term, boost):
    term boost x And boosts x Or boosts, multiplied from the top in float32 as prepare() hands
    ctx.boost down (boolean_filter.cpp:153-154, 204).  Anything else raises ValueError."""
    if not flt.subs:
        raise ValueError("an Or without children")
    if flt.merge != MERGE_SUM and len(flt.subs) > 1:
        raise ValueError("an Or with And children merges with SUM on the GPU path (MAX / MIN over "
                         "clauses are not built)")
    mult = f32(f32(mult) * f32(flt.boost))
    clauses = []
    for s in flt.subs:
        if type(s) is by_term:
            clauses.append([(s.term, f32(mult * f32(s.boost)))])
        elif type(s) is And:
            clauses.append(_and_members(s, mult))
        elif type(s) is Or:
            one = len(s.subs) == 1
            if s.min_match > 1 or (flt.min_match > 1 and not one):
                raise ValueError("an Or child of an Or is flattened into it only where both have "
                                 "min_match <= 1: a min-match over nested Ors is not on the GPU path")
            if s.merge != MERGE_SUM and not one:
                raise ValueError("an Or child of an Or merges with SUM on the GPU path")
            clauses += or_clauses(s, mult)
        elif isinstance(s, Not):
            raise ValueError("an Or with a Not child matches all docs but some (zero-score fill, "
                             "boolean_filter.cpp:120-127): not on the GPU path")
        elif isinstance(s, by_phrase):
            raise ValueError("a by_phrase next to an And child in an Or ((a AND b) OR \"c d\") is not on "
                             "the GPU path: a clause is a by_term or an And of by_term")
        else:
            raise ValueError("%s inside an Or is not on the GPU path" % type(s).__name__)
    if sum(len(c) for c in clauses) > _lib.MAX_TERMS:
        raise ValueError("an Or has at most %d terms in all its clauses" % _lib.MAX_TERMS)
    return clauses


def boolean_tree(flt, mult=1.0):
    """A nested filter of by_term / And / Or / Not, normalised for the tree encoding
    (IRS_HIP_TREE_NODE).  Returns ("leaf", term, boost) or ("node", op, min_match, children), every
    child a pair (negated, subtree):
      a node of one positive child collapses into that child, its boost multiplied in (the single
      node case, boolean_filter.cpp:152-155); an And child of an And is flattened into it; a SUM Or
      child with min_match <= 1 is flattened into an Or with min_match <= 1; Not(Not(f)) is f
      (optimize_not, boolean_filter.cpp:35-48).
    A leaf's boost is its own times every ancestor's, multiplied from the top in float32 as prepare()
    hands ctx.boost down (boolean_filter.cpp:153-154, 204); what stands under a Not scores nothing.
    Anything else raises ValueError."""
    if type(flt) is by_term:
        return ("leaf", int(flt.term), f32(f32(mult) * f32(flt.boost)))
    if isinstance(flt, Not):
        raise ValueError("a filter of only Not matches all docs but some (zero-score fill): "
                         "not on the GPU path")
    if isinstance(flt, (by_phrase, by_terms, by_doc_set)):
        raise ValueError("a %s inside a nested boolean filter is not on the GPU path: the leaves of a "
                         "tree (IRS_HIP_TREE_NODE) are by_term" % type(flt).__name__)
    if type(flt) not in (And, Or):
        raise ValueError("%s inside a nested boolean filter is not on the GPU path" % type(flt).__name__)
    if type(flt) is And and flt.op != OP_AND:
        raise ValueError("an And child with op %d is not on the GPU path" % flt.op)
    if not flt.subs:
        raise ValueError("%s without children" % ("an And" if type(flt) is And else "an Or"))
    if flt.merge != MERGE_SUM and len(flt.subs) > 1:
        raise ValueError("a nested boolean filter merges with SUM at every level on the GPU path "
                         "(MAX / MIN are not built)")
    conj = type(flt) is And
    if not conj and flt.min_match < 1:
        raise ValueError("an Or with min_match 0 matches all docs (boolean_filter.cpp:213): not on the "
                         "GPU path")
    mult = f32(f32(mult) * f32(flt.boost))
    children = []
    for s in flt.subs:
        f, neg = _unwrap_not(s)
        if neg and not conj:
            raise ValueError("an Or with a Not child matches all docs but some (zero-score fill, "
                             "boolean_filter.cpp:120-127): not on the GPU path")
        sub = boolean_tree(f, f32(1) if neg else mult)
        if sub[0] == "node" and not neg and (
                (conj and sub[1] == OP_AND) or
                (not conj and flt.min_match <= 1 and sub[1] == OP_OR)):
            children += sub[3]     # (same operator: flattened)
        else:
            children.append((neg, sub))
    if conj and all(neg for neg, _ in children):
        raise ValueError("an And of only Not children matches all docs but some (zero-score fill): "
                         "not on the GPU path")
    if len(children) == 1 and (conj or flt.min_match <= 1):
        return children[0][1]
    return ("node", OP_AND if conj else flt.op, 0 if conj or flt.min_match <= 1 else int(flt.min_match), children)


def tree_entries(tree):
    """The prefix form of a normalised tree's children: one item per entry — ("leaf", term, boost),
    ("not", term) or ("node", op, span, min_match, negated), a node followed by the `span` entries
    of its subtree.  (n_leaves, n_nodes) with it."""
    out = []
    n_leaves = n_nodes = 0
    for neg, sub in tree[3]:
        if sub[0] == "leaf":
            out.append(("not", sub[1]) if neg else sub)
            n_leaves += 1
        else:
            inner, nl, nn = tree_entries(sub)
            out.append(("node", sub[1], len(inner), sub[2], neg))
            out += inner
            n_leaves += nl
            n_nodes += nn + 1
    return out, n_leaves, n_nodes


def _terms_of(flt):
    if isinstance(flt, Not):
        raise ValueError("Not is taken by prepare() only (as a child of an And), not here")
    if isinstance(flt, by_term):
        return OP_OR, [flt]
    if not flt.subs or any(not isinstance(s, by_term) for s in flt.subs):
        raise ValueError("only flat Or/And of by_term are on the GPU path")
    return flt.op, list(flt.subs)


@dataclass
class PreparedQuery:
    """filter::prepared: the op plus (term, global stats, boost) per sub-filter."""
    op: int
    terms: list            # term ordinals
    scorers: list          # (kind, c0, norm_const, norm_length) per term
    min_match: int = 0
    offsets: list | None = None   # OP_PHRASE: position of every term in the phrase
    merge: int = MERGE_SUM
    excluded: list = field(default_factory=list)   # term ordinals under Not (IRS_HIP_EXCLUDE)
    alts: list | None = None   # OP_PHRASE: True for an entry that is one more member of the part
                               # before it (IRS_HIP_PHRASE_ALT); OP_AND: ... of the group before it
                               # (IRS_HIP_GROUP_ALT, the same bit)
    required: list | None = None   # OP_PHRASE: True for an entry that is a required term — a by_term
                                   # child of the And that holds the phrase (IRS_HIP_PHRASE_REQUIRED),
                                   # carrying its own scorer; None: a phrase alone
    doc_set: int | None = None     # by_doc_set under the And: the row of the batch's doc sets the
                                   # query is restricted to (irs_hip_batch_set_doc_sets); None: none
    optional: list | None = None   # OP_PHRASE: True for an entry that is an optional term — a by_term
                                   # child of the Or that holds the phrase (IRS_HIP_PHRASE_OPTIONAL),
                                   # carrying its own scorer; None: no Or around the phrase
    clause: list | None = None     # OP_OR / OP_MINMATCH: True for an entry that is one more required
                                   # member of the clause before it (IRS_HIP_CLAUSE_AND) — an Or with
                                   # And children, min_match counting clauses; None: a flat Or
    tree: list | None = None       # a tree query (IRS_HIP_TREE_NODE): per entry None — a leaf with its
                                   # scorer —, "not" — a negated leaf, an IRS_HIP_EXCLUDE entry where it
                                   # stands — or (op, span, min_match, negated) — a node entry (its
                                   # term is None); `op` / `min_match` are the root's; None: no tree
    opens: list | None = None      # OP_PHRASE: True for an entry that is the first word of a FURTHER
                                   # phrase of the And (IRS_HIP_PHRASE_NEXT): the words of phrase 1, of
                                   # phrase 2, ..., then the required terms; None: one phrase
    or_opens: list | None = None   # OP_PHRASE: True for an entry that is the first word of an
                                   # ALTERNATIVE phrase of the Or (IRS_HIP_PHRASE_OR): the words of
                                   # phrase 1, of phrase 2, ...; None: one phrase


# ------------------------------------------------------------------ segment --

class SegmentReader:
    """irs::SubReader + postings_reader of one segment, resident on one GPU."""

    def __init__(self, doc_file, metas, num_docs, layout, norms=None, norm_width=1,
                 docs_with_field=None, total_term_freq=0, device=0, has_freq=True, L=None,
                 wand_count=0, pos_file=None, pos_features=0, norm_kind=0, wand_type=0,
                 doc_mask=None):
        self.L = L or _lib.lib()
        self.doc_file = np.ascontiguousarray(doc_file, np.uint8)
        self.metas = np.zeros(len(metas), TERM_META)
        for name in TERM_META.names:
            self.metas[name] = np.asarray(metas)[name]
        self.num_docs, self.layout, self.device = int(num_docs), int(layout), int(device)
        self.norms = None if norms is None else np.ascontiguousarray(norms, np.uint8)
        self.norm_width = norm_width
        self.docs_with_field = int(num_docs if docs_with_field is None else docs_with_field)
        self.total_term_freq = int(total_term_freq)
        self.pos_file = None if pos_file is None else np.ascontiguousarray(pos_file, np.uint8)
        # the segment's DocumentMask (deleted doc ids): SegmentReaderImpl::mask, applied by every batch
        self.doc_mask = None if doc_mask is None else np.ascontiguousarray(doc_mask, np.uint32)
        desc = SegmentDesc(
            device, layout, self.doc_file.ctypes.data, self.doc_file.size, num_docs,
            int(has_freq), None if self.norms is None else self.norms.ctypes.data, norm_width, 1,
            0 if self.norms is None else self.norms.size // norm_width,
            self.metas.ctypes.data, len(self.metas), int(wand_count),
            None if self.pos_file is None else self.pos_file.ctypes.data,
            0 if self.pos_file is None else self.pos_file.size, int(pos_features), int(norm_kind),
            int(wand_type),
            None if self.doc_mask is None or not self.doc_mask.size else self.doc_mask.ctypes.data,
            0 if self.doc_mask is None else self.doc_mask.size)
        h = C.c_void_p()
        _lib.check(self.L, self.L.irs_hip_segment_open(C.byref(desc), C.byref(h)),
                   "irs_hip_segment_open")
        self.handle = h

    @classmethod
    def from_synth(cls, seg, device=0, L=None, has_freq=True, doc_mask=None):
        return cls(seg.doc_file, seg.metas, seg.num_docs, seg.layout, seg.norms, 1,
                   seg.docs_with_field, seg.total_term_freq, device, has_freq, L,
                   getattr(seg, "wand_count", 0), getattr(seg, "pos_file", None),
                   wand_type=getattr(seg, "wand_type", 0),
                   doc_mask=getattr(seg, "doc_mask", None) if doc_mask is None else doc_mask)

    def close(self):
        if self.handle:
            self.L.irs_hip_segment_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_bytes(self) -> int:
        return self.L.irs_hip_segment_device_bytes(self.handle)

    def live_docs_count(self) -> int:
        """SubReader::live_docs_count: docs that are not in the segment's doc_mask."""
        return self.L.irs_hip_segment_live_docs(self.handle)

    def decode_term(self, term: int, want_freq: bool = True):
        n = int(self.metas[term]["docs_count"])
        docs = np.zeros(max(n, 1), np.uint32)
        freqs = np.zeros(max(n, 1), np.uint32) if want_freq else None
        cnt = C.c_uint32()
        _lib.check(self.L, self.L.irs_hip_decode_term(
            self.handle, term, docs.ctypes.data, None if freqs is None else freqs.ctypes.data,
            docs.size, C.byref(cnt)), "irs_hip_decode_term")
        return docs[:cnt.value], (None if freqs is None else freqs[:cnt.value])

    def decode_positions(self, term: int):
        """Every position of every doc of the term, doc after doc (term_meta::freq values)."""
        n = int(self.metas[term]["freq"])
        out = np.zeros(max(n, 1), np.uint32)
        cnt = C.c_uint64()
        _lib.check(self.L, self.L.irs_hip_decode_positions(
            self.handle, term, out.ctypes.data, out.size, C.byref(cnt)),
            "irs_hip_decode_positions")
        return out[:cnt.value]

    def bit_union(self, terms, n_words: int, initial=None):
        """postings_reader::bit_union: (bitset as uint64 words, sum of docs_count)."""
        t = np.ascontiguousarray(terms, np.uint32)
        bits = np.zeros(n_words, np.uint64) if initial is None else \
            np.ascontiguousarray(initial, np.uint64).copy()
        cnt = C.c_uint64()
        _lib.check(self.L, self.L.irs_hip_bit_union(
            self.handle, t.ctypes.data if t.size else None, t.size, bits.ctypes.data, n_words,
            C.byref(cnt)), "irs_hip_bit_union")
        return bits, cnt.value

    def bit_union_counts(self, term_sets):
        """The populations of several term sets' unions (irs_hip_bit_union_counts): one number per
        set comes back, the bitsets stay on the device."""
        sets = [np.ascontiguousarray(t, np.uint32) for t in term_sets]
        offsets = np.zeros(len(sets) + 1, np.uint32)
        np.cumsum([len(t) for t in sets], out=offsets[1:])
        flat = np.concatenate(sets) if sets and offsets[-1] else np.zeros(1, np.uint32)
        counts = np.zeros(max(len(sets), 1), np.uint64)
        _lib.check(self.L, self.L.irs_hip_bit_union_counts(
            self.handle, flat.ctypes.data, offsets.ctypes.data, len(sets), counts.ctypes.data),
            "irs_hip_bit_union_counts")
        return counts[:len(sets)]

    def term_directory(self, term: int):
        nb = int(self.metas[term]["docs_count"]) // 128
        last = np.zeros(max(nb, 1), np.uint32)
        offs = np.zeros(max(nb, 1), np.uint64)
        cnt = C.c_uint32()
        _lib.check(self.L, self.L.irs_hip_term_directory(
            self.handle, term, last.ctypes.data, offs.ctypes.data, last.size, C.byref(cnt)),
            "irs_hip_term_directory")
        return last[:cnt.value], offs[:cnt.value]

    def wand_source(self):
        """(blocks whose (max freq, min norm) was read from the index's own wand data, all blocks)."""
        a, b = C.c_uint64(), C.c_uint64()
        _lib.check(self.L, self.L.irs_hip_segment_wand_source(self.handle, C.byref(a), C.byref(b)),
                   "irs_hip_segment_wand_source")
        return a.value, b.value

    def term_blockmax(self, term: int):
        """Per full block of the term: (largest frequency, smallest non-zero norm) — the
        block-max data WAND batches prune with."""
        nb = int(self.metas[term]["docs_count"]) // 128
        mf = np.zeros(max(nb, 1), np.uint32)
        mn = np.zeros(max(nb, 1), np.uint32)
        cnt = C.c_uint32()
        _lib.check(self.L, self.L.irs_hip_term_blockmax(
            self.handle, term, mf.ctypes.data, mn.ctypes.data, mf.size, C.byref(cnt)),
            "irs_hip_term_blockmax")
        return mf[:cnt.value], mn[:cnt.value]

    def batch(self, prepared, k: int, doc_sets=None):
        """`doc_sets`: the bitsets the queries' by_doc_set children name rows of — u64[rows][words],
        bit = doc id: a numpy array (copied to the device) or a torch tensor on the device
        (borrowed: QueryBatch.set_doc_sets)."""
        return QueryBatch(self, prepared, k, doc_sets=doc_sets)


class QueryArrays:
    """The C arrays irs_hip_batch_create_multi takes for a list of prepared queries on a list
    of segments: irs_hip_query[nq] and irs_hip_term_scorer[n_segs][n_entries] (every segment
    gets the same scorer constants and its own term ordinals).  Building them is the host half
    of filter::prepare; creating a batch from them is one C call."""

    def __init__(self, n_segs, queries, terms, k):
        self.n_segs, self.queries, self.terms, self.k = int(n_segs), queries, terms, int(k)

    @classmethod
    def from_prepared(cls, segs, prepared, k):
        """(A query's by_doc_set row is no part of the arrays: QueryBatch reads it from the prepared
        queries it is given, or the caller hands row_of_unit to set_doc_sets.)"""
        n_entries = sum(len(p.terms) + len(p.excluded) for p in prepared)
        queries = np.zeros(len(prepared), QUERY)
        terms = np.zeros((len(segs), max(n_entries, 1)), TERM_SCORER)
        at = 0
        for q, p in enumerate(prepared):
            queries[q] = (p.op, len(p.terms) + len(p.excluded), at, int(k), p.min_match, p.merge)
            offs = p.offsets if p.offsets is not None else [0] * len(p.terms)
            alts = p.alts if p.alts is not None else [False] * len(p.terms)
            reqs = p.required if p.required is not None else [False] * len(p.terms)
            opts = p.optional if p.optional is not None else [False] * len(p.terms)
            more = p.clause if p.clause is not None else [False] * len(p.terms)
            nxts = p.opens if p.opens is not None else [False] * len(p.terms)
            ors = p.or_opens if p.or_opens is not None else [False] * len(p.terms)
            tree = p.tree if p.tree is not None else [None] * len(p.terms)
            for t, (kind, c0, nc, nl), off, alt, req, opt, cl, nxt, orr, nd in zip(p.terms, p.scorers, offs, alts, reqs,
                                                                                  opts, more, nxts, ors, tree):
                if nd == "not":          # a negated leaf where it stands: no scorer
                    kind, c0, nc, nl, off = EXCLUDE, 0.0, 0.0, 0.0, 0
                elif nd is not None:     # a node entry: its op, the entries of its subtree, its min_match
                    n_op, span, mm, neg = nd
                    kind, c0, nc, nl = TREE_NODE | n_op | (EXCLUDE if neg else 0), 0.0, 0.0, 0.0
                    off = span | (mm << 16)
                kind = kind | CLAUSE_AND if cl else kind
                kind = kind | PHRASE_NEXT if nxt else kind
                kind = kind | PHRASE_OR if orr else kind
                kind = kind | PHRASE_ALT if alt else kind   # (GROUP_ALT for an And: the same bit)
                kind = kind | PHRASE_REQUIRED if req else kind
                kind = kind | PHRASE_OPTIONAL if opt else kind
                for s, sr in enumerate(segs):       # same scorer, the segment's own ordinal
                    present = t is not None and 0 <= t < len(sr.metas)
                    terms[s, at] = (t if present else NO_TERM, kind, c0, nc, nl, off)
                at += 1
            for t in p.excluded:                     # behind the included entries
                for s, sr in enumerate(segs):
                    present = t is not None and 0 <= t < len(sr.metas)
                    terms[s, at] = (t if present else NO_TERM, EXCLUDE, 0.0, 0.0, 0.0, 0)
                at += 1
        return cls(len(segs), queries, terms, k)


def prepare_disjunctions(term_rows, scorer, segment_stats, segs, k, boost=1.0):
    """prepare() + QueryArrays.from_prepared for the common case — every row of `term_rows`
    (int array [nq][n_terms] of term ordinals) is an Or of by_term filters with one boost —
    with the statistics of ALL terms computed at once (numpy), value for value what
    BM25.collect / TFIDF.collect / term_scorer compute one term at a time (the test suite
    compares the two).  This is the per-batch host work of a serving loop."""
    rows = np.ascontiguousarray(term_rows, np.int64)
    nq, nt = rows.shape
    flat = rows.reshape(-1)
    dwf = sum(s.docs_with_field for s in segment_stats)
    ttf = sum(s.total_term_freq for s in segment_stats)
    dwt = np.zeros(flat.size, np.float64)
    for st in segment_stats:
        dc = np.asarray(st.docs_count)
        ok = (flat >= 0) & (flat < len(dc))
        dwt[ok] += dc[flat[ok]]
    if isinstance(scorer, BM25):
        idf = np.log1p((float(dwf) - dwt + 0.5) / (dwt + 0.5)).astype(np.float32)
        c0 = (f32(f32(boost) * f32(scorer.k + f32(1))) * idf).astype(np.float32)
        probe = scorer.collect(dwf, 1, ttf)
        kind = scorer.term_scorer(probe)[0]
        nc, nl = probe.norm_const, probe.norm_length
    else:
        idf = np.log1p((dwf + 1.0) / (dwt + 1.0)).astype(np.float32)
        c0 = (f32(boost) * idf).astype(np.float32)
        kind, nc, nl = scorer.term_scorer(TermStats(f32(1)))[0], f32(0), f32(0)
    queries = np.zeros(nq, QUERY)
    queries["op"], queries["n_terms"], queries["k"] = OP_OR, nt, int(k)
    queries["first_term"] = np.arange(nq, dtype=np.uint32) * nt
    queries["min_match"], queries["merge"] = 1, MERGE_SUM
    terms = np.zeros((len(segs), max(flat.size, 1)), TERM_SCORER)
    for s, sr in enumerate(segs):
        present = (flat >= 0) & (flat < len(sr.metas))
        terms["term"][s, :flat.size] = np.where(present, flat, NO_TERM).astype(np.uint32)
    terms["kind"][:, :flat.size] = kind
    terms["c0"][:, :flat.size] = c0
    terms["norm_const"][:, :flat.size] = nc
    terms["norm_length"][:, :flat.size] = nl
    return QueryArrays(len(segs), queries, terms, k)


def prepare_filters(filters, scorer, segment_stats, segs, k):
    """prepare() + QueryArrays.from_prepared for ANY list of the flat filters of this path
    (by_term, Or, Or with min_match, And, by_phrase — one list may mix the boolean kinds; phrases
    go in batches of their own) with the statistics of all terms computed at once: value for value
    what the term-by-term prepare() yields (tests/test_host_prepare.py compares the two).  The
    reference harness builds and prepares every task's filter inside its timer
    (index-search.cpp:694-722, in C++); this is that stage for a batch without a Python loop over
    the terms."""
    nq = len(filters)
    ops, nts, mms, mgs = (np.zeros(nq, np.int64) for _ in range(4))
    tl, bl, ol = [], [], []
    ol_any = False
    # (one pass over the filter objects, the inner loops as list comprehensions: for 1000 filters
    # of 8 terms this loop IS the stage's time)
    for q, flt in enumerate(filters):
        cls = type(flt)
        if cls is by_term:
            ops[q], nts[q] = OP_OR, 1
            mgs[q] = MERGE_SUM
            tl.append(flt.term)
            bl.append(flt.boost)
            continue
        if cls is by_terms:
            flt.check()
            pairs = flt.pairs()
            ops[q], nts[q], mms[q], mgs[q] = OP_MULTITERM, len(pairs), int(flt.min_match), MERGE_SUM
            tl += [t for t, _ in pairs]
            bl += [tb if flt.boost == 1.0 else f32(f32(flt.boost) * f32(tb)) for _, tb in pairs]
            if ol_any:
                ol += [0] * len(pairs)
            continue
        if isinstance(flt, by_phrase):
            if flt.variadic:
                raise ValueError("variadic by_phrase (a part of several terms) is taken by "
                                 "prepare(), not by the array path prepare_filters")
            n = len(flt.terms)
            ops[q], nts[q] = OP_PHRASE, n
            if not ol_any:
                ol = [0] * len(tl)
                ol_any = True
            tl.extend(flt.terms)
            bl.extend([flt.boost] * n)
            ol.extend(flt.offsets)
            continue
        if cls is Or or cls is And:
            subs = flt.subs
            try:
                terms_q = [s.term for s in subs]
                boosts_q = [s.boost for s in subs]
            except AttributeError:
                terms_q = None
            if not subs or terms_q is None or (set(map(type, subs)) != {by_term} and
                                               any(not isinstance(s, by_term) for s in subs)):
                if any(isinstance(s, Not) for s in subs):
                    raise ValueError("Not is taken by prepare() (IRS_HIP_EXCLUDE), not by the "
                                     "array path prepare_filters")
                if cls is And and sum(isinstance(s, by_phrase) for s in subs) > 1:
                    raise ValueError("several by_phrase children of an And (IRS_HIP_PHRASE_NEXT) are "
                                     "taken by prepare(..., phrase_conjunctions=True), not by the "
                                     "array path prepare_filters")
                if cls is Or and sum(isinstance(s, by_phrase) for s in subs) > 1:
                    raise ValueError("several by_phrase children of an Or (IRS_HIP_PHRASE_OR) are "
                                     "taken by prepare(..., phrase_disjunctions=True), not by the "
                                     "array path prepare_filters")
                if any(isinstance(s, by_phrase) for s in subs):
                    raise ValueError("a by_phrase inside an And (a phrase plus required terms, "
                                     "IRS_HIP_PHRASE_REQUIRED) is taken by prepare(), not by the "
                                     "array path prepare_filters")
                if cls is Or and any(isinstance(s, (And, Or)) for s in subs):
                    raise ValueError("an Or with And children (IRS_HIP_CLAUSE_AND) is taken by "
                                     "prepare(..., and_clauses=True), deeper trees (IRS_HIP_TREE_NODE) by "
                                     "prepare(..., boolean_trees=True), not by the array path prepare_filters")
                raise ValueError("only flat Or/And of by_term are on the array path: an And with "
                                 "Or children is taken by prepare()")
            op = flt.op
            if flt.boost != 1.0:   # (boost_filter::boost() of the Or / And times each term's)
                boosts_q = [f32(f32(flt.boost) * f32(b)) for b in boosts_q]
        else:
            op, subs = _terms_of(flt)
            terms_q = [s.term for s in subs]
            boosts_q = [s.boost for s in subs]
        ops[q], nts[q] = op, len(terms_q)
        mms[q] = int(getattr(flt, "min_match", 0))
        mgs[q] = int(getattr(flt, "merge", MERGE_SUM))
        tl += terms_q
        bl += boosts_q
        if ol_any:
            ol += [0] * len(terms_q)
    if not ol_any:
        ol = np.zeros(len(tl), np.uint32)
    flat = np.asarray(tl, np.int64)
    boost = np.asarray(bl, np.float32)
    first = np.zeros(nq, np.int64)
    np.cumsum(nts[:-1], out=first[1:])
    dwf = sum(s.docs_with_field for s in segment_stats)
    ttf = sum(s.total_term_freq for s in segment_stats)
    dwt = np.zeros(flat.size, np.float64)
    for st in segment_stats:
        dc = np.asarray(st.docs_count)
        ok = (flat >= 0) & (flat < len(dc))
        dwt[ok] += dc[flat[ok]]
    if isinstance(scorer, BM25):
        idf = np.log1p((float(dwf) - dwt + 0.5) / (dwt + 0.5)).astype(np.float32)
        probe = scorer.collect(dwf, 1, ttf)
        kind = scorer.term_scorer(probe)[0]
        nc, nl = probe.norm_const, probe.norm_length
    else:
        idf = np.log1p((dwf + 1.0) / (dwt + 1.0)).astype(np.float32)
        kind, nc, nl = scorer.term_scorer(TermStats(f32(1)))[0], f32(0), f32(0)
    # by_phrase: ONE stats blob per phrase, into which every term's idf was added in phrase order
    # (float32 `idf +=`: bm25.cpp:381-383, tfidf.cpp:272-275) — every entry carries that sum
    ph = np.nonzero(ops == OP_PHRASE)[0]
    if ph.size:
        acc = np.zeros(ph.size, np.float32)
        for j in range(int(nts[ph].max())):
            on = nts[ph] > j
            acc[on] = (acc[on] + idf[first[ph[on]] + j]).astype(np.float32)
        of_q = np.repeat(np.arange(nq), nts)
        slot = np.full(nq, -1, np.int64)
        slot[ph] = np.arange(ph.size)
        is_ph = slot[of_q] >= 0
        idf = idf.copy()
        idf[is_ph] = acc[slot[of_q[is_ph]]]
    if isinstance(scorer, BM25):
        c0 = ((boost * f32(scorer.k + f32(1))).astype(np.float32) * idf).astype(np.float32)
    else:
        c0 = (boost * idf).astype(np.float32)
    queries = np.zeros(nq, QUERY)
    queries["op"], queries["n_terms"], queries["first_term"] = ops, nts, first
    queries["k"], queries["min_match"], queries["merge"] = int(k), mms, mgs
    terms = np.zeros((len(segs), max(flat.size, 1)), TERM_SCORER)
    for s, sr in enumerate(segs):
        present = (flat >= 0) & (flat < len(sr.metas))
        terms["term"][s, :flat.size] = np.where(present, flat, NO_TERM).astype(np.uint32)
    terms["kind"][:, :flat.size] = kind
    terms["c0"][:, :flat.size] = c0
    terms["norm_const"][:, :flat.size] = nc
    terms["norm_length"][:, :flat.size] = nl
    terms["phrase_offset"][:, :flat.size] = np.asarray(ol, np.uint32)
    return QueryArrays(len(segs), queries, terms, k)


class DeviceBuffer:
    """Device memory by irs_hip_device_alloc / _upload / _download: what a caller without a HIP
    toolchain of its own hands to the *_to_device calls.  `ptr` is the device address."""

    def __init__(self, L, device: int, nbytes: int):
        self.L, self.device, self.nbytes = L, int(device), int(nbytes)
        p = C.c_void_p()
        _lib.check(L, L.irs_hip_device_alloc(self.device, max(self.nbytes, 8), C.byref(p)), "irs_hip_device_alloc")
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _lib.check(self.L, self.L.irs_hip_device_upload(self.device, self.ptr, arr.ctypes.data, arr.nbytes),
                   "irs_hip_device_upload")
        return self

    def download(self, dtype, shape):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        _lib.check(self.L, self.L.irs_hip_device_download(self.device, out.ctypes.data, self.ptr, out.nbytes),
                   "irs_hip_device_download")
        return out

    def close(self):
        if self.ptr:
            self.L.irs_hip_device_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # (interpreter shutdown: the library may be gone)
            pass


class QueryBatch:
    """A batch of prepared queries on one segment — or on several segments of one device
    at once (irs_hip_batch_create_multi): then every result array gets a leading segment
    axis, [n_segs][nq]..., in the order the readers were given.  `prepared`: a list of
    PreparedQuery, or the QueryArrays made from one."""

    def __init__(self, seg, prepared, k: int | None = None, doc_sets=None):
        self.handle = None
        self.segs = list(seg) if isinstance(seg, (list, tuple)) else [seg]
        self.multi = isinstance(seg, (list, tuple))
        arrays = prepared if isinstance(prepared, QueryArrays) else \
            QueryArrays.from_prepared(self.segs, prepared, k)
        assert arrays.n_segs == len(self.segs)
        self.seg, self.L, self.k = self.segs[0], self.segs[0].L, arrays.k
        self.nq_user = len(arrays.queries)
        self.nq = self.nq_user * len(self.segs)          # execution units
        self.queries, self.terms = arrays.queries, arrays.terms
        h = C.c_void_p()
        handles = (C.c_void_p * len(self.segs))(*[sr.handle for sr in self.segs])
        _lib.check(self.L, self.L.irs_hip_batch_create_multi(
            handles, len(self.segs), self.queries.ctypes.data, self.nq_user,
            self.terms.ctypes.data, self.terms.shape[1], C.byref(h)),
            "irs_hip_batch_create_multi")
        self.handle = h
        rows = [] if isinstance(prepared, QueryArrays) else [getattr(p, "doc_set", None) for p in prepared]
        if any(r is not None for r in rows):
            try:
                if doc_sets is None:
                    raise ValueError("a query with a by_doc_set child needs the batch's doc_sets")
                one = [_lib.NO_DOC_SET if r is None else int(r) for r in rows]
                self.set_doc_sets(doc_sets, np.tile(np.array(one, np.uint32), len(self.segs)))
            except Exception:
                self.close()
                raise
        elif doc_sets is not None:
            # (QueryArrays carry no rows: the caller names them — set_doc_sets(sets, row_of_unit))
            self.close()
            raise ValueError("doc_sets without a by_doc_set query: call set_doc_sets(sets, row_of_unit)")

    def configure(self, tile_docs=0, pilot_stride=0, cand_cap=0):
        _lib.check(self.L, self.L.irs_hip_batch_configure(self.handle, tile_docs, pilot_stride,
                                                          cand_cap), "irs_hip_batch_configure")
        return self

    def set_shared_threshold(self, enable=True):
        """One threshold per query for its units on the batch's segments
        (irs_hip_batch_set_shared_threshold): for callers that merge the per-segment lists."""
        _lib.check(self.L, self.L.irs_hip_batch_set_shared_threshold(self.handle, int(bool(enable))),
                   "irs_hip_batch_set_shared_threshold")
        return self

    def set_comm(self, comm):
        """One threshold per query across RANKS (irs_hip_batch_set_comm): `comm` = a
        distributed.Communicator (or None to detach); every rank attaches one to its batch of the
        same queries and runs the batches in the same order."""
        self._comm = comm   # (must outlive the batch)
        _lib.check(self.L, self.L.irs_hip_batch_set_comm(self.handle, comm.handle if comm else None),
                   "irs_hip_batch_set_comm")
        return self

    def set_path(self, path):
        """PATH_AUTO / PATH_ITEMS / PATH_JOINED (irs_hip_batch_set_path)."""
        _lib.check(self.L, self.L.irs_hip_batch_set_path(self.handle, int(path)),
                   "irs_hip_batch_set_path")
        return self

    def set_async(self, enable=True):
        """Hand the host half of run() to the library's worker thread (1), keep it on the caller's
        thread (0), or follow the process default (-1): irs_hip_batch_set_async."""
        _lib.check(self.L, self.L.irs_hip_batch_set_async(self.handle, int(enable)),
                   "irs_hip_batch_set_async")
        return self

    def path(self):
        """Which path the last run took (PATH_ITEMS / PATH_JOINED)."""
        v = C.c_int(0)
        _lib.check(self.L, self.L.irs_hip_batch_path(self.handle, C.byref(v)), "irs_hip_batch_path")
        return int(v.value)

    def set_paired_tiles(self, enable=True):
        """Joined plain disjunctions on paired doc tiles: 1 / True = where it pays (default: segments
        of ~2.4 M docs and more), 2 = whatever the size, 0 / False = never (32-bit tiles).  The results
        are bit-identical either way."""
        _lib.check(self.L, self.L.irs_hip_batch_set_paired_tiles(self.handle, int(enable)),
                   "irs_hip_batch_set_paired_tiles")
        return self

    def paired_tiles(self):
        """Whether the last run's joined plain disjunctions ran on paired tiles."""
        v = C.c_int(0)
        _lib.check(self.L, self.L.irs_hip_batch_paired_tiles(self.handle, C.byref(v)),
                   "irs_hip_batch_paired_tiles")
        return bool(v.value)

    def tail_stream_used(self):
        """Whether the last run ended on the device's tail stream (irs_hip_batch_tail_stream_used)."""
        v = C.c_int(0)
        _lib.check(self.L, self.L.irs_hip_batch_tail_stream_used(self.handle, C.byref(v)),
                   "irs_hip_batch_tail_stream_used")
        return bool(v.value)

    def set_wand(self, enable=True):
        """ExecutionContext::wand (index-search --search-mode wand): block-max pruning."""
        _lib.check(self.L, self.L.irs_hip_batch_set_wand(self.handle, int(enable)),
                   "irs_hip_batch_set_wand")
        return self

    def set_min_scores(self, min_scores):
        """irs::score::Min per query (the harness heap's k-th score so far); None clears."""
        if min_scores is None:
            ptr = None
        else:
            arr = np.ascontiguousarray(min_scores, np.float32)
            assert arr.shape == (self.nq_user,)
            ptr = arr.ctypes.data
        _lib.check(self.L, self.L.irs_hip_batch_set_min_scores(self.handle, ptr),
                   "irs_hip_batch_set_min_scores")
        return self

    def profile(self, enable=True):
        """True / 1: kernel timings; 2: count what the block-driven kernels decode; 3: both."""
        _lib.check(self.L, self.L.irs_hip_batch_profile(self.handle, int(enable)),
                   "irs_hip_batch_profile")
        return self

    def plan(self, stream=None):
        """Queue the planning stage of the next run on `stream` (irs_hip_batch_plan)."""
        _lib.check(self.L, self.L.irs_hip_batch_plan(self.handle, stream), "irs_hip_batch_plan")
        return self

    def run(self, stream=None):
        _lib.check(self.L, self.L.irs_hip_batch_run(self.handle, stream), "irs_hip_batch_run")
        return self

    def timings(self):
        ms = (C.c_float * _lib.K_COUNT)()
        _lib.check(self.L, self.L.irs_hip_batch_timings(self.handle, ms), "irs_hip_batch_timings")
        return [float(x) for x in ms]

    def reruns(self) -> int:
        n = C.c_uint32()
        _lib.check(self.L, self.L.irs_hip_batch_reruns(self.handle, C.byref(n)),
                   "irs_hip_batch_reruns")
        return n.value

    def unit_mask(self, unit: int, n_words: int):
        """The docs unit `unit` (segment * n_queries + query) did not match whatever it scored in
        the last run — deleted plus excluded — as a bit_union-style bitset (bit = doc id)."""
        out = np.zeros(n_words, np.uint64)
        _lib.check(self.L, self.L.irs_hip_batch_unit_mask(self.handle, unit, out.ctypes.data, n_words),
                   "irs_hip_batch_unit_mask")
        return out

    def set_doc_sets(self, sets, row_of_unit=None, n_rows=None, n_words=None):
        """Restrict units to doc sets (irs_hip_batch_set_doc_sets): `sets` u64[rows][words] in
        bit_union's layout (bit = doc id), `row_of_unit` [units] row indices, _lib.NO_DOC_SET for an
        unrestricted unit (unit = segment * n_queries + query).  A numpy array is copied into memory
        of the batch (the host form); a torch tensor on the device — or a device address with
        n_rows / n_words — is BORROWED: it stays valid and unchanged until the results have been
        fetched or the sets are replaced.  None clears the filters."""
        if sets is None or row_of_unit is None:
            self._doc_sets = None
            _lib.check(self.L, self.L.irs_hip_batch_set_doc_sets(self.handle, None, 0, 0, None),
                       "irs_hip_batch_set_doc_sets")
            return self
        rows = np.ascontiguousarray(row_of_unit, np.uint32).reshape(-1)
        if rows.size != self.nq:
            raise ValueError("row_of_unit: one row per unit (%d)" % self.nq)
        if isinstance(sets, np.ndarray):
            arr = np.ascontiguousarray(sets, np.uint64)
            if arr.ndim != 2:
                raise ValueError("doc sets: u64[rows][words]")
            _lib.check(self.L, self.L.irs_hip_batch_set_doc_sets_host(
                self.handle, arr.ctypes.data, arr.shape[0], arr.shape[1], rows.ctypes.data),
                "irs_hip_batch_set_doc_sets_host")
            self._doc_sets = None
            return self
        if hasattr(sets, "data_ptr"):   # a torch tensor: device memory
            if sets.dim() != 2 or sets.element_size() != 8 or not sets.is_contiguous():
                raise ValueError("doc sets: a contiguous 64-bit tensor [rows][words]")
            ptr, n_rows, n_words = sets.data_ptr(), sets.shape[0], sets.shape[1]
        else:
            if n_rows is None or n_words is None:
                raise ValueError("doc sets by device address: n_rows and n_words")
            ptr = int(sets)
        _lib.check(self.L, self.L.irs_hip_batch_set_doc_sets(
            self.handle, ptr, int(n_rows), int(n_words), rows.ctypes.data), "irs_hip_batch_set_doc_sets")
        self._doc_sets = sets   # (borrowed by the library)
        return self

    def doc_set_stats(self):
        """What the doc sets let the last run skip (irs_hip_batch_doc_set_stats): a dict of tiles,
        tiles_skipped (work-item units; exact), leads, leads_skipped (block-driven and phrase
        units; counted under profile(2) only)."""
        v = [C.c_uint64() for _ in range(4)]
        _lib.check(self.L, self.L.irs_hip_batch_doc_set_stats(self.handle, *[C.byref(x) for x in v]),
                   "irs_hip_batch_doc_set_stats")
        return dict(zip(("tiles", "tiles_skipped", "leads", "leads_skipped"), (int(x.value) for x in v)))

    def match_words(self) -> int:
        """The fewest 64-bit words a match-set row may have: a bit for every doc id of the batch's
        largest segment."""
        return max(int(sr.num_docs) for sr in self.segs) // 64 + 1

    def match_sets(self, n_words=None, sets=True):
        """Unscored execution (irs_hip_batch_match_sets): (sets u64[units][n_words] or None,
        counts u64[units]) — every doc each unit (segment * n_queries + query) matches as a
        bit_union-style bitset (bit = doc id), and how many.  sets=False: the counts alone."""
        n_words = self.match_words() if n_words is None else int(n_words)
        out = np.empty((self.nq, n_words), np.uint64) if sets else None
        counts = np.empty(self.nq, np.uint64)
        _lib.check(self.L, self.L.irs_hip_batch_match_sets(
            self.handle, out.ctypes.data if sets else None, n_words, counts.ctypes.data),
            "irs_hip_batch_match_sets")
        return out, counts

    def match_sets_to_device(self, d_sets, n_words: int, d_counts, stream=None):
        """The same into device memory (irs_hip_batch_match_sets_to_device), queued on `stream`:
        d_sets u64[units][n_words], d_counts u64[units]; either may be None."""
        _lib.check(self.L, self.L.irs_hip_batch_match_sets_to_device(
            self.handle, d_sets, int(n_words), d_counts, stream), "irs_hip_batch_match_sets_to_device")
        return self

    def score_docs(self, docs, offsets=None, matched=True):
        """doc_iterator::seek + score for docs the caller names (irs_hip_batch_score_docs).  `docs`:
        a list of arrays, one per unit (segment * n_queries + query), each strictly ascending doc
        ids of the unit's segment — or one flat u32 array with `offsets` u64[units + 1].  Returns
        (scores, matched) in the same shape: the score run() gives the doc under its unit (0 where
        it does not match) and whether it matches; matched=False: (scores, None)."""
        lists = offsets is None
        if lists:
            if len(docs) != self.nq:
                raise ValueError("docs: one list per unit (%d)" % self.nq)
            arrs = [np.ascontiguousarray(d, np.uint32).reshape(-1) for d in docs]
            offsets = np.zeros(self.nq + 1, np.uint64)
            np.cumsum([a.size for a in arrs], out=offsets[1:])
            flat = np.concatenate(arrs) if arrs else np.zeros(0, np.uint32)
        else:
            flat = np.ascontiguousarray(docs, np.uint32).reshape(-1)
            offsets = np.ascontiguousarray(offsets, np.uint64).reshape(-1)
            if offsets.size != self.nq + 1:
                raise ValueError("offsets: units + 1 entries (%d)" % (self.nq + 1))
            if offsets.size and int(offsets[-1]) != flat.size:
                raise ValueError("offsets[-1] != len(docs)")
        flat = np.ascontiguousarray(flat, np.uint32)
        n = max(flat.size, 1)   # (an empty call still hands over valid addresses)
        buf = np.zeros(n, np.uint32)
        buf[:flat.size] = flat
        scores = np.zeros(n, np.float32)
        hit = np.zeros(n, np.uint8) if matched else None
        _lib.check(self.L, self.L.irs_hip_batch_score_docs(
            self.handle, buf.ctypes.data, offsets.ctypes.data, scores.ctypes.data,
            hit.ctypes.data if matched else None), "irs_hip_batch_score_docs")
        scores = scores[:flat.size]
        hit = hit[:flat.size].astype(bool) if matched else None
        if not lists:
            return scores, hit
        cut = offsets[1:-1].astype(np.int64)
        return np.split(scores, cut), (np.split(hit, cut) if matched else None)

    def score_docs_to_device(self, d_docs, d_offsets, n_docs: int, d_scores, d_matched=None, stream=None):
        """The same on device memory (irs_hip_batch_score_docs_to_device), queued on `stream`:
        d_docs u32[n_docs], d_offsets u64[units + 1], d_scores f32[n_docs], d_matched u8[n_docs] or
        None — device addresses.  Docs the host form refuses come back unmatched."""
        _lib.check(self.L, self.L.irs_hip_batch_score_docs_to_device(
            self.handle, d_docs, d_offsets, int(n_docs), d_scores, d_matched, stream),
            "irs_hip_batch_score_docs_to_device")
        return self

    def _nested(self, parents, match, merge, none_boost, n_words=None):
        """(irs_hip_nested, what keeps its parent rows alive): `parents` a numpy u64[n_segs][n_words]
        array — uploaded for the call — or a device address with n_words."""
        lo, hi = match
        d = _lib.Nested()
        d.match_min = int(lo)
        d.match_max = _lib.NESTED_NO_MAX if hi is None else int(hi)
        d.merge, d.none_boost = int(merge), float(none_boost)
        if isinstance(parents, np.ndarray):
            arr = np.ascontiguousarray(parents, np.uint64)
            if arr.ndim == 1:
                arr = arr.reshape(1, -1)
            if arr.ndim != 2 or arr.shape[0] != len(self.segs):
                raise ValueError("parents: u64[n_segs][n_words], a row per segment of the batch")
            buf = DeviceBuffer(self.L, self.seg.device, arr.nbytes).upload(arr)
            d.d_parents, d.n_words = buf.ptr, arr.shape[1]
            return d, buf
        if n_words is None:
            raise ValueError("parents by device address: n_words")
        d.d_parents, d.n_words = int(parents), int(n_words)
        return d, None

    def nested_sets(self, parents, match=(1, None), merge=MERGE_SUM, none_boost=0.0, sets=True, n_words=None):
        """ByNestedFilter, unscored (irs_hip_batch_nested_sets): the batch's queries are the child
        filter, `parents` the parent docs of every segment as bitsets (bit = doc id).  Returns
        (sets u64[units][n_words] or None, counts u64[units]): the parents whose block of children
        holds match = (min, max) of them (max None: no maximum; (0, 0): none; (1, None): any)."""
        d, keep = self._nested(parents, match, merge, none_boost, n_words)
        try:
            out = np.empty((self.nq, int(d.n_words)), np.uint64) if sets else None
            counts = np.empty(self.nq, np.uint64)
            _lib.check(self.L, self.L.irs_hip_batch_nested_sets(
                self.handle, C.byref(d), out.ctypes.data if sets else None, counts.ctypes.data),
                "irs_hip_batch_nested_sets")
        finally:
            if keep is not None:
                keep.close()
        return out, counts

    def nested_sets_to_device(self, parents, d_sets, d_counts, match=(1, None), merge=MERGE_SUM,
                              none_boost=0.0, n_words=None, stream=None):
        """The same into device memory (irs_hip_batch_nested_sets_to_device): d_sets
        u64[units][n_words], d_counts u64[units], device addresses, either may be None — rows that
        irs_hip_batch_set_doc_sets of a parent-level batch takes as they are."""
        d, keep = self._nested(parents, match, merge, none_boost, n_words)
        try:
            _lib.check(self.L, self.L.irs_hip_batch_nested_sets_to_device(
                self.handle, C.byref(d), d_sets, d_counts, stream), "irs_hip_batch_nested_sets_to_device")
        finally:
            if keep is not None:
                keep.close()
        return self

    def nested_topk(self, parents, match=(1, None), merge=MERGE_SUM, none_boost=0.0, n_words=None):
        """ByNestedFilter, scored (irs_hip_batch_nested_topk): (hits HIT[units][k], counts[units],
        totals[units]) — every unit's k best hit parents, each scored by `merge` over its matching
        children's scores ((0, 0): none_boost), ordered (score desc, doc asc)."""
        d, keep = self._nested(parents, match, merge, none_boost, n_words)
        try:
            hits = np.zeros((self.nq, self.k), HIT)
            counts = np.zeros(self.nq, np.uint32)
            totals = np.zeros(self.nq, np.uint64)
            _lib.check(self.L, self.L.irs_hip_batch_nested_topk(
                self.handle, C.byref(d), hits.ctypes.data, self.k, counts.ctypes.data, totals.ctypes.data),
                "irs_hip_batch_nested_topk")
        finally:
            if keep is not None:
                keep.close()
        return hits, counts, totals

    def touched(self):
        """(`.doc` + norm bytes decoded, positions read) by the last run (And / by_phrase)."""
        a, p = C.c_uint64(), C.c_uint64()
        _lib.check(self.L, self.L.irs_hip_batch_touched(self.handle, C.byref(a), C.byref(p)),
                   "irs_hip_batch_touched")
        return a.value, p.value

    def work(self):
        a, p = C.c_uint64(), C.c_uint64()
        _lib.check(self.L, self.L.irs_hip_batch_work(self.handle, C.byref(a), C.byref(p)),
                   "irs_hip_batch_work")
        return a.value, p.value

    def stream_counts(self):
        """(distinct (segment, term) streams of the joined units, streams the last run decoded
        itself): irs_hip_batch_stream_counts — the rest came out of the device's stream cache."""
        d, n = C.c_uint32(), C.c_uint32()
        _lib.check(self.L, self.L.irs_hip_batch_stream_counts(self.handle, C.byref(d), C.byref(n)),
                   "irs_hip_batch_stream_counts")
        return d.value, n.value

    def clause_units(self) -> int:
        """irs_hip_batch_clause_units: the batch's units of Ors with And children
        (IRS_HIP_CLAUSE_AND: k_clause_pilot / k_clause_score)."""
        n = C.c_uint32()
        _lib.check(self.L, self.L.irs_hip_batch_clause_units(self.handle, C.byref(n)), "irs_hip_batch_clause_units")
        return n.value

    def phrase_conj_units(self) -> int:
        """irs_hip_batch_phrase_conj_units: the batch's units of several phrases in one And
        (IRS_HIP_PHRASE_NEXT: k_phrases_and), (segment, query) pairs."""
        n = C.c_uint32()
        _lib.check(self.L, self.L.irs_hip_batch_phrase_conj_units(self.handle, C.byref(n)),
                   "irs_hip_batch_phrase_conj_units")
        return n.value

    def phrase_disj_units(self) -> int:
        """irs_hip_batch_phrase_disj_units: the batch's units of several phrases in one Or
        (IRS_HIP_PHRASE_OR: k_phrases_or), (segment, query) pairs."""
        n = C.c_uint32()
        _lib.check(self.L, self.L.irs_hip_batch_phrase_disj_units(self.handle, C.byref(n)),
                   "irs_hip_batch_phrase_disj_units")
        return n.value

    def tree_units(self) -> int:
        """irs_hip_batch_tree_units: the batch's units of tree queries (IRS_HIP_TREE_NODE entries:
        k_tree_pilot / k_tree_score)."""
        n = C.c_uint32()
        _lib.check(self.L, self.L.irs_hip_batch_tree_units(self.handle, C.byref(n)), "irs_hip_batch_tree_units")
        return n.value

    def wide_units(self) -> int:
        """irs_hip_batch_wide_units: the batch's units of by_terms / wide expansion queries
        (IRS_HIP_OP_MULTITERM), (segment, query) pairs."""
        n = C.c_uint32()
        _lib.check(self.L, self.L.irs_hip_batch_wide_units(self.handle, C.byref(n)), "irs_hip_batch_wide_units")
        return n.value

    def image_counts(self):
        """(distinct bound images the paired launch reads, images the last run made itself):
        irs_hip_batch_image_counts; (0, 0) for a batch that does not pair."""
        d, n = C.c_uint32(), C.c_uint32()
        _lib.check(self.L, self.L.irs_hip_batch_image_counts(self.handle, C.byref(d), C.byref(n)),
                   "irs_hip_batch_image_counts")
        return d.value, n.value

    def rescore_paths(self):
        """irs_hip_batch_rescore_paths: units of the last paired launch that looked up (the window's
        docs only, every staged doc: window too large, every staged doc: no more than k staged)."""
        p = (C.c_uint32 * 3)()
        _lib.check(self.L, self.L.irs_hip_batch_rescore_paths(self.handle, p), "irs_hip_batch_rescore_paths")
        return tuple(int(x) for x in p)

    def results(self):
        hits = np.zeros((self.nq, self.k), HIT)
        counts = np.zeros(self.nq, np.uint32)
        totals = np.zeros(self.nq, np.uint64)
        _lib.check(self.L, self.L.irs_hip_batch_results(
            self.handle, hits.ctypes.data, self.k, counts.ctypes.data, totals.ctypes.data),
            "irs_hip_batch_results")
        if self.multi:
            n = len(self.segs)
            return (hits.reshape(n, self.nq_user, self.k), counts.reshape(n, self.nq_user),
                    totals.reshape(n, self.nq_user))
        return hits, counts, totals

    def results_to_host(self, stream=None):
        """Queue the copy of the checked results to page-locked host memory
        (irs_hip_batch_results_to_host); host_results() waits for it."""
        _lib.check(self.L, self.L.irs_hip_batch_results_to_host(self.handle, stream),
                   "irs_hip_batch_results_to_host")
        return self

    def host_results(self):
        """(hits HIT[nq][k_max], counts[nq], totals[nq]) as numpy VIEWS of the batch's page-locked
        result memory: valid until the batch is closed, run or copied again."""
        hp, cp, tp, ks = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32()
        _lib.check(self.L, self.L.irs_hip_batch_host_results(
            self.handle, C.byref(hp), C.byref(ks), C.byref(cp), C.byref(tp)),
            "irs_hip_batch_host_results")
        k = int(ks.value)
        hits = np.frombuffer((C.c_uint8 * (self.nq * k * HIT.itemsize)).from_address(hp.value), HIT)
        counts = np.frombuffer((C.c_uint8 * (self.nq * 4)).from_address(cp.value), np.uint32)
        totals = np.frombuffer((C.c_uint8 * (self.nq * 8)).from_address(tp.value), np.uint64)
        hits = hits.reshape(self.nq, k)
        if self.multi:
            n = len(self.segs)
            return (hits.reshape(n, self.nq_user, k), counts.reshape(n, self.nq_user),
                    totals.reshape(n, self.nq_user))
        return hits, counts, totals

    def device_results(self):
        dh, dc, km = C.c_void_p(), C.c_void_p(), C.c_uint32()
        _lib.check(self.L, self.L.irs_hip_batch_device_results(
            self.handle, C.byref(dh), C.byref(dc), C.byref(km)), "irs_hip_batch_device_results")
        return dh.value, dc.value, km.value

    def results_to_device(self, d_hits: int, d_counts: int, stream=None):
        _lib.check(self.L, self.L.irs_hip_batch_results_to_device(
            self.handle, d_hits, d_counts, stream), "irs_hip_batch_results_to_device")

    def close(self):
        if self.handle:
            self.L.irs_hip_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stream_cache_stats(L=None, device=0):
    """The device's cache of decoded posting streams (irs_hip_device_stream_cache_stats) as a dict:
    bytes_held, budget, streams, hits, misses, evictions."""
    L = L or _lib.lib()
    st = _lib.StreamCacheStats()
    _lib.check(L, L.irs_hip_device_stream_cache_stats(device, C.byref(st)),
               "irs_hip_device_stream_cache_stats")
    return {name: int(getattr(st, name)) for name, _ in st._fields_}


def cached_images(L=None, device=0):
    """The bound images the device's cache can serve (irs_hip_device_image_count)."""
    L = L or _lib.lib()
    n = C.c_uint64()
    _lib.check(L, L.irs_hip_device_image_count(device, C.byref(n)), "irs_hip_device_image_count")
    return int(n.value)


def join_bound_rule(kind, norm_const, norm_length, tf_bound, L=None):
    """irs_hip_join_bound_rule: (u[256][256] by (tf, norm), U, slack, docs per paired tile), or None
    where the signature gets no image."""
    L = L or _lib.lib()
    u = np.zeros((256, 256), np.uint16)
    scale, slack, tile = C.c_float(), C.c_float(), C.c_uint32()
    rc = L.irs_hip_join_bound_rule(kind, norm_const, norm_length, tf_bound,
                                   u.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(scale),
                                   C.byref(slack), C.byref(tile))
    if rc == _lib.EUNSUPPORTED:
        return None
    _lib.check(L, rc, "irs_hip_join_bound_rule")
    return u, float(scale.value), float(slack.value), int(tile.value)


def join_half_rule(cs, scale, L=None):
    """irs_hip_join_half_rule: the integer weight k of a term weight cs on an image of scale U."""
    L = L or _lib.lib()
    k = C.c_uint32()
    _lib.check(L, L.irs_hip_join_half_rule(cs, scale, C.byref(k)), "irs_hip_join_half_rule")
    return int(k.value)


def join_half_probe(entries, k, high_half, L=None, device=0):
    """irs_hip_join_half_probe: the paired kernel's per-posting helper over `entries` (uint32)."""
    L = L or _lib.lib()
    e = np.ascontiguousarray(entries, np.uint32)
    out = np.zeros(e.size, np.uint32)
    p = C.POINTER(C.c_uint32)
    _lib.check(L, L.irs_hip_join_half_probe(device, e.ctypes.data_as(p), e.size, int(k), int(bool(high_half)),
                                            out.ctypes.data_as(p)), "irs_hip_join_half_probe")
    return out


def set_stream_cache(nbytes, L=None, device=0):
    """The cache's byte budget (irs_hip_device_set_stream_cache); 0 switches it off."""
    L = L or _lib.lib()
    _lib.check(L, L.irs_hip_device_set_stream_cache(device, int(nbytes)),
               "irs_hip_device_set_stream_cache")


# -------------------------------------------------------------------- index --

@dataclass
class SegmentStats:
    """What by_term::prepare reads from a segment without touching postings."""
    docs_with_field: int
    total_term_freq: int
    docs_count: np.ndarray  # per term ordinal: term_meta::docs_count


def prepare(filters, scorer, segment_stats, required_terms=False, optional_terms=False, and_clauses=False,
            phrase_conjunctions=False, phrase_disjunctions=False, boolean_trees=False):
    """filter::prepare for a list of filters against ALL segments: statistics are
    index-global (term_filter.cpp:102-125): D = sum docs_with_field,
    d = sum docs_count of the term, avgdl from the summed field frequency.
    required_terms=True: And([by_phrase, by_term..., Not(...)...]) — a phrase plus required terms,
    IRS_HIP_PHRASE_REQUIRED — is taken.  Off by default: prepare() then refuses the shape as it
    always did (ValueError), so callers that send what prepare() refuses down their CPU path see no
    change until they ask for it.
    optional_terms=True: Or([by_phrase, by_term...]) — a phrase or optional terms,
    IRS_HIP_PHRASE_OPTIONAL — is taken, also as the one included child of And([Or([...]), Not(...)]).
    Off by default in the same way.
    and_clauses=True: Or([And([by_term...]), by_term, Or([...])...]) — an Or with And children, a
    disjunction of clauses, IRS_HIP_CLAUSE_AND (or_clauses) — is taken.  Off by default in the same
    way: without it such an Or is refused as it always was.
    phrase_conjunctions=True: And([by_phrase, by_phrase..., by_term..., Not(...)...]) — two to four
    phrases in one And, plus required terms, IRS_HIP_PHRASE_NEXT — is taken.  Off by default in the
    same way: without it two phrases in one And are refused as they always were.
    phrase_disjunctions=True: Or([by_phrase, by_phrase...]) — two to four phrases in one Or,
    IRS_HIP_PHRASE_OR — is taken, also as the one included child of And([Or([...]), Not(...)...,
    by_doc_set(r)]).  Off by default in the same way: without it two phrases in one Or are refused as
    they always were.
    boolean_trees=True: a tree of by_term / And / Or (with min_match) / Not nested to any depth —
    `a AND (b OR (c AND d))`, `(a AND NOT b) OR c`, IRS_HIP_TREE_NODE (boolean_tree) — is taken where
    every other route, under the flags given, refuses it; a filter one of them takes keeps its route
    and its bytes.  Off by default in the same way: without it every refusal stays as it was."""
    dwf = sum(s.docs_with_field for s in segment_stats)
    ttf = sum(s.total_term_freq for s in segment_stats)
    out = []
    if boolean_trees:
        for flt in filters:
            try:
                out += prepare([flt], scorer, segment_stats, required_terms, optional_terms, and_clauses,
                               phrase_conjunctions, phrase_disjunctions)
            except ValueError:
                out.append(_prepare_tree(flt, scorer, segment_stats, dwf, ttf))
        return out
    for flt in filters:
        flt, doc_set = split_doc_set(flt)
        if doc_set is not None:
            # (the doc set is no part of what is prepared: no score, no statistic)
            p = prepare([flt], scorer, segment_stats, required_terms, optional_terms, and_clauses,
                        phrase_conjunctions, phrase_disjunctions)[0]
            if p.clause is not None:
                raise ValueError("a by_doc_set on an Or with And children is not on the GPU path "
                                 "(its units read the streams every unit shares)")
            p.doc_set = doc_set
            out.append(p)
            continue
        flt, excluded = split_exclusions(flt)
        if excluded:
            # (the excluded part is prepared without scorers: no score, no statistic)
            p = prepare([flt], scorer, segment_stats, required_terms, optional_terms, and_clauses,
                        phrase_conjunctions, phrase_disjunctions)[0]
            if p.clause is not None:
                raise ValueError("Not around an Or with And children (((a AND b) OR c) AND NOT d) is "
                                 "not on the GPU path")
            p.excluded = [int(t) for t in excluded]
            out.append(p)
            continue
        if isinstance(flt, by_terms):
            # statistics per term exactly as for an Or of by_terms: the field's over the whole
            # index, the term's summed over the segments that hold it
            flt.check()
            scorers = []
            for t, tb in flt.pairs():
                dwt = sum(int(st.docs_count[t]) for st in segment_stats if 0 <= t < len(st.docs_count))
                stats = scorer.collect(dwf, dwt, ttf)
                scorers.append(scorer.term_scorer(stats, tb if flt.boost == 1.0 else f32(f32(flt.boost) * f32(tb))))
            out.append(PreparedQuery(OP_MULTITERM, [t for t, _ in flt.pairs()], scorers, int(flt.min_match)))
            continue
        if isinstance(flt, by_phrase) and flt.variadic:
            out.append(_prepare_variadic(flt, scorer, segment_stats, dwf, ttf))
            continue
        if isinstance(flt, by_phrase):
            one = _phrase_scorer(flt, flt.boost, scorer, segment_stats, dwf, ttf)
            out.append(PreparedQuery(OP_PHRASE, list(flt.terms), [one] * len(flt.terms), 0,
                                     [int(o) for o in flt.offsets]))
            continue
        if phrase_disjunctions and type(flt) is Or and sum(isinstance(s, by_phrase) for s in flt.subs) > 1:
            out.append(_prepare_phrases_or(flt, scorer, segment_stats, dwf, ttf))
            continue
        if type(flt) is Or and optional_terms and any(isinstance(s, by_phrase) for s in flt.subs):
            out.append(_prepare_phrase_or(flt, scorer, segment_stats, dwf, ttf))
            continue
        if (phrase_conjunctions and type(flt) is And and flt.op == OP_AND and
                sum(isinstance(s, by_phrase) for s in flt.subs) > 1):
            out.append(_prepare_phrases_and(flt, scorer, segment_stats, dwf, ttf))
            continue
        if isinstance(flt, (Or, And)) and any(isinstance(s, by_phrase) for s in flt.subs):
            if type(flt) is And and not required_terms:
                raise ValueError("a by_phrase next to other children of an And (a phrase plus required "
                                 "terms, IRS_HIP_PHRASE_REQUIRED) is taken by "
                                 "prepare(..., required_terms=True)")
            out.append(_prepare_phrase_and(flt, scorer, segment_stats, dwf, ttf))
            continue
        if type(flt) is And and (flt.boost != 1.0 or any(type(s) is not by_term for s in flt.subs)):
            out.append(_prepare_groups(flt, scorer, segment_stats, dwf, ttf))
            continue
        if and_clauses and type(flt) is Or and any(type(s) is not by_term for s in flt.subs):
            out.append(_prepare_clauses(flt, scorer, segment_stats, dwf, ttf))
            continue
        op, subs = _terms_of(flt)
        mult = float(getattr(flt, "boost", 1.0)) if type(flt) is not by_term else 1.0
        scorers = []
        for s in subs:
            dwt = 0
            for st in segment_stats:
                if 0 <= s.term < len(st.docs_count):
                    dwt += int(st.docs_count[s.term])
            stats = scorer.collect(dwf, dwt, ttf)
            scorers.append(scorer.term_scorer(stats, s.boost if mult == 1.0 else f32(f32(mult) * f32(s.boost))))
        out.append(PreparedQuery(op, [s.term for s in subs], scorers,
                                 int(getattr(flt, "min_match", 0)),
                                 merge=int(getattr(flt, "merge", MERGE_SUM))))
    return out


def _phrase_scorer(flt, boost, scorer, segment_stats, dwf, ttf):
    """FixedPrepareCollect (phrase_filter.cpp:212-293): term_stats.finish() of every phrase term
    lands in ONE stats blob — BM25::collect / TFIDF::collect do `idf +=` (bm25.cpp:381-383,
    tfidf.cpp:272-275), the norm constants are equal."""
    idf = f32(0)
    stats = None
    for t in flt.terms:
        dwt = sum(int(st.docs_count[t]) for st in segment_stats
                  if 0 <= t < len(st.docs_count))
        stats = scorer.collect(dwf, dwt, ttf)
        idf = f32(idf + stats.idf)
    return scorer.term_scorer(TermStats(idf, stats.norm_const, stats.norm_length), boost)


def _prepare_phrase_and(flt, scorer, segment_stats, dwf, ttf):
    """prepare() of And([by_phrase, by_term...]) — a phrase plus required terms (And::prepare ->
    make_conjunction over the children, boolean_filter.cpp:150-210): the phrase gets its
    FixedPrepareCollect blob from its own words, every by_term its own statistics; the And's boost
    multiplies into every child's in float32.  Entries: the phrase's words, then the required terms
    (IRS_HIP_PHRASE_REQUIRED).  What is taken: ONE by_phrase of plain terms, at least one by_term,
    merge SUM, at most 8 words and terms in all (Not children were split off before)."""
    taken = ("an And takes ONE by_phrase of plain terms plus by_term children "
             "(and Not children), merged with SUM")
    if type(flt) is not And or flt.op != OP_AND:
        raise ValueError("a by_phrase inside an Or is not on the GPU path: " + taken)
    phrases = [s for s in flt.subs if isinstance(s, by_phrase)]
    others = [s for s in flt.subs if not isinstance(s, by_phrase)]
    if len(phrases) > 1:
        raise ValueError("two phrases in one And are not on the GPU path: " + taken)
    ph = phrases[0]
    if ph.variadic:
        raise ValueError("a variadic by_phrase with required terms is not on the GPU path: " + taken)
    for s in others:
        if type(s) is Or:
            raise ValueError("an Or group next to a by_phrase is not on the GPU path: " + taken)
        if type(s) is not by_term:
            raise ValueError("%s next to a by_phrase is not on the GPU path: %s" % (type(s).__name__, taken))
    if not others:
        raise ValueError("an And of one by_phrase alone is that phrase: send the by_phrase itself "
                         "(or under And([..., Not(...)]))")
    if flt.merge != MERGE_SUM:
        raise ValueError("an And with a by_phrase child merges with SUM on the GPU path "
                         "(MAX / MIN over a phrase and terms are not built)")
    if len(ph.terms) < 2:
        raise ValueError("a by_phrase of one term is a by_term: " + taken)
    if len(ph.terms) + len(others) > _lib.MAX_PHRASE_TERMS:
        raise ValueError("a by_phrase plus required terms has at most %d entries in all"
                         % _lib.MAX_PHRASE_TERMS)
    mult = f32(flt.boost)
    one = _phrase_scorer(ph, f32(mult * f32(ph.boost)), scorer, segment_stats, dwf, ttf)
    terms, scorers = list(ph.terms), [one] * len(ph.terms)
    for s in others:
        dwt = sum(int(st.docs_count[s.term]) for st in segment_stats if 0 <= s.term < len(st.docs_count))
        terms.append(s.term)
        scorers.append(scorer.term_scorer(scorer.collect(dwf, dwt, ttf), f32(mult * f32(s.boost))))
    return PreparedQuery(OP_PHRASE, terms, scorers, 0, [int(o) for o in ph.offsets] + [0] * len(others),
                         required=[False] * len(ph.terms) + [True] * len(others))


def _prepare_phrases_and(flt, scorer, segment_stats, dwf, ttf):
    """prepare() of And([by_phrase, by_phrase..., by_term...]) — several phrases in one And, plus
    required terms (And::prepare -> make_conjunction over the children, boolean_filter.cpp:150-210):
    every phrase gets its OWN FixedPrepareCollect blob from its own words, every by_term its own
    statistics; the And's boost multiplies into every child's in float32.  Entries: the words of
    phrase 1, of phrase 2 (its first word with IRS_HIP_PHRASE_NEXT), ..., then the required terms
    (IRS_HIP_PHRASE_REQUIRED).  What is taken: 2-4 phrases of plain terms, each of at least two
    words, 0 or more by_term children, merge SUM, at most 8 words and terms in all (Not children
    were split off before)."""
    taken = ("an And takes 2-4 by_phrase children of plain terms (two words or more each) plus "
             "by_term children (and Not children), merged with SUM, at most %d words and terms in all"
             % _lib.MAX_PHRASE_TERMS)
    phrases = [s for s in flt.subs if isinstance(s, by_phrase)]
    others = [s for s in flt.subs if not isinstance(s, by_phrase)]
    if any(ph.variadic for ph in phrases):
        raise ValueError("a variadic by_phrase next to another phrase is not on the GPU path: " + taken)
    for s in others:
        if type(s) is Or:
            raise ValueError("an Or group next to by_phrase children is not on the GPU path: " + taken)
        if type(s) is not by_term:
            raise ValueError("%s next to by_phrase children is not on the GPU path: %s" % (type(s).__name__, taken))
    if flt.merge != MERGE_SUM:
        raise ValueError("an And with by_phrase children merges with SUM on the GPU path "
                         "(MAX / MIN over phrases and terms are not built)")
    if any(len(ph.terms) < 2 for ph in phrases):
        raise ValueError("a by_phrase of one term is a by_term: " + taken)
    if len(phrases) > 4:
        raise ValueError("more than four phrases in one And are not on the GPU path: " + taken)
    if sum(len(ph.terms) for ph in phrases) + len(others) > _lib.MAX_PHRASE_TERMS:
        raise ValueError("phrases plus required terms have at most %d entries in all" % _lib.MAX_PHRASE_TERMS)
    mult = f32(flt.boost)
    terms, scorers, offsets, opens = [], [], [], []
    for i, ph in enumerate(phrases):
        one = _phrase_scorer(ph, f32(mult * f32(ph.boost)), scorer, segment_stats, dwf, ttf)
        terms += list(ph.terms)
        scorers += [one] * len(ph.terms)
        offsets += [int(o) for o in ph.offsets]
        opens += [i > 0] + [False] * (len(ph.terms) - 1)
    n_words = len(terms)
    for s in others:
        dwt = sum(int(st.docs_count[s.term]) for st in segment_stats if 0 <= s.term < len(st.docs_count))
        terms.append(s.term)
        scorers.append(scorer.term_scorer(scorer.collect(dwf, dwt, ttf), f32(mult * f32(s.boost))))
    return PreparedQuery(OP_PHRASE, terms, scorers, 0, offsets + [0] * len(others),
                         required=([False] * n_words + [True] * len(others)) if others else None,
                         opens=opens + [False] * len(others))


def _prepare_phrases_or(flt, scorer, segment_stats, dwf, ttf):
    """prepare() of Or([by_phrase, by_phrase...]) — several phrases in one Or (Or::prepare prepares
    every child on its own, boolean_filter.cpp:150-210; MakeDisjunction over PhraseIterators,
    disjunction.hpp:1411-1467): every phrase gets its OWN FixedPrepareCollect blob from its own
    words; the Or's boost multiplies into every phrase's in float32.  Entries: the words of phrase 1,
    of phrase 2 (its first word with IRS_HIP_PHRASE_OR), ...  What is taken: 2-4 phrases of plain
    terms, each of at least two words, nothing else, min_match <= 1, merge SUM, at most 8 words in
    all (Not children and a by_doc_set were split off before)."""
    taken = ("an Or takes 2-4 by_phrase children of plain terms (two words or more each) and nothing "
             "else, min_match <= 1, merged with SUM, at most %d words in all" % _lib.MAX_PHRASE_TERMS)
    phrases = [s for s in flt.subs if isinstance(s, by_phrase)]
    others = [s for s in flt.subs if not isinstance(s, by_phrase)]
    if any(ph.variadic for ph in phrases):
        raise ValueError("a variadic by_phrase next to another phrase in an Or is not on the GPU path: " + taken)
    for s in others:
        raise ValueError("%s next to several by_phrase children of an Or is not on the GPU path: %s"
                         % (type(s).__name__, taken))
    if flt.min_match > 1:
        raise ValueError("an Or of by_phrase children with min_match > 1 is not on the GPU path: " + taken)
    if flt.merge != MERGE_SUM:
        raise ValueError("an Or of by_phrase children merges with SUM on the GPU path "
                         "(MAX / MIN over phrases are not built)")
    if any(len(ph.terms) < 2 for ph in phrases):
        raise ValueError("a by_phrase of one term is a by_term: " + taken)
    if len(phrases) > 4:
        raise ValueError("more than four phrases in one Or are not on the GPU path: " + taken)
    if sum(len(ph.terms) for ph in phrases) > _lib.MAX_PHRASE_TERMS:
        raise ValueError("the phrases of an Or have at most %d words in all" % _lib.MAX_PHRASE_TERMS)
    mult = f32(flt.boost)
    terms, scorers, offsets, opens = [], [], [], []
    for i, ph in enumerate(phrases):
        one = _phrase_scorer(ph, f32(mult * f32(ph.boost)), scorer, segment_stats, dwf, ttf)
        terms += list(ph.terms)
        scorers += [one] * len(ph.terms)
        offsets += [int(o) for o in ph.offsets]
        opens += [i > 0] + [False] * (len(ph.terms) - 1)
    return PreparedQuery(OP_PHRASE, terms, scorers, 0, offsets, or_opens=opens)


def _prepare_phrase_or(flt, scorer, segment_stats, dwf, ttf):
    """prepare() of Or([by_phrase, by_term...]) — a phrase or optional terms (Or::prepare prepares
    every child on its own, boolean_filter.cpp:150-210; MakeDisjunction over {PhraseIterator, term
    iterators}, disjunction.hpp:1411-1467): the phrase gets its FixedPrepareCollect blob from its
    own words, every by_term its own statistics; the Or's boost (and those of nested SUM Ors of
    terms, flattened as _or_members does) multiplies into every child's in float32.  Entries: the
    phrase's words, then the optional terms (IRS_HIP_PHRASE_OPTIONAL).  What is taken: ONE by_phrase
    of plain terms, min_match <= 1, merge SUM, at most 8 words and terms in all."""
    taken = ("an Or takes ONE by_phrase of plain terms plus by_term children (and SUM Ors of "
             "by_term), min_match <= 1, merged with SUM")
    phrases = [s for s in flt.subs if isinstance(s, by_phrase)]
    others = [s for s in flt.subs if not isinstance(s, by_phrase)]
    if len(phrases) > 1:
        raise ValueError("two phrases in one Or are not on the GPU path: " + taken)
    ph = phrases[0]
    if ph.variadic:
        raise ValueError("a variadic by_phrase with optional terms is not on the GPU path: " + taken)
    if flt.min_match > 1:
        raise ValueError("an Or with a by_phrase child and min_match > 1 is not on the GPU path: " + taken)
    if flt.merge != MERGE_SUM and len(flt.subs) > 1:
        raise ValueError("an Or with a by_phrase child merges with SUM on the GPU path "
                         "(MAX / MIN over a phrase and terms are not built)")
    if any(isinstance(s, And) for s in others):
        raise ValueError("an And child next to a by_phrase in an Or ((a AND b) OR \"c d\") is not on "
                         "the GPU path: " + taken)
    if len(ph.terms) < 2:
        raise ValueError("a by_phrase of one term is a by_term: " + taken)
    mult = f32(flt.boost)
    # (a by_phrase in a nested Or, Not, min_match > 1 or non-SUM nested Ors: refused there)
    members = _or_members(replace(flt, subs=others), mult)
    if len(ph.terms) + len(members) > _lib.MAX_PHRASE_TERMS:
        raise ValueError("a by_phrase plus optional terms has at most %d entries in all"
                         % _lib.MAX_PHRASE_TERMS)
    one = _phrase_scorer(ph, f32(mult * f32(ph.boost)), scorer, segment_stats, dwf, ttf)
    terms, scorers = list(ph.terms), [one] * len(ph.terms)
    for t, boost in members:
        dwt = sum(int(st.docs_count[t]) for st in segment_stats if 0 <= t < len(st.docs_count))
        terms.append(t)
        scorers.append(scorer.term_scorer(scorer.collect(dwf, dwt, ttf), boost))
    p = PreparedQuery(OP_PHRASE, terms, scorers, 0, [int(o) for o in ph.offsets] + [0] * len(members))
    if members:   # (an Or of the phrase alone is the phrase)
        p.optional = [False] * len(ph.terms) + [True] * len(members)
    return p


def _prepare_groups(flt, scorer, segment_stats, dwf, ttf):
    """prepare() of an And with Or children: per-term statistics as for any by_term, the boost
    product per member; every member after a group's first flagged IRS_HIP_GROUP_ALT.  A tree
    whose groups all have one member is a flat And, sent as one."""
    groups = and_groups(flt)
    terms, scorers, alts = [], [], []
    for g in groups:
        for i, (t, boost) in enumerate(g):
            dwt = sum(int(st.docs_count[t]) for st in segment_stats if 0 <= t < len(st.docs_count))
            terms.append(t)
            scorers.append(scorer.term_scorer(scorer.collect(dwf, dwt, ttf), boost))
            alts.append(i > 0)
    return PreparedQuery(OP_AND, terms, scorers, int(flt.min_match), merge=int(flt.merge),
                         alts=alts if any(alts) else None)


def _prepare_clauses(flt, scorer, segment_stats, dwf, ttf):
    """prepare() of an Or with And children (Or::prepare prepares every child on its own,
    boolean_filter.cpp:150-210): per-term statistics as for any by_term, the boost product per
    member; every member after a clause's first flagged IRS_HIP_CLAUSE_AND; min_match counts
    clauses.  A tree whose clauses all have one member is a flat Or, sent as one."""
    clauses = or_clauses(flt)
    terms, scorers, more = [], [], []
    for c in clauses:
        for i, (t, boost) in enumerate(c):
            dwt = sum(int(st.docs_count[t]) for st in segment_stats if 0 <= t < len(st.docs_count))
            terms.append(t)
            scorers.append(scorer.term_scorer(scorer.collect(dwf, dwt, ttf), boost))
            more.append(i > 0)
    return PreparedQuery(flt.op, terms, scorers, int(flt.min_match), merge=MERGE_SUM,
                         clause=more if any(more) else None)


def _prepare_tree(flt, scorer, segment_stats, dwf, ttf):
    """prepare() of a nested boolean filter the other routes refuse (And::prepare / Or::prepare
    prepare every child on its own, boolean_filter.cpp:55-312): normalised (boolean_tree), then the
    root's children in prefix order — per leaf the statistics of any by_term and its boost product,
    a negated leaf without scorer, a node entry per inner node.  A tree that normalises to one level
    is sent as the flat query it is."""
    tree = boolean_tree(flt)
    if tree[0] == "leaf":
        tree = ("node", OP_OR, 0, [(False, tree)])
    entries, n_leaves, n_nodes = tree_entries(tree)
    if n_leaves > _lib.MAX_TERMS:
        raise ValueError("a nested boolean filter has at most %d leaves in all, Nots included" % _lib.MAX_TERMS)
    if n_nodes > _lib.MAX_TERMS - 1:
        raise ValueError("a nested boolean filter has at most %d inner nodes below its root" % (_lib.MAX_TERMS - 1))

    def one(t, boost):
        dwt = sum(int(st.docs_count[t]) for st in segment_stats if 0 <= t < len(st.docs_count))
        return scorer.term_scorer(scorer.collect(dwf, dwt, ttf), boost)

    _, op, min_match, _ = tree
    if n_nodes == 0:     # one level: a flat Or / And / min-match, the negated leaves behind it
        leaves = [e for e in entries if e[0] == "leaf"]
        return PreparedQuery(op, [e[1] for e in leaves], [one(e[1], e[2]) for e in leaves], min_match,
                             merge=MERGE_SUM, excluded=[e[1] for e in entries if e[0] == "not"])
    terms, scorers, marks = [], [], []
    for e in entries:
        if e[0] == "leaf":
            terms.append(e[1]); scorers.append(one(e[1], e[2])); marks.append(None)
        elif e[0] == "not":
            terms.append(e[1]); scorers.append((EXCLUDE, f32(0), f32(0), f32(0))); marks.append("not")
        else:
            terms.append(None); scorers.append((0, f32(0), f32(0), f32(0))); marks.append(tuple(e[1:]))
    return PreparedQuery(op, terms, scorers, min_match, merge=MERGE_SUM, tree=marks)


def variadic_slots(parts, segment_stats):
    """VariadicPrepareCollect's statistics (phrase_filter.cpp:295-432) — docs_with_term of every
    collector slot, collector after collector.  In each segment a part's visitor yields its members
    present there (docs_count > 0) in dictionary order, and the i-th of them is collected into slot
    i (term_offset_ restarts per segment, :159-186) of collector phrase_part_stats[found_parts]:
    the count of parts that had members in that segment before this one."""
    slots = [[] for _ in parts]
    for st in segment_stats:
        found = 0
        for part in parts:
            present = [t for t in part if 0 <= t < len(st.docs_count) and int(st.docs_count[t]) > 0]
            col = slots[found]
            for i, t in enumerate(present):
                if i == len(col):
                    col.append(0)
                col[i] += int(st.docs_count[t])
            found += 1 if present else 0
    return [dwt for col in slots for dwt in col]


def _prepare_variadic(flt, scorer, segment_stats, dwf, ttf):
    """prepare() of a variadic by_phrase: ONE stats blob into which every slot was finished in
    collector order (`idf +=`), entries part after part, every member after a part's first flagged
    IRS_HIP_PHRASE_ALT."""
    parts = flt.parts()
    idf = f32(0)
    stats = scorer.collect(dwf, 0, ttf)   # (no slot at all: nothing matches; same norm constants)
    for dwt in variadic_slots(parts, segment_stats):
        stats = scorer.collect(dwf, dwt, ttf)
        idf = f32(idf + stats.idf)
    one = scorer.term_scorer(TermStats(idf, stats.norm_const, stats.norm_length), flt.boost)
    terms, offs, alts = [], [], []
    for part, off in zip(parts, flt.offsets):
        for i, t in enumerate(part):
            terms.append(t)
            offs.append(int(off))
            alts.append(i > 0)
    return PreparedQuery(OP_PHRASE, terms, [one] * len(terms), 0, offs, alts=alts)


def merge_topk_host(per_segment, k: int):
    """Global top-k over segments ordered (score desc, segment asc, doc asc) —
    the ordering tests/search/wand_test.cpp:72-86 fixes for the harness heap.
    per_segment: list of (hits HIT[nq][k], counts[nq]). Host-side variant used by
    tests; the GPU variant is irs_hip_merge_topk."""
    nq = len(per_segment[0][1])
    out = []
    for q in range(nq):
        rows = []
        for s, (hits, counts) in enumerate(per_segment):
            n = int(counts[q])
            for i in range(n):
                rows.append((-float(hits[q, i]["score"]), s, int(hits[q, i]["doc"])))
        rows.sort()
        out.append([(-a, s, d) for a, s, d in rows[:k]])
    return out


# ---------------------------------------------- scored multi-term expansion --
# by_prefix / by_wildcard / by_range WITH scorers (MultiTermQuery, multiterm_query.cpp:112-184):
# the filter's term visitor hands every visited term of every segment to a
# limited_sample_collector (limited_sample_collector.hpp:43-120) which keeps the
# `scored_terms_limit` (segment, term) states with the LONGEST postings — key = (docs_count, then
# the term's offset in the segment's visit), larger wins, a newcomer replaces the smallest only
# when strictly larger — as SCORED states; everything else is unscored.  execute() is then a
# disjunction (min_match 1, Sum) of one scored iterator per scored state and ONE
# lazy_bitset_iterator over the unscored terms: a doc matches when any visited term holds it, its
# score is the sum over the scored terms holding it (0 for docs only unscored terms hold).
# Statistics (limited_sample_collector::score :123-165): per distinct term the field statistics of
# the WHOLE index and term statistics collected from the segments where the term is SCORED only.
#
# On this path: the scored part is an ordinary Or of <= IRS_HIP_MAX_TERMS by_term filters — the
# scored_terms_limit of the reference's benchmark (scripts/search-benchmark.sh:
# --scored-terms-limit=16) fits — with a term absent from the segments where it is unscored; with
# more scored states, up to IRS_HIP_MAX_WIDE_TERMS (limits up to 64: ArangoSearch ships 128, the
# reference's default is 1024, range_filter.hpp:58), it is one by_terms query with min_match 1
# (IRS_HIP_OP_MULTITERM) over the same slots.  The unscored part and the total are
# irs_hip_bit_union, as in the reference.

def scored_states(visits_docs_counts, limit: int):
    """limited_sample_collector::collect over the segments' visits in order.
    visits_docs_counts[s] = docs_count of the terms segment s's visit yields, in visit order.
    -> sorted list of (segment, offset) that end up scored."""
    # (which of two EQUAL keys — the same docs_count at the same visit offset in two segments — is
    # the heap's root is decided by std::push_heap / std::pop_heap themselves: the binary heap below
    # moves its elements exactly as libstdc++'s does, so ties resolve as in the reference)
    rows = []          # (frequency, offset, segment) per scored state
    order = []         # binary min-heap of indices into rows
    above = lambda i, j: rows[j][:2] < rows[i][:2]            # row i sorts behind row j

    def sift_in(hole, idx):                                    # std::__push_heap
        while hole > 0 and above(order[(hole - 1) // 2], idx):
            order[hole] = order[(hole - 1) // 2]
            hole = (hole - 1) // 2
        order[hole] = idx

    def drop_root_to_back():                                   # std::pop_heap
        idx, order[-1] = order[-1], order[0]
        n, hole, child = len(order) - 1, 0, 0
        while child < (n - 1) // 2:
            child = 2 * (child + 1)
            if above(order[child], order[child - 1]):
                child -= 1
            order[hole] = order[child]
            hole = child
        if n % 2 == 0 and child == (n - 2) // 2:
            child = 2 * (child + 1)
            order[hole] = order[child - 1]
            hole = child - 1
        sift_in(hole, idx)

    for s, counts in enumerate(visits_docs_counts):
        for off, f in enumerate(counts):
            if limit <= 0:
                continue
            if len(rows) < limit:
                rows.append((int(f), off, s))
                order.append(len(rows) - 1)
                sift_in(len(order) - 1, order[-1])
            elif rows[order[0]][:2] < (int(f), off):         # strictly larger keys only
                root = order[0]
                drop_root_to_back()
                rows[root] = (int(f), off, s)
                sift_in(len(order) - 1, order[-1])
    return sorted((s, off) for _, off, s in rows)


def _scored_states_fast(visits_docs_counts, limit: int):
    """scored_states without the heap where the outcome does not depend on it: the collector keeps
    the `limit` largest keys (docs_count, offset); only when the key at the cut also occurs right
    behind it (the same docs_count at the same offset in two segments) the heap's own order
    decides, and the emulation runs."""
    if limit <= 0:
        return []
    seg = np.concatenate([np.full(len(c), s, np.int64) for s, c in enumerate(visits_docs_counts)] or [np.zeros(0, np.int64)])
    off = np.concatenate([np.arange(len(c), dtype=np.int64) for c in visits_docs_counts] or [np.zeros(0, np.int64)])
    frq = np.concatenate([np.asarray(c, np.int64) for c in visits_docs_counts] or [np.zeros(0, np.int64)])
    if frq.size <= limit:
        return sorted(zip(seg.tolist(), off.tolist()))
    order = np.lexsort((off, frq))[::-1]          # by (docs_count, offset), largest first
    a, b = order[limit - 1], order[limit]
    if frq[a] == frq[b] and off[a] == off[b]:
        return scored_states(visits_docs_counts, limit)
    top = order[:limit]
    return sorted(zip(seg[top].tolist(), off[top].tolist()))


class PreparedExpansion:
    """One scored multi-term filter prepared against all segments."""

    def __init__(self, scored, scored_in, unscored_in, scorers, visited_in=None, slots=None,
                 present=None, c0=None, limit=None):
        self.scored = scored            # distinct scored term ordinals (query term slots)
        self.scored_in = scored_in      # [segment] -> set of scored ordinals there
        self._unscored_in = unscored_in  # (None: worked out from visited_in when asked for)
        self.scorers = scorers          # (kind, c0, norm_const, norm_length) per slot
        self.visited_in = visited_in    # [segment] -> np.uint32 ordinals the visitor yielded there
        self.slots = slots              # `scored` as np.uint32
        self.present = present          # bool [segment][slot]: the slot's term is scored in the segment
        self.c0 = c0                    # float32 per slot (scorers[j][1])
        self.limit = limit              # the scored_terms_limit it was prepared with (None: not known)

    @property
    def unscored_in(self):
        """[segment] -> np.uint32 ordinals that are visited but unscored there (visit order)."""
        if self._unscored_in is None:
            self._unscored_in = [
                va[~np.isin(va, np.fromiter(sc, np.uint32, len(sc)))] if sc else va
                for va, sc in zip(self.visited_in, self.scored_in)]
        return self._unscored_in

    def n_unscored(self, s: int) -> int:
        return len(self.visited_in[s]) - len(self.scored_in[s]) if self._unscored_in is None \
            else len(self._unscored_in[s])


def _top_offsets_padded(visit_arrays, lens, flat_counts, limit):
    """-> (rows, cols) of the `limit` largest (docs_count, offset) keys of every visit, offsets
    ascending within a row; flat_counts = the docs_counts of the concatenated visits."""
    nq = len(visit_arrays)
    width = int(lens.max()) if nq else 0
    if limit <= 0 or width == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    inside = np.arange(width)[None, :] < lens[:, None]       # row-major order = concatenation order
    key = np.full((nq, width), -1, np.int64)
    key[inside] = flat_counts * (1 << 24) + np.broadcast_to(np.arange(width), (nq, width))[inside]
    if width > limit:
        top = np.argpartition(key, width - limit, axis=1)[:, width - limit:]
    else:
        top = np.broadcast_to(np.arange(width), (nq, width)).copy()
    top.sort(axis=1)                                          # offsets ascending = ordinals ascending
    ok = np.take_along_axis(key, top, axis=1) >= 0
    rows = np.broadcast_to(np.arange(nq)[:, None], top.shape)[ok]
    return rows, top[ok]


def _top_offsets_one_segment(visit_arrays, counts_of, limit):
    """The collector's choice for MANY filters over ONE segment at once: offsets are unique within
    a visit, so it keeps the `limit` largest (docs_count, offset) keys — no heap order involved.
    -> (rows, cols, lens): for filter q the scored visit offsets cols[rows == q], ascending.
    Long visits (a wildcard: thousands of mostly rare terms) first drop everything below a
    docs_count that still leaves every filter its `limit` largest: the keys are then sorted out
    among a few percent of the elements."""
    nq = len(visit_arrays)
    lens = np.fromiter((len(v) for v in visit_arrays), np.int64, nq)
    if limit <= 0 or nq == 0 or int(lens.max()) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), lens
    flat = np.concatenate(visit_arrays)
    cnt = counts_of[flat]
    keep_about = 4 * limit * nq
    if len(flat) <= 4 * keep_about:
        rows, cols = _top_offsets_padded(visit_arrays, lens, cnt, limit)
        return rows, cols, lens
    # a docs_count that about 4 * limit elements per filter reach (from a sample)
    sample = cnt[:: max(1, len(flat) // 16384)]
    cut = np.partition(sample, len(sample) - 1 - min(len(sample) - 1, (keep_about * len(sample)) // len(flat)))[
        len(sample) - 1 - min(len(sample) - 1, (keep_about * len(sample)) // len(flat))]
    at = np.flatnonzero(cnt >= cut)
    ends = np.cumsum(lens)
    row_at = np.searchsorted(ends, at, side="right")
    above = np.bincount(row_at, minlength=nq)
    settled = (above >= limit) | (above == lens)       # the `limit` largest are all at or above the cut
    rows_out, cols_out = [], []
    if settled.any():
        sel = settled[row_at]
        sub_rows_all, sub_at = row_at[sel], at[sel]
        ids = np.flatnonzero(settled)
        # the kept elements of the settled filters as (shorter) visits of their own: positions in
        # the original visit are what the keys need, so they ride along
        sub_lens = above[ids]
        sub_col = sub_at - (ends - lens)[sub_rows_all]            # offset in the original visit
        width = int(sub_lens.max())
        inside = np.arange(width)[None, :] < sub_lens[:, None]
        key = np.full((len(ids), width), -1, np.int64)
        key[inside] = cnt[sub_at] * (1 << 24) + sub_col
        if width > limit:
            top = np.argpartition(key, width - limit, axis=1)[:, width - limit:]
        else:
            top = np.broadcast_to(np.arange(width), (len(ids), width)).copy()
        picked = np.take_along_axis(key, top, axis=1)
        picked = np.where(picked >= 0, picked & ((1 << 24) - 1), 1 << 30)     # -> original offsets
        picked.sort(axis=1)
        ok = picked < (1 << 30)
        rows_out.append(np.broadcast_to(ids[:, None], picked.shape)[ok])
        cols_out.append(picked[ok])
    rest = np.flatnonzero(~settled)
    if rest.size:                                       # (few: the cut was too high for them)
        starts = ends - lens
        sub = [visit_arrays[q] for q in rest]
        sub_cnt = np.concatenate([cnt[starts[q]:ends[q]] for q in rest])
        r, c = _top_offsets_padded(sub, lens[rest], sub_cnt, limit)
        rows_out.append(rest[r])
        cols_out.append(c)
    rows, cols = np.concatenate(rows_out), np.concatenate(cols_out)
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], lens


def prepare_expansions(visits, limit, scorer, segment_stats, boost=1.0):
    """filter::prepare of scored multi-term filters: visits[q][s] = term ordinals the filter's
    visitor yields in segment s (ascending term order, as term_reader::iterator() enumerates).
    The statistics of all scored terms of all filters are worked out at once (numpy), value for
    value what scorer.collect / term_scorer yield one term at a time.  `limit` (scored_terms_limit):
    the scored states of a filter are at most `limit` query term slots.  Limits up to 64 are taken
    (expansion_arrays); a filter prepared with a larger one is what it always was — an Or of all its
    slots, which batch create refuses beyond IRS_HIP_MAX_TERMS."""
    dwf = sum(s.docs_with_field for s in segment_stats)
    ttf = sum(s.total_term_freq for s in segment_stats)
    dcs = [np.asarray(st.docs_count) for st in segment_stats]
    n_segs = len(segment_stats)
    parts, all_dwt = [], []
    if n_segs == 1 and len(visits):
        # one segment: every filter's choice in a few array operations
        vas = [np.asarray(per_seg[0], np.uint32) for per_seg in visits]
        rows, cols, lens = _top_offsets_one_segment(vas, dcs[0].astype(np.int64), limit)
        starts = np.cumsum(lens) - lens
        flat = np.concatenate(vas) if len(vas) else np.zeros(0, np.uint32)
        at = starts[rows] + cols
        scored_flat = flat[at]
        all_dwt = dcs[0][scored_flat.astype(np.int64)].astype(np.float64)
        per_q = np.bincount(rows, minlength=len(vas)) if len(rows) else np.zeros(len(vas), np.int64)
        scored_parts = np.split(scored_flat, np.cumsum(per_q)[:-1])
        for va, sp in zip(vas, scored_parts):
            parts.append((sp, None, None, [va]))
    else:
        for per_seg in visits:
            counts = [dcs[s][np.asarray(v, np.int64)] if len(v) else np.zeros(0, np.int64)
                      for s, v in enumerate(per_seg)]
            states = _scored_states_fast(counts, limit)
            scored_in = [set() for _ in per_seg]
            for s, off in states:
                scored_in[s].add(int(per_seg[s][off]))
            slots = sorted(set().union(*scored_in)) if scored_in else []
            # term statistics from the segments where the term is scored (collector::score)
            all_dwt.extend(sum(int(dcs[s][t]) for s in range(len(per_seg)) if t in scored_in[s]) for t in slots)
            unscored_in, visited_in = [], []
            for s, v in enumerate(per_seg):
                va = np.asarray(v, np.uint32)
                keep = ~np.isin(va, np.fromiter(scored_in[s], np.uint32, len(scored_in[s]))) if scored_in[s] else \
                    np.ones(len(va), bool)
                unscored_in.append(va[keep])
                visited_in.append(va)
            parts.append((np.asarray(slots, np.uint32), scored_in, unscored_in, visited_in))
    dwt = np.asarray(all_dwt, np.float64)
    if isinstance(scorer, BM25):
        idf = np.log1p((float(dwf) - dwt + 0.5) / (dwt + 0.5)).astype(np.float32)
        probe = scorer.collect(dwf, 1, ttf)
        kind = scorer.term_scorer(probe)[0]
        nc, nl = probe.norm_const, probe.norm_length
        c0 = (f32(f32(boost) * f32(scorer.k + f32(1))) * idf).astype(np.float32)
    else:
        idf = np.log1p((dwf + 1.0) / (dwt + 1.0)).astype(np.float32)
        kind, nc, nl = scorer.term_scorer(TermStats(f32(1)))[0], f32(0), f32(0)
        c0 = (f32(boost) * idf).astype(np.float32)
    out, at = [], 0
    for slots, scored_in, unscored_in, visited_in in parts:
        n = len(slots)
        mine = c0[at:at + n]
        at += n
        slot_list = slots.tolist()
        if scored_in is None:                       # (one segment: every slot is scored there)
            scored_in = [set(slot_list)]
            present = np.ones((1, n), bool)
        else:
            present = np.array([[t in sc for t in slot_list] for sc in scored_in], bool).reshape(n_segs, n)
        out.append(PreparedExpansion(slot_list, scored_in, unscored_in,
                                     [(kind, x, nc, nl) for x in mine], visited_in, slots, present, mine,
                                     limit))
    return out


def expansion_arrays(segs, prepared, k):
    """The scored parts of a list of prepared expansions as ONE batch: an Or per filter whose term
    slots are absent (NO_TERM) in the segments where the term is unscored — a by_terms query with
    min_match 1 (OP_MULTITERM) where a filter prepared with a limit of up to 64 has more than
    IRS_HIP_MAX_TERMS slots.  Filters
    without any scored term get a one-slot query of an absent term (matches nothing)."""
    n_segs, nq = len(segs), len(prepared)
    n_slots = np.fromiter((max(1, len(p.scored)) for p in prepared), np.int64, nq)
    first = np.cumsum(n_slots) - n_slots
    n_entries = int(n_slots.sum())
    queries = np.zeros(nq, QUERY)
    queries["op"], queries["n_terms"], queries["first_term"] = OP_OR, n_slots, first
    taken = np.fromiter((p.limit is None or p.limit <= _lib.MAX_WIDE_TERMS for p in prepared), bool, nq)
    queries["op"][(n_slots > _lib.MAX_TERMS) & (n_slots <= _lib.MAX_WIDE_TERMS) & taken] = OP_MULTITERM
    queries["k"], queries["min_match"], queries["merge"] = int(k), 1, MERGE_SUM
    terms = np.zeros((n_segs, n_entries), TERM_SCORER)
    terms["term"] = NO_TERM                      # (also the one slot of a filter without scored terms)
    terms["kind"] = SCORE_BM1
    real = [q for q, p in enumerate(prepared) if p.scored]
    if real:
        where = np.concatenate([first[q] + np.arange(len(prepared[q].scored)) for q in real])
        slots = np.concatenate([prepared[q].slots for q in real])
        present = np.concatenate([prepared[q].present for q in real], axis=1)      # [seg][slot]
        kind, _, nc, nl = prepared[real[0]].scorers[0]
        terms["term"][:, where] = np.where(present, slots[None, :], np.uint32(NO_TERM))
        terms["kind"][:, where] = kind
        terms["c0"][:, where] = np.concatenate([prepared[q].c0 for q in real])[None, :]
        terms["norm_const"][:, where] = nc
        terms["norm_length"][:, where] = nl
    return QueryArrays(n_segs, queries, terms, k)


def execute_expansions(readers, prepared, k):
    """MultiTermQuery::execute for every (filter, segment) + the harness's top k per segment:
    hits HIT[n_segs][nq][k], counts, totals.  The scored disjunctions are one batch; a segment's
    total is the population of the union of ALL visited terms' postings (bit_union, like
    lazy_bitset_iterator + the scored iterators); where fewer than k docs score, the list is filled
    with the docs only unscored terms hold (score 0, ascending doc id: this path's tie order)."""
    n_segs, nq = len(readers), len(prepared)
    b = QueryBatch(readers, expansion_arrays(readers, prepared, k))
    hits, counts, totals = (x.copy() for x in b.run().results())
    b.close()
    hits = hits.reshape(n_segs, nq, k)
    counts = counts.reshape(n_segs, nq)
    totals = totals.reshape(n_segs, nq)
    for s, sr in enumerate(readers):
        n_words = (sr.num_docs + 64) // 64
        # the totals: the population of the union of ALL visited terms, for every filter that has
        # unscored terms here, in one call (only the counts cross PCIe)
        need = [q for q, p in enumerate(prepared) if p.n_unscored(s)]
        visited = [prepared[q].visited_in[s] for q in need]
        if need:
            totals[s, need] = sr.bit_union_counts(visited)
        for q, v in zip(need, visited):
            have = int(counts[s, q])
            if have >= k or int(totals[s, q]) <= have:
                continue
            # fewer than k docs score: the rest of the list are docs only unscored terms hold
            p = prepared[q]
            only, _ = sr.bit_union(v, n_words)
            if p.scored_in[s]:
                sc, _ = sr.bit_union(np.array(sorted(p.scored_in[s]), np.uint32), n_words)
                only = only & ~sc
            docs = np.nonzero(np.unpackbits(only.view(np.uint8), bitorder="little"))[0][:k - have]
            hits[s, q, have:have + len(docs)]["doc"] = docs
            hits[s, q, have:have + len(docs)]["score"] = 0.0
            counts[s, q] = have + len(docs)
    return hits, counts, totals
