"""Nested And / Or / Not trees of by_term — IRS_HIP_TREE_NODE: `a AND (b OR (c AND d))`,
`(a AND NOT b) OR c`, `+a +(b c d)~2` (And::prepare / Or::prepare prepare every child on its own,
boolean_filter.cpp:55-312; boolean_query.cpp:127-247, conjunction.hpp:436-490,
disjunction.hpp:1411-1467, exclusion.hpp), on k_tree_pilot / k_tree_score (csrc/tree.h).

Expected values come from the oracle as it stands: per leaf oracle.score_all over that one entry with
its boost product and index-global statistics, composed HERE by a recursive function over the filter
objects (compose), apart from the code under test: a node's match is a bool array, its score the
float64 sum over its matching positive children.  One body per case runs on the emulator (CPU tier)
and on the GPU.

The tie case asks for "one re-run": the batch counts re-runs per run, the case asserts exactly 1."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle
import parity
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, TFIDF, And, Not, Or, by_doc_set, by_phrase, by_term, by_terms
from test_or_clauses import (ABSENT, ALL, BORDER, N_HAND, T128, T129, TEMPTY, TILE, TONE, TTAIL, _present,
                             _score_entries, check, hand_lists)

f32 = np.float32
TREE, EXCL = _lib.TREE_NODE, _lib.EXCLUDE


# ------------------------------------------------------------- expectations --

def unwrap(flt):
    neg = False
    while isinstance(flt, Not):
        flt, neg = flt.filter, not neg
    return flt, neg


class Leaves:
    """oracle.score_all per (term, boost) of one segment and scorer, once."""

    def __init__(self, seg, scorer, all_segs=None):
        self.seg, self.scorer, self.all_segs, self.got = seg, scorer, all_segs or [seg], {}
        self.n1 = seg.num_docs + 1

    def __call__(self, term, boost):
        key = (int(term), float(boost))
        if key not in self.got:
            if _present(self.seg, term):
                sc, m = _score_entries(self.seg, [(term, f32(boost))], oracle.OP_OR, self.scorer, self.all_segs)
                self.got[key] = (m, sc.astype(np.float64))
            else:       # an absent term matches nothing
                self.got[key] = (np.zeros(self.n1, bool), np.zeros(self.n1, np.float64))
        return self.got[key]


def compose(flt, leaves, mult=f32(1)):
    """(matched bool[n1], score f64[n1]) of a filter tree, bottom up; boosts multiply from the top in
    float32."""
    if type(flt) is by_term:
        return leaves(flt.term, f32(mult * f32(flt.boost)))
    assert type(flt) in (And, Or), flt
    mult = f32(mult * f32(flt.boost))
    pos, neg = [], []
    for s in flt.subs:
        f, n = unwrap(s)
        (neg if n else pos).append(compose(f, leaves, f32(1) if n else mult))
    if type(flt) is And:
        assert pos, "an And needs a positive child"
        m = np.ones(leaves.n1, bool)
        for cm, _ in pos:
            m &= cm
        for cm, _ in neg:
            m &= ~cm
    else:
        assert not neg, "an Or has no negated children"
        m = sum(cm.astype(np.int64) for cm, _ in pos) >= max(1, int(flt.min_match))
    score = np.zeros(leaves.n1, np.float64)
    for cm, cs in pos:      # every matching positive child, not only min_match of them
        score += np.where(cm, cs, 0.0)
    return m, np.where(m, score, 0.0)


def expected(seg, flt, scorer, all_segs=None):
    """(score f64[num_docs + 1], matched bool[num_docs + 1]) — check()'s order."""
    m, s = compose(flt, Leaves(seg, scorer, all_segs))
    return s, m


def flat_score(flt, doc, leaves, mult=f32(1)):
    """The same tree for ONE doc, scalar by scalar: (matches, float64 sum of the per-leaf scores that
    count) — the second formulation case_parity holds compose against."""
    if type(flt) is by_term:
        m, s = leaves(flt.term, f32(mult * f32(flt.boost)))
        return bool(m[doc]), float(s[doc])
    mult = f32(mult * f32(flt.boost))
    n_pos = total = 0
    n_match, barred = 0, False
    for s in flt.subs:
        f, n = unwrap(s)
        cm, cs = flat_score(f, doc, leaves, f32(1) if n else mult)
        if n:
            barred = barred or cm
        else:
            n_pos += 1
            n_match += cm
            total += cs if cm else 0.0
    ok = (n_match == n_pos and not barred) if type(flt) is And else n_match >= max(1, int(flt.min_match))
    return ok, (total if ok else 0.0)


def n_leaves(flt):
    flt, _ = unwrap(flt)
    return 1 if type(flt) is by_term else sum(n_leaves(s) for s in flt.subs)


def depth(flt):
    flt, _ = unwrap(flt)
    return 0 if type(flt) is by_term else 1 + max(depth(s) for s in flt.subs)


# ------------------------------------------------- the encoding, written out --

def literal_entries(flt, scorer, stats):
    """The root's children in prefix order, one (term | None, kind, c0, nc, nl, phrase_offset) per
    entry, every And / Or below the root a node entry — the filter as it is written, nothing
    normalised; scorers as prepare() gives any by_term."""
    dwf = sum(s.docs_with_field for s in stats)
    ttf = sum(s.total_term_freq for s in stats)

    def one(t, boost):
        dwt = sum(int(st.docs_count[t]) for st in stats if 0 <= t < len(st.docs_count))
        return scorer.term_scorer(scorer.collect(dwf, dwt, ttf), boost)

    def children(node, mult):
        mult = f32(mult * f32(node.boost))
        out = []
        for s in node.subs:
            f, neg = unwrap(s)
            if type(f) is by_term:
                out.append((f.term, EXCL, 0.0, 0.0, 0.0, 0) if neg else
                           (f.term,) + tuple(one(f.term, f32(mult * f32(f.boost)))) + (0,))
            else:
                inner = children(f, f32(1) if neg else mult)
                mm = int(f.min_match) if f.op == _lib.OP_MINMATCH else 0
                out.append((None, TREE | f.op | (EXCL if neg else 0), 0.0, 0.0, 0.0, len(inner) | (mm << 16)))
                out += inner
        return out

    return children(flt, f32(1))


def literal_arrays(readers, filters, scorer, stats, k):
    """search.QueryArrays of tree queries, the entry arrays written directly."""
    ents = [literal_entries(f, scorer, stats) for f in filters]
    queries = np.zeros(len(filters), _lib.QUERY)
    terms = np.zeros((len(readers), max(1, sum(len(e) for e in ents))), _lib.TERM_SCORER)
    at = 0
    for q, (flt, es) in enumerate(zip(filters, ents)):
        mm = int(flt.min_match) if flt.op == _lib.OP_MINMATCH else 0
        queries[q] = (flt.op, len(es), at, int(k), mm, search.MERGE_SUM)
        for t, kind, c0, nc, nl, off in es:
            for s, sr in enumerate(readers):
                present = t is not None and 0 <= t < len(sr.metas)
                terms[s, at] = (t if present else _lib.NO_TERM, kind, c0, nc, nl, off)
            at += 1
    return search.QueryArrays(len(readers), queries, terms, k)


def _info(b):
    return {"reruns": b.reruns(), "tree": b.tree_units(), "clause": b.clause_units(), "wide": b.wide_units(),
            "path": b.path(), "paired": b.paired_tiles(), "streams": b.stream_counts()}


def _run(sr, filters, scorer, k, stats, cand_cap=0, path=None, literal=False, **flags):
    readers = sr if isinstance(sr, list) else [sr]
    if literal:
        prep = literal_arrays(readers, filters, scorer, stats, k)
    else:
        prep = search.prepare(filters, scorer, stats, boolean_trees=True, **flags)
    b = search.QueryBatch(readers if isinstance(sr, list) else sr, prep, k)
    if cand_cap:
        b.configure(cand_cap=cand_cap)
    if path is not None:
        b.set_path(path)
    h, c, t = (x.copy() for x in b.run().results())
    info = _info(b)
    b.close()
    return h, c, t, info


def T(t, boost=1.0):
    return by_term(t, boost)


def chain(terms, boosts=None):
    """A left-deep chain alternating And / Or: ((((t0 AND t1) OR t2) AND t3) OR t4) ... — the root is
    the last operator."""
    boosts = boosts or [1.0] * len(terms)
    node = And([T(terms[0], boosts[0]), T(terms[1], boosts[1])])
    for i in range(2, len(terms)):
        node = (Or if i % 2 == 0 else And)([node, T(terms[i], boosts[i])])
    return node


# -------------------------------------------------------------------- cases --

def case_abi(L):
    """IRS_HIP_TREE_NODE at batch create: every EINVAL / EUNSUPPORTED line of the header, the limits,
    the batch controls refused on such a batch (which afterwards still runs), tree_units(), and a
    query without node entries validated as before."""
    num_docs = 3000
    rng = np.random.default_rng(11)
    lists = []
    for t in range(24):
        docs = np.unique(rng.choice(num_docs, 400 + 25 * t, replace=False) + 1).astype(np.uint32)
        lists.append((docs, (1 + (docs + t) % 4).astype(np.uint32)))
    lists[20] = (lists[20][0], np.where(lists[20][0] % 50 == 0, 256, 1).astype(np.uint32))   # tf 256
    lists[21] = (lists[21][0], np.where(lists[21][0] % 50 == 0, 255, 1).astype(np.uint32))   # tf 255
    seg = synth.segment_from_lists(lists, num_docs, synth.LAYOUT_SIMD4)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    assert TREE == 0x8000
    OR, AND, MM = _lib.OP_OR, _lib.OP_AND, _lib.OP_MINMATCH

    def create(flt, mutate=None, k=10):
        arr = flt if isinstance(flt, search.QueryArrays) else literal_arrays([sr], [flt], BM25(), st, k)
        if mutate:
            mutate(arr)
        h = C.c_void_p()
        rc = L.irs_hip_batch_create(sr.handle, arr.queries.ctypes.data, len(arr.queries),
                                    arr.terms.ctypes.data, arr.terms.shape[1], C.byref(h))
        if rc == 0:
            L.irs_hip_batch_destroy(h)
        return rc

    def edit(**kw):
        def f(arr):
            for name, changes in kw.items():
                for j, v in changes.items():
                    arr.terms[0, j][name] = v
        return f

    def query(**kw):
        def f(arr):
            for name, v in kw.items():
                arr.queries[0][name] = v
        return f

    # a AND (b OR (c AND d)): entries a, NODE(OR, 4), b, NODE(AND, 2), c, d
    nest = And([T(0), Or([T(1), And([T(2), T(3)])])])
    arr = literal_arrays([sr], [nest], BM25(), st, 10)
    assert arr.terms[0, :6]["kind"].tolist() == [0, TREE | OR, 0, TREE | AND, 0, 0]
    assert arr.terms[0, :6]["phrase_offset"].tolist() == [0, 4, 0, 2, 0, 0]
    assert tuple(arr.queries[0])[:3] == (AND, 6, 0)
    assert create(nest) == _lib.OK
    # IRS_HIP_EINVAL
    assert create(nest, edit(phrase_offset={3: 3})) == _lib.EINVAL            # a span past its parent
    assert create(nest, edit(phrase_offset={1: 5})) == _lib.EINVAL            # ... past the query
    assert create(nest, edit(phrase_offset={3: 0})) == _lib.EINVAL            # a span of 0
    assert create(nest, edit(phrase_offset={1: 0})) == _lib.EINVAL
    assert create(nest, edit(kind={3: TREE | _lib.OP_PHRASE})) == _lib.EINVAL     # a node op outside the three
    assert create(nest, edit(kind={3: TREE | _lib.OP_MULTITERM})) == _lib.EINVAL
    assert create(nest, edit(kind={3: TREE | 5})) == _lib.EINVAL
    assert create(nest, edit(phrase_offset={1: 4 | (1 << 16)})) == _lib.EINVAL    # min_match on an OR node
    assert create(nest, edit(phrase_offset={3: 2 | (2 << 16)})) == _lib.EINVAL    # ... on an AND node
    assert create(nest, edit(kind={2: EXCL})) == _lib.EINVAL                  # a negated leaf under an Or node
    assert create(nest, edit(kind={3: TREE | AND | EXCL})) == _lib.EINVAL     # a negated subtree under an Or node
    assert create(nest, query(op=_lib.OP_PHRASE)) == _lib.EINVAL              # the flag under PHRASE
    assert create(nest, query(op=_lib.OP_MULTITERM, min_match=1)) == _lib.EINVAL
    assert create(nest, query(op=5)) == _lib.EINVAL
    for other in (_lib.CLAUSE_AND, _lib.PHRASE_ALT, _lib.PHRASE_REQUIRED, _lib.PHRASE_OPTIONAL,
                  _lib.PHRASE_NEXT, _lib.PHRASE_OR):
        assert create(nest, edit(kind={3: TREE | AND | other})) == _lib.EINVAL, other   # with another shape flag
        assert create(nest, edit(kind={4: other})) == _lib.EINVAL, other                # ... on a leaf of a tree
    assert create(nest, query(merge=3)) == _lib.EINVAL
    assert create(nest, query(k=0)) == _lib.EINVAL
    assert create(nest, edit(c0={4: -1.0})) == _lib.EINVAL
    assert create(nest, edit(kind={4: 7})) == _lib.EINVAL
    assert create(nest, edit(term={4: len(lists)})) == _lib.EINVAL
    assert create(nest, edit(kind={5: EXCL}, term={5: len(lists)})) == _lib.EINVAL    # a negated leaf's term, too
    # what is taken
    assert create(nest, edit(kind={5: EXCL})) == _lib.OK                      # c AND NOT d
    assert create(nest, edit(kind={1: TREE | OR | EXCL})) == _lib.OK          # a AND NOT (b OR (c AND d))
    assert create(nest, edit(kind={1: TREE | MM}, phrase_offset={1: 4 | (2 << 16)})) == _lib.OK
    assert create(nest, edit(kind={1: TREE | MM}, phrase_offset={1: 4 | (3 << 16)})) == _lib.OK   # above its children: empty
    assert create(nest, edit(term={4: _lib.NO_TERM})) == _lib.OK
    assert create(nest, edit(term={4: 21})) == _lib.OK                        # a frequency of 255 fits
    assert create(nest, edit(c0={4: 0.0})) == _lib.OK
    for mm in (1, 2, 3):
        assert create(nest, query(op=MM, min_match=mm)) == _lib.OK, mm
    assert create(nest, query(op=OR, min_match=7)) == _lib.OK                 # (ignored under OR / AND)
    # IRS_HIP_EUNSUPPORTED
    assert create(nest, query(merge=search.MERGE_MAX)) == _lib.EUNSUPPORTED
    assert create(nest, query(merge=search.MERGE_MIN)) == _lib.EUNSUPPORTED
    assert create(nest, edit(kind={4: EXCL, 5: EXCL})) == _lib.EUNSUPPORTED   # an And node of only Nots
    assert create(And([Not(T(0)), Not(Or([T(1), And([T(2), T(3)])]))])) == _lib.EUNSUPPORTED    # ... the root
    assert create(nest, lambda a: (query(op=OR)(a), edit(kind={0: EXCL})(a))) == _lib.EUNSUPPORTED   # a Not under the root Or
    assert create(nest, lambda a: (query(op=MM, min_match=1)(a), edit(kind={0: EXCL})(a))) == _lib.EUNSUPPORTED
    assert create(nest, edit(kind={1: TREE | MM})) == _lib.EUNSUPPORTED       # a MINMATCH node with min_match 0
    assert create(nest, query(op=MM, min_match=0)) == _lib.EUNSUPPORTED       # ... the root
    assert create(nest, edit(term={4: 20})) == _lib.EUNSUPPORTED              # a frequency of 256
    assert create(nest, edit(kind={5: EXCL}, term={5: 20})) == _lib.EUNSUPPORTED
    wide = And([T(0, 1.0), Or([T(1), And([T(2), T(3)]), T(4), T(5)])])
    five = edit(norm_const={j: 0.3 + 0.1 * j for j in (0, 2, 4, 5, 6)})
    four = edit(norm_const={j: 0.3 + 0.1 * j for j in (0, 2, 4)})
    assert create(wide, five) == _lib.EUNSUPPORTED and create(wide, four) == _lib.OK
    # the limits: 16 leaves, 15 node entries
    c16 = chain(list(range(16)))
    assert n_leaves(c16) == 16 and sum(1 for e in literal_entries(c16, BM25(), st) if e[0] is None) == 14
    assert create(c16) == _lib.OK
    fifteen = Or([chain(list(range(14))), Or([T(14)]), Or([T(15)])])
    ents = literal_entries(fifteen, BM25(), st)
    assert sum(1 for e in ents if e[0] is None) == 15 and n_leaves(fifteen) == 16
    assert create(fifteen) == _lib.OK                                         # 16 leaves with 15 nodes
    sixteen_nodes = Or([chain(list(range(14))), Or([T(14)]), Or([Or([T(15)])])])
    assert sum(1 for e in literal_entries(sixteen_nodes, BM25(), st) if e[0] is None) == 16
    assert create(sixteen_nodes) == _lib.EUNSUPPORTED                         # 16 node entries
    assert create(chain(list(range(17)))) == _lib.EUNSUPPORTED                # 17 leaves
    assert create(Or([And([T(0), T(1)])] + [T(t) for t in range(2, 17)])) == _lib.EUNSUPPORTED
    deep = T(0)
    for _ in range(40):
        deep = Or([deep])
    assert create(Or([deep, T(1)])) == _lib.EUNSUPPORTED                      # 40 nested node entries
    with pytest.raises(ValueError, match="at most 16 leaves"):
        search.prepare([chain(list(range(17)))], BM25(), st, boolean_trees=True)

    # a query without node entries is validated exactly as before
    flat = search.prepare([Or([T(0), T(1)])], BM25(), st)
    flat[0].excluded = [5]
    behind = search.QueryArrays.from_prepared([sr], flat, 10)
    assert create(behind) == _lib.OK
    behind.terms[0, 1], behind.terms[0, 2] = behind.terms[0, 2].copy(), behind.terms[0, 1].copy()
    assert create(behind) == _lib.EINVAL                                      # an included entry behind an excluded one
    many = search.prepare([Or([T(t) for t in range(16)])], BM25(), st)
    many[0].terms.append(16)
    many[0].scorers.append(many[0].scorers[0])
    assert create(search.QueryArrays.from_prepared([sr], many, 10)) == _lib.EINVAL    # 17 included entries
    unknown = search.QueryArrays.from_prepared([sr], search.prepare([Or([T(0), T(1)])], BM25(), st), 10)
    unknown.terms[0, 1]["kind"] = 0x4000 | 7
    assert create(unknown) == _lib.EINVAL

    # refused on a batch with such a query, which afterwards still runs correctly
    flts = [nest, Or([T(1), T(2)]), Or([And([T(3), Not(T(4))]), T(6)]), And([T(0), Or([T(1), T(2), T(5)], min_match=2)])]
    b = sr.batch(search.prepare(flts, BM25(), st, boolean_trees=True), 10)
    assert b.tree_units() == 3 and b.clause_units() == 0 and b.wide_units() == 0
    rows = np.full((1, num_docs // 64 + 1), ~np.uint64(0), np.uint64)
    with pytest.raises(_lib.IrsHipError) as e:
        b.set_doc_sets(rows, np.zeros(4, np.uint32))
    assert e.value.status == _lib.EUNSUPPORTED
    assert L.irs_hip_batch_set_comm(b.handle, None) == _lib.EUNSUPPORTED
    with pytest.raises(_lib.IrsHipError) as e:
        b.match_sets()
    assert e.value.status == _lib.EUNSUPPORTED
    b.set_wand(True)
    b.set_shared_threshold(True)
    h, c, t = b.run().results()
    with pytest.raises(_lib.IrsHipError) as e:
        b.match_sets()
    assert e.value.status == _lib.EUNSUPPORTED
    for q, flt in enumerate(flts):
        if q != 1:
            check(flt, 10, h[q], c[q], t[q], *expected(seg, flt, BM25()))
    parity.check_single_segment(seg, flts[1:2], BM25(), 10, h[1:2], c[1:2], t[1:2])
    b.close()
    # shapes the other routes take: no tree unit
    plain = sr.batch(search.prepare([flts[1], And([T(0), Or([T(1), T(2)])])], BM25(), st, boolean_trees=True), 10)
    plain.run()
    assert plain.tree_units() == 0
    plain.close()
    sr.close()


A, B_, C_, D_, E_ = 0, 1, 2, 3, 4      # the frequent hand terms


def hand_queries():
    """(filter, what it is about), by name.  Every one of them stays a tree under
    search.boolean_tree (no other route takes it)."""
    q = {}
    q["nest"] = And([T(A), Or([T(B_), And([T(C_), T(D_)])])])                # a AND (b OR (c AND d))
    q["andnot_or"] = Or([And([T(A), Not(T(B_))]), T(C_)])                    # (a AND NOT b) OR c
    q["not_and"] = And([T(A), Not(And([T(B_), T(C_)]))])                     # a AND NOT (b AND c)
    q["mm_group"] = And([T(A), Or([T(B_), T(C_), T(D_)], min_match=2)])      # +a +(b c d)~2
    q["mm_mixed"] = Or([And([T(A), T(B_)]), T(C_), Or([T(D_), T(E_)])], min_match=2)
    q["twice"] = Or([And([T(0), T(2)]), And([T(0), Or([T(4), T(6)])])])      # term 0 in two branches
    q["chain16"] = chain(list(range(16)))                                    # 16 leaves, 15 nodes with the root
    q["absent_and"] = Or([And([T(A), Or([T(B_), T(ABSENT)]), T(ABSENT)]), And([T(C_), T(D_)])])
    q["absent_or"] = And([T(A), Or([T(ABSENT), T(TEMPTY), And([T(C_), T(D_)])])])
    q["absent_not"] = Or([And([T(A), Not(T(ABSENT)), Not(T(TEMPTY))]), And([T(B_), T(C_)])])
    q["not_absent_tree"] = And([T(A), Not(And([T(B_), T(ABSENT)])), Or([T(C_), And([T(D_), T(E_)])])])
    q["all_empty"] = And([T(A), Or([T(ABSENT), And([T(TEMPTY), T(B_)])])])
    q["mm_above"] = And([T(A), Or([T(B_), T(ABSENT), T(TEMPTY)], min_match=2)])     # one present child of two needed
    q["mm_deep"] = Or([And([T(A), T(B_)]), And([T(C_), Not(T(D_))]), Or([T(5), T(6)], min_match=2), T(TTAIL)], min_match=2)
    q["zero"] = Or([And([T(A), Not(T(B_))], boost=0.0), And([T(TONE), Or([T(C_), T(D_)])])])   # matches, scores 0
    q["boosts"] = And([T(0, 0.25), Or([T(1, 4.0), And([T(2, 0.5), T(3, 2.0)], boost=0.25),
                                       Or([T(5, 0.5), T(7, 4.0)], min_match=2, boost=2.0)], boost=0.5),
                       Not(And([T(4), T(6)]))], boost=4.0)
    q["short"] = Or([And([T(T128), Or([T(0), T(1)])]), And([T(T129), Not(T(0))]),
                     And([T(TTAIL), Or([T(2), T(3)], min_match=2)]), And([T(TONE), Or([T(0), T(4)])])])
    return q


def case_lists(L, layout):
    lists = hand_lists()
    N = N_HAND
    norms = (np.arange(N, dtype=np.uint32) * 7 % 200 + 20).astype(np.uint8)
    seg = synth.segment_from_lists(lists, N, layout, norms=norms)
    seg.metas[TEMPTY]["docs_count"] = 0       # an ordinal whose range is empty here
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    named = hand_queries()
    names = list(named)
    filters = [named[n] for n in names]
    at = {n: i for i, n in enumerate(names)}
    has = [set(l[0].tolist()) for l in lists]
    has[TEMPTY] = set()
    assert all(d in has[0] and d in has[2] and d in has[4] for d in BORDER)     # held by several leaves
    assert all(ALL in s for t, s in enumerate(has) if t != TEMPTY)
    abc = has[A] & has[B_] & has[C_]
    assert len(abc) > 3
    for scorer in (TFIDF(True), BM25(), BM25(0.0, 0.0)):
        lv = Leaves(seg, scorer)
        exp = []
        for f in filters:
            m, s = compose(f, lv)
            exp.append((s, m))
        E = {n: exp[at[n]] for n in names}
        one = {t: lv(t, f32(1))[1] for t in (0, 2, 4, 6)}
        # what the lists say
        assert set(np.nonzero(E["nest"][1])[0].tolist()) == has[A] & (has[B_] | (has[C_] & has[D_]))
        assert set(np.nonzero(E["andnot_or"][1])[0].tolist()) == (has[A] - has[B_]) | has[C_]
        for d in sorted(abc)[:4]:         # a + b + c: a hit through c, scoring c only
            assert E["andnot_or"][1][d] and E["andnot_or"][0][d] == one[2][d] > 0
        assert set(np.nonzero(E["not_and"][1])[0].tolist()) == has[A] - (has[B_] & has[C_])
        two = {d for d in has[A] if (d in has[B_]) + (d in has[C_]) + (d in has[D_]) >= 2}
        assert set(np.nonzero(E["mm_group"][1])[0].tolist()) == two
        for d in BORDER:      # both branches match: term 0 scores twice
            assert E["twice"][1][d]
            want = 2 * one[0][d] + one[2][d] + one[4][d] + (one[6][d] if d in has[6] else 0.0)
            assert abs(E["twice"][0][d] - want) <= 1e-9 * max(want, 1e-30)
        assert E["chain16"][1][ALL] and n_leaves(named["chain16"]) == 16
        assert set(np.nonzero(E["absent_and"][1])[0].tolist()) == has[C_] & has[D_]
        assert set(np.nonzero(E["absent_or"][1])[0].tolist()) == has[A] & has[C_] & has[D_]
        assert set(np.nonzero(E["absent_not"][1])[0].tolist()) == has[A] | (has[B_] & has[C_])
        assert not E["all_empty"][1].any() and not E["mm_above"][1].any()
        zm = E["zero"][1]
        assert set(np.nonzero(zm)[0].tolist()) == (has[A] - has[B_]) | {ALL}
        assert (E["zero"][0][sorted((has[A] - has[B_]) - {ALL})] == 0).all()
        for k in (1, 10, 4096):
            h, c, t, info = _run(sr, filters, scorer, k, st)
            assert info["tree"] == len(filters) and info["clause"] == 0 and info["wide"] == 0, info
            for q, flt in enumerate(filters):
                check(flt, k, h[q], c[q], t[q], *exp[q])
            assert int(t[at["all_empty"]]) == 0 and int(t[at["mm_above"]]) == 0
            if k == 4096:
                got = dict(zip(h[at["andnot_or"], :int(c[at["andnot_or"]])]["doc"].tolist(),
                               h[at["andnot_or"], :int(c[at["andnot_or"]])]["score"].tolist()))
                for d in sorted(abc)[:4]:
                    if d in got:
                        assert abs(got[d] - one[2][d]) <= parity.REL_TOL * one[2][d]
        # the entry arrays written directly give what prepare() gives
        sub = [named[n] for n in ("nest", "andnot_or", "mm_group", "boosts", "chain16")]
        hl, cl, tl, il = _run(sr, sub, scorer, 100, st, literal=True)
        hp, cp, tp, ip = _run(sr, sub, scorer, 100, st)
        assert il["tree"] == ip["tree"] == len(sub)
        assert np.array_equal(tl, tp) and np.array_equal(cl, cp) and np.array_equal(hl["doc"], hp["doc"])
        assert np.allclose(hl["score"], hp["score"], rtol=parity.REL_TOL, atol=0)
    # every score ties (zero boosts): the candidates overflow a small buffer; exact re-run, tie order
    ties = [Or([And([T(0, 0.0), Not(T(1))]), T(4, 0.0)]),
            And([T(1), Or([T(3), And([T(5), T(7)])])], boost=0.0),
            Or([And([T(0), T(2)]), T(6), Or([T(3), T(8)], min_match=2)], min_match=2, boost=0.0)]
    h, c, t, info = _run(sr, ties, BM25(0.0, 0.0), 64, st, cand_cap=64)
    print("tie re-runs:", info["reruns"])
    assert info["reruns"] == 1 and info["tree"] == 3, info
    for q, flt in enumerate(ties):
        sc, m = expected(seg, flt, BM25(0.0, 0.0))
        assert m.sum() > 64
        check(flt, 64, h[q], c[q], t[q], sc, m)
        assert (h[q, :64]["score"] == 0).all()
        assert np.array_equal(h[q, :64]["doc"], np.nonzero(m)[0][:64])
    sr.close()
    # deleted docs: a border doc, the last doc, the doc that holds everything, a doc of a AND b AND c
    gone = [7, TILE, ALL, N, min(abc - {ALL})]
    seg2 = synth.segment_from_lists(lists, N, layout, norms=norms)
    seg2.doc_mask = np.array(sorted(gone), np.uint32)
    sr2 = search.SegmentReader.from_synth(seg2, L=L)
    st2 = [parity.segment_stats(seg2)]
    for scorer in (BM25(), TFIDF(True)):
        sub = [named[n] for n in ("nest", "andnot_or", "not_and", "mm_mixed", "twice", "chain16", "short")]
        h, c, t, _ = _run(sr2, sub, scorer, 100, st2)
        for q, flt in enumerate(sub):
            sc, m = expected(seg2, flt, scorer)
            assert not m[gone].any()
            check(flt, 100, h[q], c[q], t[q], sc, m)
        assert int(t[1]) == int(expected(seg, named["andnot_or"], scorer)[1].sum()) - \
            sum(1 for d in gone if d in (has[A] - has[B_]) | has[C_])
    sr2.close()


def case_routes(L, layout=synth.LAYOUT_SIMD4):
    """The same filter through the tree encoding (the entry arrays written directly) and through the
    route that already takes it: equal total hits and hit docs, scores within REL_TOL."""
    lists = hand_lists()
    N = N_HAND
    norms = (np.arange(N, dtype=np.uint32) * 7 % 200 + 20).astype(np.uint8)
    seg = synth.segment_from_lists(lists, N, layout, norms=norms)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    k = 4096
    pairs = [
        # Or([And..]) against and_clauses=True
        (Or([And([T(0), T(1, 2.0)]), And([T(2), T(3)], boost=2.0), T(TTAIL, 0.5)]), None, {"and_clauses": True}),
        (Or([And([T(4), T(5)]), And([T(4), T(6)]), T(T129)], min_match=2), None, {"and_clauses": True}),
        # And([Or..]) against the grouped And
        (And([T(1), Or([T(2), T(7, 0.5)]), Or([T(3), T(5), T(6)], boost=2.0)]), None, {}),
        # And([a, b, Not(c)]) against IRS_HIP_EXCLUDE: the tree form holds a AND b as a node
        (And([And([T(0), T(2, 4.0)]), Not(T(4))]), And([T(0), T(2, 4.0), Not(T(4))]), {}),
        (And([And([T(1), T(3)]), Not(T(0)), Not(T(TTAIL))]), And([T(1), T(3), Not(T(0)), Not(T(TTAIL))]), {}),
    ]
    for scorer in (BM25(), TFIDF(True)):
        for tree_form, route_form, flags in pairs:
            route_form = route_form or tree_form
            ht, ct, tt, it = _run(sr, [tree_form], scorer, k, st, literal=True)
            b = sr.batch(search.prepare([route_form], scorer, st, **flags), k)
            hr, cr, tr = (x.copy() for x in b.run().results())
            ir = _info(b)
            b.close()
            assert it["tree"] == 1 and ir["tree"] == 0, (it, ir)
            n = int(tt[0])
            assert 0 < n <= k, (tree_form, n)      # (every hit is returned: the doc sets compare exactly)
            assert n == int(tr[0]) and int(ct[0]) == int(cr[0]) == n
            dt, dr = np.argsort(ht[0, :n]["doc"]), np.argsort(hr[0, :n]["doc"])
            assert np.array_equal(ht[0, :n]["doc"][dt], hr[0, :n]["doc"][dr])
            a, r = ht[0, :n]["score"][dt].astype(np.float64), hr[0, :n]["score"][dr].astype(np.float64)
            assert (np.abs(a - r) <= parity.REL_TOL * np.maximum(np.abs(r), 1e-30)).all(), tree_form
            check(tree_form, k, ht[0], ct[0], tt[0], *expected(seg, tree_form, scorer))
    sr.close()


PICK = [0.25, 0.5, 1.0, 1.0, 2.0, 4.0]


def refused(flt):
    """Does prepare() WITHOUT the keyword refuse the filter — as it did before there were trees: only
    such a filter reaches the tree route."""
    st = [search.SegmentStats(1000, 100_000, np.full(64, 10, np.int64))]
    try:
        search.prepare([flt], BM25(), st)
    except ValueError:
        return True
    return False


def nested(flt):
    """Does the filter keep a second level once children of their parent's own operator are merged
    into it (And into And, plain Or into plain Or) — or is it one flat query written with brackets."""
    for s in flt.subs:
        f, neg = unwrap(s)
        if type(f) is by_term:
            continue
        same = not neg and type(f) is type(flt) and (type(f) is And or (f.min_match <= 1 and flt.min_match <= 1))
        if not same or nested(f):
            return True
    return False


def random_tree(rng, frequent=10, rare=(12, 40), max_depth=4):
    """One tree of 3..16 leaves, depth up to `max_depth`: And nodes of 2..3 children (plus, often, a Not
    of a rarer term or of a small And), Or nodes of 2..4, min-match Ors of 3..4 with min_match 2;
    positive leaves from the `frequent` most frequent ranks, so that conjunctions of them have docs.
    Only trees that prepare() refuses without the keyword and that stay nested: the others keep their
    routes."""
    def leaf():
        return by_term(int(rng.integers(frequent)), float(rng.choice(PICK)))

    def gen(d, top):
        if d == 0 or (not top and rng.random() < 0.4):
            return leaf()
        kind = rng.choice(["and", "or", "mm"], p=[0.4, 0.4, 0.2])
        boost = float(rng.choice(PICK))
        if kind == "and":
            subs = [gen(d - 1, False) for _ in range(int(rng.integers(2, 4)))]
            r = rng.random()
            if r < 0.35:
                subs.append(Not(by_term(int(rng.integers(*rare)))))
            elif r < 0.5:
                subs.append(Not(And([leaf(), by_term(int(rng.integers(*rare)))])))
            return And(subs, boost=boost)
        if kind == "or":
            return Or([gen(d - 1, False) for _ in range(int(rng.integers(2, 5)))], boost=boost)
        return Or([gen(d - 1, False) for _ in range(int(rng.integers(3, 5)))], min_match=2, boost=boost)

    while True:
        t = gen(int(rng.integers(2, max_depth + 1)), True)
        if 3 <= n_leaves(t) <= 16 and depth(t) >= 2 and refused(t) and nested(t):
            return t


def random_trees(n, seed):
    rng = np.random.default_rng(seed)
    return [random_tree(rng) for _ in range(n)]


PARITY_SEED = 5      # chosen on the CPU, by the oracle alone, so that both preconditions hold (below)


def parity_preconditions(seg, filters, scorer, k):
    """Every tree matches at least one doc and at least half of them more than k; for the best 2k docs
    of every tree the composed sums are within REL_TOL / 4 of the scalar float64 formulation."""
    exp = []
    for f in filters:
        lv = Leaves(seg, scorer)
        m, s = compose(f, lv)
        assert m.any(), ("a tree without matches", f)
        top = np.argsort(-s, kind="stable")[:2 * k]
        for d in top[m[top]]:
            fm, fs = flat_score(f, int(d), lv)
            assert fm and abs(fs - s[d]) <= parity.REL_TOL / 4 * max(fs, 1e-30), ("precondition", f, int(d))
        exp.append((s, m))
    assert sum(int(m.sum()) > k for _, m in exp) * 2 >= len(filters), "at least half match more than k"
    return exp


def case_parity(L, num_docs, max_rank, layout, n_queries=24, seed=PARITY_SEED):
    seg = synth.build_segment(num_docs, max_rank, layout=layout)
    seg.doc_mask = np.arange(9, num_docs, 101, dtype=np.uint32)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    filters = random_trees(n_queries, seed)
    assert all(3 <= n_leaves(f) <= 16 and 2 <= depth(f) <= 4 for f in filters)
    assert any("Not" in repr(f) for f in filters) and any("min_match=2" in repr(f) for f in filters)
    for scorer in (BM25(), TFIDF(True)):
        exp = parity_preconditions(seg, filters, scorer, 128)
        for k in (64, 128):
            h, c, t, info = _run(sr, filters, scorer, k, st)
            assert info["tree"] == n_queries, info
            for q, flt in enumerate(filters):
                check(flt, k, h[q], c[q], t[q], *exp[q])
    sr.close()


def case_mixed(L, num_docs, max_rank, layout):
    """Tree queries interleaved with ordinary ones: the ordinary ones are bit for bit what a batch
    without the tree queries gives, on the same path; the tree ones equal a batch of their own."""
    seg = synth.build_segment(num_docs, max_rank, layout=layout)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    rng = np.random.default_rng(17)
    tr = random_trees(4, 23)
    ordinary = [Or([by_term(int(t)) for t in rng.choice(max_rank, 8, replace=False)]) for _ in range(3)]
    ordinary += [And([by_term(int(t)) for t in rng.choice(16, 3, replace=False)]) for _ in range(2)]
    ordinary += [Or([by_term(int(t)) for t in rng.choice(24, 6, replace=False)], min_match=2)]
    ordinary += [And([by_term(1), Or([by_term(2), by_term(7)])])]        # a grouped And
    ordinary += [by_terms(list(range(3, 25)), 2)]
    ordinary += [Or([And([by_term(0), by_term(1)]), by_term(5)])]        # an Or of clauses
    mixed = [tr[0], ordinary[0], ordinary[3], tr[1], ordinary[1], ordinary[5], ordinary[6], tr[2],
             ordinary[2], ordinary[4], ordinary[7], ordinary[8], tr[3]]
    at_t = [mixed.index(f) for f in tr]
    at_o = [mixed.index(f) for f in ordinary]
    for scorer in (BM25(), TFIDF(True)):
        for path in (None, _lib.PATH_JOINED, _lib.PATH_ITEMS):
            hm, cm, tm, im = _run(sr, mixed, scorer, 50, st, path=path, and_clauses=True)
            ho, co, to, io = _run(sr, ordinary, scorer, 50, st, path=path, and_clauses=True)
            ht, ct, tt, it = _run(sr, tr, scorer, 50, st, path=path, and_clauses=True)
            assert im["tree"] == 4 and io["tree"] == 0 and it["tree"] == 4
            assert im["clause"] == 1 and io["clause"] == 1 and it["clause"] == 0
            assert im["wide"] == 1 and io["wide"] == 1 and it["wide"] == 0
            assert im["path"] == io["path"] and im["paired"] == io["paired"], (path, im, io)
            assert np.array_equal(hm[at_o], ho) and np.array_equal(cm[at_o], co) and np.array_equal(tm[at_o], to)
            assert np.array_equal(hm[at_t], ht) and np.array_equal(cm[at_t], ct) and np.array_equal(tm[at_t], tt)
            for q in at_t:
                check(mixed[q], 50, hm[q], cm[q], tm[q], *expected(seg, mixed[q], scorer))
        parity.check_single_segment(seg, ordinary[:6], scorer, 50, ho[:6], co[:6], to[:6])
    sr.close()


def case_multi(L, sizes, max_rank=96, k=50):
    """create_multi: a leaf absent from one segment, statistics over all segments, units indexed
    segment * n_queries + query, the merged top k against the composed expectation."""
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    segs = [synth.build_segment(int(n), max_rank, first_doc=int(f)) for n, f in zip(sizes, first)]
    segs[1].metas[5]["docs_count"] = 0
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    stats = [parity.segment_stats(s) for s in segs]
    filters = random_trees(4, 41)
    filters.append(And([T(1), Or([T(5), And([T(2), T(3)], boost=2.0)])]))       # segment 1: the Or drops its first child
    filters.append(Or([And([T(5, 2.0), Or([T(0), T(1)])]), And([T(5), T(4), Not(T(2))])]))   # segment 1: nothing
    filters.append(Or([And([T(0), Not(T(5))]), And([T(1), T(2)])]))             # segment 1: the Not has no effect
    filters.append(And([T(0), Or([T(1), T(5), T(2)], min_match=2)]))
    for scorer in (BM25(), TFIDF(True)):
        prep = search.prepare(filters, scorer, stats, boolean_trees=True)
        dwf = sum(s.docs_with_field for s in segs)
        ttf = sum(s.total_term_freq for s in segs)
        dwt5 = sum(int(s.metas[5]["docs_count"]) for s in segs)
        assert prep[4].terms[2] == 5 and prep[4].scorers[2] == scorer.term_scorer(scorer.collect(dwf, dwt5, ttf), 1.0)
        b = search.QueryBatch(readers, prep, k)
        assert b.tree_units() == len(filters) * len(segs)
        b.set_shared_threshold(True)       # (leaves every tree unit a threshold of its own)
        h, c, t = b.run().results()
        assert h.shape[:2] == (len(segs), len(filters))
        per = [[expected(s, flt, scorer, segs) for flt in filters] for s in segs]
        for i, s in enumerate(segs):
            for q, flt in enumerate(filters):
                check(flt, k, h[i, q], c[i, q], t[i, q], *per[i][q])
        assert int(t[1, 5]) == 0 and int(t[0, 5]) > 0
        merged = search.merge_topk_host([(h[i], c[i]) for i in range(len(segs))], k)
        for q, flt in enumerate(filters):
            allsc = np.concatenate([per[i][q][0][per[i][q][1]] for i in range(len(segs))])
            ref = np.sort(allsc)[::-1][:k]
            assert int(t[:, q].sum()) == allsc.size, q
            got = np.array([r[0] for r in merged[q]])
            assert len(got) == len(ref), (q, len(got), len(ref))
            assert np.allclose(got, ref, rtol=parity.REL_TOL, atol=0), q
        b.close()
    for r in readers:
        r.close()


def case_streams(L, num_docs, max_rank):
    """The tree units' leaves are streams of the batch's one set: shared with an ordinary query,
    between branches and with a negated leaf, served by the device's stream cache, the same results
    without it."""
    seg = synth.build_segment(num_docs, max_rank)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    a, b_, c_, d = 2, 3, 4, 5
    tree = And([T(a), Or([T(b_), And([T(a, 2.0), T(c_)])]), Not(And([T(d), T(b_)]))])
    plain = Or([T(a), T(b_), T(d)])
    flts = [tree, plain]
    search.set_stream_cache(0, L=L)
    try:
        h0, c0, t0, i0 = _run(sr, flts, BM25(), 20, st, path=_lib.PATH_JOINED)
        assert i0["path"] == _lib.PATH_JOINED and i0["tree"] == 1
        assert i0["streams"] == (4, 4), i0       # a, b, c, d: the union, all decoded by the run
        ht, ct, tt, it = _run(sr, [tree], BM25(), 20, st)
        assert it["streams"] == (4, 4), it
        search.set_stream_cache(64 << 20, L=L)
        h1, c1, t1, i1 = _run(sr, flts, BM25(), 20, st, path=_lib.PATH_JOINED)
        h2, c2, t2, i2 = _run(sr, flts, BM25(), 20, st, path=_lib.PATH_JOINED)
        assert i1["streams"] == (4, 4) and i2["streams"] == (4, 0), (i1, i2)
        for h, c, t in ((h1, c1, t1), (h2, c2, t2)):
            assert np.array_equal(h, h0) and np.array_equal(c, c0) and np.array_equal(t, t0)
        assert np.array_equal(ht[0], h0[0])
        check(tree, 20, h0[0], c0[0], t0[0], *expected(seg, tree, BM25()))
    finally:
        search.set_stream_cache(0, L=L)
        L.irs_hip_device_trim(0)
    sr.close()


CHUNK_TILES = 9                  # launch_tree_score: 17 tiles in cpq = 2 chunks of ceil(17 / 2)
N_CHUNKS = 16 * TILE + 5         # 17 tiles, the last one nearly empty
N_SHORT = TILE + 5               # 2 tiles: the second workgroup of such a unit has no tile
HOT_TILES = (3, 12)              # one tile of chunk 0, one of chunk 1
STAGE = 512                      # kWideCands: candidate staging slots per chunk


def _chunk_lists(num_docs, seed):
    """Terms 0 .. 5 of a segment whose matches are concentrated: a core of docs that hold terms 0 and 2
    (tf 1 .. 30) — 1000 in each tile of HOT_TILES where the segment has them, 150 anywhere — of which
    every second holds term 1, two of three term 3, two of five term 5 and every seventh term 4 (the
    negated leaf); 60 docs in tile 0 that hold terms 0, 1, 2, 3, 5 at tf 200 .. 255 (the best of every
    query: a pilot that counted tile 0 twice would take their bin); the docs at every CHUNK_TILES
    border, the last doc of the first tile, the first of the second and the segment's last doc hold
    0, 1, 2, 3, 5; beside the core every term holds 300 docs of its own."""
    rng = np.random.default_rng(seed)
    n_tiles = (num_docs + TILE - 1) // TILE
    free = np.ones(num_docs + 1, bool)
    free[0] = False
    fixed = {TILE, TILE + 1, num_docs}
    for t in range(CHUNK_TILES, n_tiles, CHUNK_TILES):
        fixed |= {t * TILE, t * TILE + 1}             # the last doc of tile t - 1, the first of tile t
    fixed = np.array(sorted(fixed), np.int64)
    free[fixed] = False

    def take(lo, hi, n):
        ids = lo + np.nonzero(free[lo:hi])[0]
        d = np.sort(rng.choice(ids, n, replace=False))
        free[d] = False
        return d
    top = take(1, TILE, 60)
    core = [take(1 + t * TILE, 1 + (t + 1) * TILE, 1000) for t in HOT_TILES if (t + 1) * TILE <= num_docs]
    core = np.sort(np.concatenate(core + [take(1, num_docs + 1, 150)]))
    i = np.arange(core.size)
    member = {0: core, 1: core[i % 2 == 0], 2: core, 3: core[i % 3 != 0], 4: core[i % 7 == 0], 5: core[i % 5 < 2]}
    lists = []
    for t in range(6):
        own = take(1, num_docs + 1, 300)
        docs = [member[t], own] + ([fixed, top] if t != 4 else [])
        tfs = [rng.integers(1, 31, member[t].size), rng.integers(1, 6, own.size)] + \
            ([rng.integers(1, 31, fixed.size), rng.integers(200, 256, top.size)] if t != 4 else [])
        d, f = np.concatenate(docs), np.concatenate(tfs)
        order = np.argsort(d)
        lists.append((d[order].astype(np.uint32), f[order].astype(np.uint32)))
    return lists, fixed, top


def case_chunks(L, layout):
    """Units of more than kWideChunkTiles = 16 tiles: one segment of 16 * 12288 + 5 docs — 17 tiles,
    cpq = 2 workgroups per unit, chunk_tiles = 9 — and in the same batch one of 12288 + 5 docs, 2 tiles,
    whose second workgroup leaves at `tile0 >= n_tiles`.  Two filters with a Not leaf and a nested And
    on _chunk_lists: more than 600 hits in tile 3 and in tile 12 (a chunk stages more than kWideCands =
    512), hits at the last doc of tile 8 and the first of tile 9 (the chunk border) and at the segment's
    last doc.  Without norms under TFIDF(False) and BM25(1.2, 0), once BM25() with norms.  Per scorer:
    k = 4096 (every hit returned: doc sets compare exactly) and k = 100 at the default stride;
    configure(0, 1, 0): 17 sampled tiles, the pilot's second round of kWideChunkTiles; the same with a
    candidate buffer of 128 slots under zero boosts (every hit ties: all are candidates, overflow, one
    re-run, the smallest doc ids)."""
    sizes = (N_CHUNKS, N_SHORT)
    built = [_chunk_lists(n, 61 + i) for i, n in enumerate(sizes)]
    filters = [And([T(0), Or([T(1), And([T(2), T(3)])]), Not(T(4))]),
               Or([And([T(0, 0.5), Not(T(4))]), And([T(2), Or([T(1, 2.0), And([T(3), T(5)])])])])]
    zero = [And(f.subs, boost=0.0) if type(f) is And else Or(f.subs, boost=0.0) for f in filters]
    assert all(refused(f) for f in filters)
    for scorer, with_norms in ((TFIDF(False), False), (BM25(1.2, 0.0), False), (BM25(), True)):
        segs = []
        for (lists, _, _), n in zip(built, sizes):
            norms = (np.arange(n, dtype=np.uint32) * 7 % 200 + 20).astype(np.uint8) if with_norms else False
            segs.append(synth.segment_from_lists(lists, n, layout, norms=norms))
        readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
        stats = [parity.segment_stats(s) for s in segs]
        per = [[expected(s, f, scorer, segs) for f in filters] for s in segs]
        per0 = [[expected(s, f, scorer, segs) for f in zero] for s in segs]
        for q in range(len(filters)):      # what the lists must give, by the oracle alone
            sc, m = per[0][q]
            tile_hits = [int(m[1 + t * TILE:1 + (t + 1) * TILE].sum()) for t in range(17)]
            assert all(tile_hits[t] >= 600 for t in HOT_TILES), tile_hits
            assert sum(tile_hits[:CHUNK_TILES]) > STAGE and sum(tile_hits[CHUNK_TILES:]) > STAGE, tile_hits
            assert m[CHUNK_TILES * TILE] and m[CHUNK_TILES * TILE + 1] and m[N_CHUNKS] and tile_hits[16] >= 1
            assert m[built[0][1]].all() and m[built[0][2]].all()
            assert 100 < int(m.sum()) <= 4096 and 100 < int(per[1][q][1].sum()) <= 4096
            assert per[1][q][1][N_SHORT] and per[1][q][1][TILE] and per[1][q][1][TILE + 1]
            best = np.argsort(-sc, kind="stable")[:60]
            assert set(best.tolist()) == set(built[0][2].tolist()), "the 60 docs of tile 0 are the best"
        for flts, exp, k, stride, cap, reruns in ((filters, per, 4096, 0, 0, 0), (filters, per, 100, 0, 0, 0),
                                                  (filters, per, 4096, 1, 0, 0), (filters, per, 100, 1, 0, 0),
                                                  (zero, per0, 100, 1, 128, 1)):
            prep = search.prepare(flts, scorer, stats, boolean_trees=True)
            b = search.QueryBatch(readers, prep, k)
            if stride or cap:
                b.configure(0, stride, cap)
            assert b.tree_units() == len(flts) * len(segs)
            h, c, t = b.run().results()
            assert b.reruns() == reruns, (k, stride, cap, b.reruns())
            for s in range(len(segs)):
                for q, flt in enumerate(flts):
                    check(flt, k, h[s, q], c[s, q], t[s, q], *exp[s][q])
                    n = int(c[s, q])
                    if cap:     # every score ties: doc id order
                        assert n == k and (h[s, q, :n]["score"] == 0).all()
                        assert np.array_equal(h[s, q, :n]["doc"], np.nonzero(exp[s][q][1])[0][:k])
                    elif k == 4096:
                        assert n == int(exp[s][q][1].sum())
                        assert np.array_equal(np.sort(h[s, q, :n]["doc"]), np.nonzero(exp[s][q][1])[0])
            b.close()
        for r in readers:
            r.close()


def case_min_scores(L, layout):
    """irs::score::Min (irs_hip_batch_set_min_scores) on a tree batch: k_tree_pilot's min_bin,
    k_tree_score's `v < thr` pre-filter on sums that still carry their scoring mask, k_select's exact
    cut.  The hand lists (three tiles), k = 50, with and without set_wand(True).  The unrestricted run
    is h0 (checked against the composed expectation); a threshold at the k-th score returns h0; at the
    10th score exactly the prefix of h0 at or above it, ties included; at the float just above it the
    correspondingly shorter prefix; 1e30 returns nothing; None returns h0 again.  Totals never change,
    nothing re-runs.  chain16's best doc (ALL) scores through all 16 leaves.  With k candidate slots a
    threshold nothing reaches stages nothing (no re-run), where the same batch without a threshold
    overflows: the pilot's min_bin bounds the candidates."""
    lists = hand_lists()
    N = N_HAND
    norms = (np.arange(N, dtype=np.uint32) * 7 % 200 + 20).astype(np.uint8)
    seg = synth.segment_from_lists(lists, N, layout, norms=norms)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    named = hand_queries()
    names = ["nest", "andnot_or", "not_and", "mm_mixed", "twice", "chain16", "boosts", "short"]
    filters = [named[n] for n in names]
    k = 50
    for scorer in (BM25(), TFIDF(True)):
        exp = [expected(seg, f, scorer) for f in filters]
        assert all(int(m.sum()) > k for _, m in exp[:-1])
        c16 = names.index("chain16")
        assert n_leaves(filters[c16]) == 16 and int(np.argmax(exp[c16][0])) == ALL
        for wand in (False, True):
            b = sr.batch(search.prepare(filters, scorer, st, boolean_trees=True), k)
            assert b.tree_units() == len(filters)
            b.set_wand(wand)
            h0, c0, t0 = (x.copy() for x in b.run().results())
            for q, flt in enumerate(filters):
                check(flt, k, h0[q], c0[q], t0[q], *exp[q])
            assert int(h0[c16, 0]["doc"]) == ALL
            assert (c0 >= 10).all() and (h0[:, 9]["score"] > 0).all()

            def run(ms):
                b.set_min_scores(None if ms is None else np.asarray(ms, f32))
                h, c, t = (x.copy() for x in b.run().results())
                assert b.reruns() == 0
                assert np.array_equal(t, t0), "a caller's threshold changes no total"
                return h, c

            def prefix(ms):
                return np.array([int((h0[q, :int(c0[q])]["score"] >= ms[q]).sum()) for q in range(len(filters))])

            def same_prefix(h, c, n, what):
                assert np.array_equal(c, n), (what, c, n)
                for q in range(len(filters)):
                    assert np.array_equal(h[q, :n[q]], h0[q, :n[q]]), (what, names[q])
            kth = np.array([h0[q, int(c0[q]) - 1]["score"] for q in range(len(filters))], f32)
            tenth = h0[:, 9]["score"].astype(f32)
            above = np.nextafter(tenth, f32(np.inf))
            same_prefix(*run(kth), c0, "the k-th score")
            n10, n_above = prefix(tenth), prefix(above)
            assert (n10 >= 10).all() and (n_above < 10).all() and (n10 < c0).any() and (n_above > 0).any()
            same_prefix(*run(tenth), n10, "the 10th score")
            same_prefix(*run(above), n_above, "above the 10th score")
            h, c = run(np.full(len(filters), 1e30, f32))
            assert (c == 0).all()
            same_prefix(*run(None), c0, "None")
            b.close()
            # k_tree_pilot's min_bin is what keeps the candidates few: with k candidate slots (the
            # fewest configure takes) the run under a threshold nothing reaches stages nothing, and
            # the same batch without a threshold — the pilot's own bin admits k docs and their
            # bin-mates — overflows and runs again
            b = sr.batch(search.prepare(filters, scorer, st, boolean_trees=True), k).configure(0, 0, k)
            b.set_wand(wand)
            b.set_min_scores(np.full(len(filters), 1e30, f32))
            h, c, t = (x.copy() for x in b.run().results())
            assert b.reruns() == 0, "the caller's bin bounds the candidates"
            assert np.array_equal(t, t0) and (c == 0).all()
            b.set_min_scores(None)
            h, c, t = (x.copy() for x in b.run().results())
            assert b.reruns() == 1, "without it the k slots overflow: the case above bites"
            assert np.array_equal(t, t0)
            same_prefix(h, c, c0, "None, k candidate slots")
            b.close()
    sr.close()


# --------------------------------------------------------------- host only --

def test_prepare_boolean_trees():
    st = [search.SegmentStats(1000, 100_000, np.arange(64, dtype=np.int64) * 3 + 20),
          search.SegmentStats(500, 40_000, np.arange(32, dtype=np.int64) * 2 + 1)]
    sc = BM25()
    segs = [type("S", (), {"metas": np.zeros(n)})() for n in (64, 32)]
    OR, AND, MM = _lib.OP_OR, _lib.OP_AND, _lib.OP_MINMATCH

    def prep(flt, **kw):
        return search.prepare([flt], sc, st, boolean_trees=True, **kw)[0]

    # normalisation: single children collapse with their boost, And into And, SUM Or (min_match <= 1)
    # into such an Or, Not(Not(f)) is f; boosts multiply from the top in float32
    flt = And([by_term(7, 0.5),
               And([by_term(9, 2.0), Not(Not(by_term(11)))], boost=4.0),
               Or([by_term(3), Or([by_term(4, 0.3), And([by_term(40)], boost=3.0)], boost=0.5),
                   And([by_term(5), Not(by_term(6)), Or([by_term(8)])])], boost=0.7),
               Not(Or([And([by_term(12), by_term(13)], boost=9.0), by_term(14)]))], boost=1.5)
    top = f32(1.5)
    o = f32(top * f32(0.7))
    oo = f32(o * f32(0.5))
    want = ("node", AND, 0, [
        (False, ("leaf", 7, f32(top * f32(0.5)))),
        (False, ("leaf", 9, f32(f32(top * f32(4.0)) * f32(2.0)))),
        (False, ("leaf", 11, f32(f32(top * f32(4.0)) * f32(1.0)))),
        (False, ("node", OR, 0, [
            (False, ("leaf", 3, f32(o * f32(1.0)))),
            (False, ("leaf", 4, f32(oo * f32(0.3)))),
            (False, ("leaf", 40, f32(f32(oo * f32(3.0)) * f32(1.0)))),
            (False, ("node", AND, 0, [(False, ("leaf", 5, o)), (True, ("leaf", 6, f32(1))),
                                      (False, ("leaf", 8, o))]))])),
        (True, ("node", OR, 0, [(False, ("node", AND, 0, [(False, ("leaf", 12, f32(9.0))), (False, ("leaf", 13, f32(9.0)))])),
                                (False, ("leaf", 14, f32(1)))]))])
    got = search.boolean_tree(flt)
    assert got == want
    assert all(type(x[2]) is np.float32 for x in (got[3][0][1], got[3][1][1], got[3][3][1][3][1][1]))
    p = prep(flt)
    assert p.op == AND and p.min_match == 0 and p.merge == search.MERGE_SUM and p.excluded == []
    assert p.terms == [7, 9, 11, None, 3, 4, 40, None, 5, 6, 8, None, None, 12, 13, 14]
    assert p.tree == [None, None, None, (OR, 7, 0, False), None, None, None, (AND, 3, 0, False), None, "not", None,
                      (OR, 4, 0, True), (AND, 2, 0, False), None, None, None]
    # statistics per leaf, as everywhere: the field's over all segments, the term's where it exists
    assert p.scorers[6] == sc.term_scorer(sc.collect(1500, int(st[0].docs_count[40]), 140_000), want[3][3][1][3][2][1][2])
    assert p.scorers[0] == sc.term_scorer(sc.collect(1500, int(st[0].docs_count[7] + st[1].docs_count[7]), 140_000), want[3][0][1][2])
    arr = search.QueryArrays.from_prepared(segs, [p], 10)
    assert tuple(arr.queries[0]) == (AND, 16, 0, 10, 0, search.MERGE_SUM)
    kinds = arr.terms[0, :16]["kind"].tolist()
    B = _lib.SCORE_BM25
    assert kinds == [B, B, B, TREE | OR, B, B, B, TREE | AND, B, EXCL, B, TREE | OR | EXCL, TREE | AND, B, B, B]
    assert arr.terms[0, :16]["phrase_offset"].tolist() == [0, 0, 0, 7, 0, 0, 0, 3, 0, 0, 0, 4, 2, 0, 0, 0]
    assert arr.terms[1, :16]["term"].tolist() == [7, 9, 11, _lib.NO_TERM, 3, 4, _lib.NO_TERM, _lib.NO_TERM, 5, 6, 8,
                                                  _lib.NO_TERM, _lib.NO_TERM, 12, 13, 14]
    assert (arr.terms[0, [3, 7, 9, 11, 12]]["c0"] == 0).all()
    # min-match nodes keep their count and are not flattened; the root's op is its own
    mm = prep(Or([And([by_term(1), Or([by_term(2), by_term(3)], min_match=2)]), by_term(4), Or([by_term(5), by_term(6)])],
                 min_match=2))
    assert mm.op == MM and mm.min_match == 2
    assert mm.tree == [(AND, 4, 0, False), None, (MM, 2, 2, False), None, None, None, (OR, 2, 0, False), None, None]
    a_mm = search.QueryArrays.from_prepared(segs, [mm], 10)
    assert a_mm.terms[0, 2]["phrase_offset"] == 2 | (2 << 16) and a_mm.terms[0, 2]["kind"] == TREE | MM
    assert search.boolean_tree(Or([by_term(1, 2.0)], boost=3.0)) == ("leaf", 1, f32(6.0))
    one_mm = search.boolean_tree(And([by_term(0), Or([by_term(1)], min_match=2)]))      # (never matches: kept)
    assert one_mm[3][1] == (False, ("node", MM, 2, [(False, ("leaf", 1, f32(1)))]))
    # a tree that normalises to one level is the flat query it is
    lvl = prep(And([And([by_term(1), by_term(2, 2.0)], boost=0.5), Not(by_term(3)), And([by_term(4)])]))
    assert lvl.tree is None and lvl.op == AND and lvl.terms == [1, 2, 4] and lvl.excluded == [3]
    assert lvl.scorers[1] == sc.term_scorer(sc.collect(1500, int(st[0].docs_count[2] + st[1].docs_count[2]), 140_000), f32(1.0))
    # routes kept byte for byte: what another route takes under the flags given keeps its bytes
    ab = And([by_term(1), by_term(2)])
    kept = [(Or([by_term(1), by_term(2, 2.0), by_term(3)], boost=0.5), {}),
            (And([by_term(1), Or([by_term(2), by_term(7)])], boost=2.0), {}),
            (And([by_term(1), by_term(2), Not(by_term(3))]), {}),
            (And([by_term(1), by_term(7), Not(Or([by_term(3), by_term(4)])), by_doc_set(2)]), {}),
            (And([And([by_term(1), Or([by_term(2), by_term(7)])]), Not(by_term(3))]), {}),
            (Or([ab, by_term(3, 0.5)], min_match=1), {"and_clauses": True}),
            (by_terms([1, 2, 3], 2), {}),
            (by_phrase([1, 2]), {})]
    for flt, kw in kept:
        with_kw = search.prepare([flt], sc, st, boolean_trees=True, **kw)
        without = search.prepare([flt], sc, st, **kw)
        assert with_kw == without and with_kw[0].tree is None, flt
        a, b = (search.QueryArrays.from_prepared(segs, x, 10) for x in (with_kw, without))
        assert a.queries.tobytes() == b.queries.tobytes() and a.terms.tobytes() == b.terms.tobytes()
        assert not (a.terms["kind"] & TREE).any()
    # ... and without and_clauses the Or of clauses is a tree
    assert prep(Or([ab, by_term(3, 0.5)])).tree == [(AND, 2, 0, False), None, None, None]
    # what is refused under the keyword, and how it says so
    for bad, msg in (
            (And([by_term(1), Or([by_term(2), ab], merge=search.MERGE_MAX)]), "merges with SUM at every level"),
            (Or([And([by_term(1), Not(by_term(2))], merge=search.MERGE_MIN), by_term(4)]), "merges with SUM at every level"),
            (Or([ab, by_term(3)], merge=search.MERGE_MAX), "merges with SUM at every level"),
            (And([by_term(1), Or([by_term(2), And([by_term(3), by_phrase([4, 5])])])]), "by_phrase inside a nested"),
            (And([by_term(1), Or([by_term(2), And([by_term(3), by_terms([4, 5])])])]), "by_terms inside a nested"),
            (And([by_term(1), Or([ab, by_doc_set(0)])]), "by_doc_set inside a nested"),
            (And([Or([ab, by_term(3)]), by_doc_set(0)]), "by_doc_set inside a nested"),
            (Or([And([by_term(1), Not(by_term(2))]), Not(by_term(3))]), "zero-score fill"),
            (And([by_term(1), Or([ab, Not(by_term(3))])]), "zero-score fill"),
            (Or([ab, And([Not(by_term(3)), Not(by_term(4))])]), "only Not children"),
            (Not(Or([ab, by_term(3)])), "only Not"),
            (chain(list(range(17))), "at most 16 leaves"),
            (Or([ab, Or([by_term(3), by_term(4)], min_match=0)]), "min_match 0"),
            (Or([ab, And([])]), "without children"),
            (And([by_term(1), Or([by_term(2), And([by_term(3), by_term(4)], op=MM)])]), "with op")):
        with pytest.raises(ValueError, match=msg):
            prep(bad)
    with pytest.raises(ValueError, match=r"boolean_trees=True"):
        search.prepare_filters([Or([ab, by_term(3)])], sc, st, segs, 10)
    # without the keyword every refusal stays word for word
    for bad, msg in (
            (Or([And([by_term(1), Or([by_term(2), by_term(3)])]), by_term(4)]), "only flat"),
            (And([by_term(1), Or([by_term(2), ab])]), "an Or with And children \\(a OR \\(b AND c\\)\\) is not on the GPU path"),
            (Or([And([by_term(1), Not(by_term(2))]), by_term(4)]), "only flat"),
            (And([by_term(1), Or([by_term(2), by_term(3), by_term(4)], min_match=2)]),
             "an Or group with min_match > 1 is not on the GPU path"),
            (And([by_term(1), Not(And([by_term(2), by_term(3)]))]), "Not of And is not on the GPU path")):
        with pytest.raises(ValueError, match=msg):
            search.prepare([bad], sc, st)
    with pytest.raises(ValueError, match="with an Or inside"):
        search.prepare([Or([And([by_term(1), Or([by_term(2), by_term(3)])]), by_term(4)])], sc, st, and_clauses=True)
    with pytest.raises(ValueError, match="with a Not inside"):
        search.prepare([Or([And([by_term(1), Not(by_term(2))]), by_term(4)])], sc, st, and_clauses=True)


# ---------------------------------------------------------------- emulator --

def test_boolean_trees_abi_emulated(simlib):
    case_abi(simlib)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_boolean_trees_lists_emulated(simlib, layout):
    case_lists(simlib, layout)


def test_boolean_trees_routes_emulated(simlib):
    case_routes(simlib)


def test_boolean_trees_parity_emulated(simlib):
    case_parity(simlib, 30_000, 128, synth.LAYOUT_SIMD4)


def test_boolean_trees_mixed_emulated(simlib):
    case_mixed(simlib, 26_000, 96, synth.LAYOUT_SIMD4)


def test_boolean_trees_multi_emulated(simlib):
    case_multi(simlib, (3_000, 1_500, 4_000))


def test_boolean_trees_streams_emulated(simlib):
    case_streams(simlib, 14_000, 64)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_boolean_trees_chunks_emulated(simlib, layout):
    case_chunks(simlib, layout)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_boolean_trees_min_scores_emulated(simlib, layout):
    case_min_scores(simlib, layout)


# --------------------------------------------------------------------- GPU --

@pytest.mark.gpu
def test_boolean_trees_abi_gpu(gpulib):
    case_abi(gpulib)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_boolean_trees_lists_gpu(gpulib, layout):
    case_lists(gpulib, layout)


@pytest.mark.gpu
def test_boolean_trees_routes_gpu(gpulib):
    case_routes(gpulib)


@pytest.mark.gpu
def test_boolean_trees_parity_gpu(gpulib):
    case_parity(gpulib, 60_000, 128, synth.LAYOUT_SIMD4)


@pytest.mark.gpu
def test_boolean_trees_mixed_gpu(gpulib):
    case_mixed(gpulib, 60_000, 128, synth.LAYOUT_SIMD4)


@pytest.mark.gpu
def test_boolean_trees_multi_gpu(gpulib):
    case_multi(gpulib, (30_000, 10_000, 45_000), max_rank=128, k=100)


@pytest.mark.gpu
def test_boolean_trees_streams_gpu(gpulib):
    case_streams(gpulib, 60_000, 128)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_boolean_trees_chunks_gpu(gpulib, layout):
    case_chunks(gpulib, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_boolean_trees_min_scores_gpu(gpulib, layout):
    case_min_scores(gpulib, layout)
