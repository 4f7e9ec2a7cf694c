"""Or filters with And children — a disjunction of clauses, IRS_HIP_CLAUSE_AND: `(a AND b) OR c`
(Or::prepare prepares every child on its own, an And child becomes a conjunction, the Or a
disjunction or min-match disjunction over the children; boolean_filter.cpp:150-210,
boolean_query.cpp:60-145 and :212-247), on k_clause_pilot / k_clause_score (csrc/clauses.h).

Expected values come from the oracle as it stands, composed here the way tests/test_nested_boolean.py
composes groups: per clause oracle.score_all over the clause's entries with their boosts and
index-global statistics (OP_AND for two or more entries, OP_OR for one; a clause with an entry the
segment lacks is emptied HERE), a doc matches when at least max(1, min_match) clauses do, its score
is the float64 sum of the matching clauses' scores.  One body per case runs on the emulator (CPU tier)
and on the GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle
import parity
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, TFIDF, And, Not, Or, by_doc_set, by_phrase, by_term, by_terms

f32 = np.float32
TILE = 12288     # docs per accumulator tile of the clause kernels (kJoinTile)


# ------------------------------------------------------------- expectations --

def clauses_of(flt, mult=f32(1)):
    """The clauses of an Or tree, (term, boost product) per member — written out here, apart from
    search.or_clauses (the code under test): a by_term child is a clause of one, an And child's
    by_term (and nested And) members are one clause, an Or child's clauses join the parent's;
    boosts multiply from the top in float32."""
    mult = f32(mult * f32(flt.boost))

    def members(a, m):
        m = f32(m * f32(a.boost))
        out = []
        for s in a.subs:
            if type(s) is by_term:
                out.append((s.term, f32(m * f32(s.boost))))
            else:
                assert type(s) is And
                out += members(s, m)
        return out

    out = []
    for s in flt.subs:
        if type(s) is by_term:
            out.append([(s.term, f32(mult * f32(s.boost)))])
        elif type(s) is And:
            out.append(members(s, mult))
        else:
            assert type(s) is Or
            out += clauses_of(s, mult)
    return out


def _present(seg, t):
    return 0 <= t < len(seg.metas) and int(seg.metas[t]["docs_count"]) > 0


def _score_entries(seg, ent, op, scorer, all_segs):
    terms = [t for t, _ in ent]
    dwf = sum(s.docs_with_field for s in all_segs)
    ttf = sum(s.total_term_freq for s in all_segs)
    dwt = [sum(int(s.metas[t]["docs_count"]) if 0 <= t < len(s.metas) else 0 for s in all_segs) for t in terms]
    sc, m = oracle.score_all(parity.oracle_view(seg), parity.metas_for(seg, terms), op,
                             parity.oracle_scorer(scorer), dwf, dwt, ttf, [b for _, b in ent])
    n1 = seg.num_docs + 1
    m = m[:n1].astype(bool)
    return np.where(m, sc[:n1], f32(0)).astype(f32), m


def expected(seg, flt, scorer, all_segs=None, exact=False):
    """(score f64[num_docs + 1], matched bool[num_docs + 1]) of an Or of clauses on `seg`;
    statistics over `all_segs` (default: this segment).  exact: every ENTRY scored on its own and
    summed in float64 (the precondition of case_parity) instead of the oracle's float32 sum per
    clause."""
    all_segs = all_segs or [seg]
    n1 = seg.num_docs + 1
    count = np.zeros(n1, np.int64)
    score = np.zeros(n1, np.float64)
    for cl in clauses_of(flt):
        if not all(_present(seg, t) for t, _ in cl):
            continue     # an absent entry: the clause is empty in this segment
        sc, m = _score_entries(seg, cl, oracle.OP_AND if len(cl) > 1 else oracle.OP_OR, scorer, all_segs)
        if exact:
            sc = np.zeros(n1, np.float64)
            for e in cl:
                sc += _score_entries(seg, [e], oracle.OP_OR, scorer, all_segs)[0].astype(np.float64)
        count += m
        score += np.where(m, sc, 0).astype(np.float64)
    matched = count >= max(1, int(flt.min_match))
    return np.where(matched, score, 0.0), matched


def check(flt, k, h, c, t, scores, matched):
    """test_multiterm.check: total hits and doc sets exactly, scores to REL_TOL, order (score
    descending, doc ascending), membership around the k-th score."""
    n_match = int(matched.sum())
    assert int(t) == n_match, ("total hits", flt, int(t), n_match)
    n = int(c)
    assert n == min(k, n_match), ("count", flt, n, k, n_match)
    if n == 0:
        return
    docs = h[:n]["doc"].astype(np.int64)
    sc = h[:n]["score"]
    assert len(set(docs.tolist())) == n, ("duplicate docs", flt)
    assert matched[docs].all(), ("unmatched doc returned", flt)
    if n == n_match:
        assert set(docs.tolist()) == set(np.nonzero(matched)[0].tolist()), ("doc set", flt)
    ref = scores[docs]
    rel = np.abs(sc - ref) / np.maximum(np.abs(ref), 1e-30)
    assert rel.max() <= parity.REL_TOL, ("score", flt, float(rel.max()))
    assert ((sc[:-1] > sc[1:]) | ((sc[:-1] == sc[1:]) & (docs[:-1] < docs[1:]))).all(), ("order", flt)
    thr = np.sort(scores[matched])[::-1][n - 1]
    must = np.nonzero(matched & (scores > thr * (1 + 2 * parity.REL_TOL)))[0]
    assert np.isin(must, docs).all(), ("missing doc above the k-th score", flt)
    assert (ref >= thr * (1 - 2 * parity.REL_TOL)).all(), ("doc below the k-th score", flt)


def _run(sr, filters, scorer, k, stats, cand_cap=0, path=None):
    prep = search.prepare(filters, scorer, stats, and_clauses=True)
    b = sr.batch(prep, k) if not isinstance(sr, list) else search.QueryBatch(sr, prep, k)
    if cand_cap:
        b.configure(cand_cap=cand_cap)
    if path is not None:
        b.set_path(path)
    h, c, t = (x.copy() for x in b.run().results())
    info = {"reruns": b.reruns(), "clause": b.clause_units(), "wide": b.wide_units(), "path": b.path(),
            "paired": b.paired_tiles(), "streams": b.stream_counts()}
    b.close()
    return h, c, t, info


# -------------------------------------------------------------------- cases --

def case_abi(L):
    """IRS_HIP_CLAUSE_AND at batch create: where the flag may stand, entry counts, merge, excluded
    entries, frequencies, min_match; the batch controls that are refused on such a batch, which
    afterwards still runs."""
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
    CL = _lib.CLAUSE_AND
    assert CL == 0x1000

    def create(prep, mutate=None, k=10):
        arr = search.QueryArrays.from_prepared([sr], prep, k)
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

    def flag(*js):
        def f(arr):
            for j in js:
                arr.terms[0, j]["kind"] |= CL
        return f

    def query(**kw):
        def f(arr):
            for name, v in kw.items():
                arr.queries[0][name] = v
        return f

    def prep(flt):
        return search.prepare([flt], BM25(), st, and_clauses=True)

    abc = prep(Or([And([by_term(0), by_term(1)]), by_term(2)]))
    assert abc[0].op == _lib.OP_OR and abc[0].clause == [False, True, False]
    arr = search.QueryArrays.from_prepared([sr], abc, 10)
    assert [int(x) & CL for x in arr.terms[0, :3]["kind"]] == [0, CL, 0]
    assert create(abc) == _lib.OK
    # where the flag may not stand
    assert create(abc, flag(0)) == _lib.EINVAL                                # the first included entry
    flat = prep(Or([by_term(0), by_term(1)]))
    flat[0].excluded = [5]
    assert create(flat, flag(2)) == _lib.EINVAL                               # an excluded entry
    assert create(prep(And([by_term(0), by_term(1)])), flag(1)) == _lib.EINVAL
    assert create(prep(by_phrase([0, 1])), flag(1)) == _lib.EINVAL
    assert create(prep(by_terms([0, 1, 2])), flag(1)) == _lib.EINVAL
    # 16 entries, not 17
    sixteen = prep(Or([And([by_term(0), by_term(1)])] + [by_term(t) for t in range(2, 16)]))
    assert len(sixteen[0].terms) == 16 and create(sixteen) == _lib.OK
    seventeen = prep(Or([And([by_term(0), by_term(1)])] + [by_term(t) for t in range(2, 16)]))
    seventeen[0].terms.append(16)
    seventeen[0].scorers.append(seventeen[0].scorers[0])
    seventeen[0].clause.append(False)
    assert create(seventeen) == _lib.EUNSUPPORTED
    with pytest.raises(ValueError):
        prep(Or([And([by_term(0), by_term(1)])] + [by_term(t) for t in range(2, 17)]))
    # merges, excluded entries
    assert create(abc, query(merge=search.MERGE_MAX)) == _lib.EUNSUPPORTED
    assert create(abc, query(merge=search.MERGE_MIN)) == _lib.EUNSUPPORTED
    assert create(abc, query(merge=3)) == _lib.EINVAL
    with_excl = prep(Or([And([by_term(0), by_term(1)]), by_term(2)]))
    with_excl[0].excluded = [5]
    assert create(with_excl) == _lib.EUNSUPPORTED
    # what an entry scored from decoded streams cannot be
    assert create(abc, edit(term={1: 20})) == _lib.EUNSUPPORTED       # a frequency of 256
    assert create(abc, edit(term={1: 21})) == _lib.OK                 # 255 fits
    assert create(abc, edit(c0={1: -1.0})) == _lib.EINVAL
    assert create(abc, edit(kind={1: 7 | CL})) == _lib.EINVAL
    assert create(abc, edit(term={1: len(lists)})) == _lib.EINVAL
    assert create(abc, edit(term={1: _lib.NO_TERM})) == _lib.OK
    assert create(abc, edit(c0={1: 0.0})) == _lib.OK
    five = edit(norm_const={j: 0.3 + 0.1 * j for j in range(5)})
    four = edit(norm_const={j: 0.3 + 0.1 * j for j in range(3)})
    assert create(sixteen, five) == _lib.EUNSUPPORTED and create(sixteen, four) == _lib.OK
    # min_match counts clauses; 0 under MINMATCH is refused as for every MINMATCH query
    assert create(abc, query(op=_lib.OP_MINMATCH, min_match=0)) == _lib.EUNSUPPORTED
    for mm in (1, 2, 3):      # (3: more than the two clauses — an empty query, not an error)
        assert create(abc, query(op=_lib.OP_MINMATCH, min_match=mm)) == _lib.OK, mm

    # refused on a batch with such a query, which afterwards still runs correctly
    flts = [Or([And([by_term(0), by_term(1)]), by_term(2)]), Or([by_term(1), by_term(2)]),
            Or([And([by_term(3), by_term(4)]), And([by_term(3), by_term(5)]), by_term(6)], min_match=2)]
    b = sr.batch(search.prepare(flts, BM25(), st, and_clauses=True), 10)
    assert b.clause_units() == 2 and b.wide_units() == 0
    rows = np.full((1, num_docs // 64 + 1), ~np.uint64(0), np.uint64)
    with pytest.raises(_lib.IrsHipError) as e:
        b.set_doc_sets(rows, np.zeros(3, np.uint32))
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
    # a flat Or and a grouped And: no clause unit
    plain = sr.batch(search.prepare([flts[1], And([by_term(0), Or([by_term(1), by_term(2)])])], BM25(), st), 10)
    plain.run()
    assert plain.clause_units() == 0
    plain.close()
    sr.close()


N_HAND = 2 * TILE + 5     # three tiles, the last one nearly empty
ALL = 5000                # the doc every term holds
BORDER = (TILE, TILE + 1, N_HAND)   # the last doc of tile 0, the first of tile 1, the last doc
T128, T129, TTAIL, TONE, TBIG, TEMPTY = 10, 11, 12, 13, 2, 19
ABSENT = 10_000
N_TERMS = 20


def hand_lists():
    """Term t holds the docs d with d % (5 + t) == t % 5, frequencies 1 + (7 d + t) % 5 — except
    T128 / T129 / TTAIL / TONE: exactly 128 / 129 / 50 / 1 postings, and TBIG, whose frequencies run
    up to 255 (the general score form next to the table rows).  Every term holds doc ALL; the even
    terms below 10 hold the docs at the tile border and the last doc."""
    N = N_HAND
    lists = []
    for t in range(N_TERMS):
        if t == T128:
            docs = {100 + 190 * i for i in range(127)}
        elif t == T129:
            docs = {50 + 180 * i for i in range(128)}
        elif t == TTAIL:
            docs = {7 + 400 * i for i in range(49)}
        elif t == TONE:
            docs = set()
        else:
            docs = set(range(t % 5 if t % 5 else 5 + t, N + 1, 5 + t))
        assert ALL not in docs or t not in (T128, T129, TTAIL)
        docs.add(ALL)
        if t % 2 == 0 and t < 10:
            docs.update(BORDER)
        d = np.array(sorted(docs), np.uint32)
        f = (1 + (7 * d + t) % 5).astype(np.uint32)
        if t == TBIG:
            f = (1 + d % 255).astype(np.uint32)
        lists.append((d, f))
    assert len(lists[T128][0]) == 128 and len(lists[T129][0]) == 129 and len(lists[TTAIL][0]) == 50
    assert len(lists[TONE][0]) == 1 and int(lists[TBIG][1].max()) == 255
    return lists


def T(t, boost=1.0):
    return by_term(t, boost)


def hand_queries():
    """(filter, what it is about), by name."""
    q = {}
    q["conj16"] = Or([And([T(t) for t in range(16)])])                       # a clause of 16
    q["8x2"] = Or([And([T(2 * i), T(2 * i + 1)]) for i in range(8)])         # 8 clauses of 2
    q["2+14"] = Or([And([T(0), T(1)])] + [T(t) for t in range(2, 16)])       # one clause, 14 single terms
    q["half"] = Or([And([T(0), T(1)]), T(TONE)])        # a doc of 0 without 1 must not match
    q["shared"] = Or([And([T(0), T(2)]), And([T(0), T(4)])])                 # term 0 in two clauses
    q["short"] = Or([And([T(T128), T(0)]), And([T(T129), T(1)]), T(TTAIL), T(TONE)])
    q["absent_in"] = Or([And([T(0), T(ABSENT)]), And([T(2), T(3)]), T(4)])   # the first clause is empty
    q["absent_one"] = Or([And([T(0), T(1)]), T(ABSENT), T(TEMPTY)])
    q["all_empty"] = Or([And([T(0), T(ABSENT)]), T(TEMPTY), And([T(TEMPTY), T(1)])])
    q["zero_clause"] = Or([And([T(0), T(1)], boost=0.0), T(TONE)])           # matches, scores 0
    q["boosts"] = Or([And([T(0, 0.25), T(2, 4.0)], boost=0.5), T(3, 2.0),
                      And([T(4, 0.5), And([T(6), T(8, 0.25)], boost=2.0)], boost=4.0),
                      Or([T(5, 0.5), And([T(7), T(9, 4.0)])], boost=2.0)], boost=0.25)
    five = [And([T(0), T(2)]), And([T(0), T(4)]), T(6), And([T(2), T(8)]), T(1)]
    for mm in (1, 2, 5, 6):                                                  # 5 clauses
        q["mm%d" % mm] = Or(list(five), min_match=mm)
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
    only0 = min(has[0] - has[1])                          # holds one member of (0 AND 1) only
    assert only0 not in has[TONE]
    assert all(d in has[0] and d in has[2] and d in has[4] for d in BORDER)
    assert all(ALL in s for s in has)
    for scorer in (TFIDF(True), BM25(), BM25(0.0, 0.0)):
        exp = [expected(seg, f, scorer) for f in filters]
        E = {n: exp[at[n]] for n in names}
        # what the lists say
        assert set(np.nonzero(E["conj16"][1])[0].tolist()) == {ALL}            # TONE holds ALL only
        assert not E["half"][1][only0] and E["half"][1][ALL]
        assert set(np.nonzero(E["half"][1])[0].tolist()) == (has[0] & has[1]) | {ALL}
        one = {t: _score_entries(seg, [(t, f32(1))], oracle.OP_OR, scorer, [seg])[0].astype(np.float64) for t in (0, 2, 4)}
        for d in BORDER:      # both clauses complete: term 0 scores twice
            want = 2 * one[0][d] + one[2][d] + one[4][d]
            assert E["shared"][1][d] and abs(E["shared"][0][d] - want) <= 1e-6 * want
        assert set(np.nonzero(E["absent_in"][1])[0].tolist()) == (has[2] & has[3]) | has[4]
        assert set(np.nonzero(E["absent_one"][1])[0].tolist()) == has[0] & has[1]
        assert not E["all_empty"][1].any()
        zc = E["zero_clause"]
        assert zc[1].sum() == len(has[0] & has[1]) and (zc[0][list((has[0] & has[1]) - {ALL})] == 0).all()
        assert E["mm5"][1][ALL] and not E["mm6"][1].any() and E["mm2"][1][TILE]
        assert E["mm1"][1].sum() > E["mm2"][1].sum() > E["mm5"][1].sum() >= 1
        for k in (1, 10, 4096):
            h, c, t, info = _run(sr, filters, scorer, k, st)
            assert info["clause"] == len(filters) and info["wide"] == 0
            for q, flt in enumerate(filters):
                check(flt, k, h[q], c[q], t[q], *exp[q])
            assert int(t[at["conj16"]]) == 1 and int(t[at["all_empty"]]) == 0 and int(t[at["mm6"]]) == 0
            if k == 4096:
                assert int(h[at["conj16"], 0]["doc"]) == ALL
                zq = at["zero_clause"]
                assert int(c[zq]) == int(zc[1].sum()) and int(h[zq, 0]["doc"]) == ALL
                assert (h[zq, 1:int(c[zq])]["score"] == 0).all()
        # only single terms, written with nested Ors: the flat Or's results exactly, no clause unit
        nested = Or([T(0), Or([T(1, 2.0), Or([T(3)])]), T(4, 0.5), Or([T(TTAIL)])])
        flat = Or([T(0), T(1, 2.0), T(3), T(4, 0.5), T(TTAIL)])
        hn, cn, tn, i_n = _run(sr, [nested], scorer, 100, st)
        hf, cf, tf, i_f = _run(sr, [flat], scorer, 100, st)
        assert i_n["clause"] == 0 and i_f["clause"] == 0
        assert np.array_equal(hn, hf) and np.array_equal(cn, cf) and np.array_equal(tn, tf)
    # every score ties (zero boosts): the candidates overflow a small buffer; exact re-run, tie order
    ties = [Or([And([T(0, 0.0), T(2, 0.0)]), T(4, 0.0)]),
            Or([And([T(1), T(3)]), And([T(5), T(7)]), T(6)], boost=0.0, min_match=1), named["8x2"]]
    h, c, t, info = _run(sr, ties, BM25(0.0, 0.0), 64, st, cand_cap=64)
    assert info["reruns"] > 0 and info["clause"] == 3
    for q, flt in enumerate(ties):
        sc, m = expected(seg, flt, BM25(0.0, 0.0))
        check(flt, 64, h[q], c[q], t[q], sc, m)
        if q < 2:
            assert (h[q, :64]["score"] == 0).all()
            assert np.array_equal(h[q, :64]["doc"], np.nonzero(m)[0][:64])
    sr.close()
    # deleted docs: a border doc, the last doc, the doc of the 16-clause, a doc that would complete
    # (0 AND 1)
    both01 = min((has[0] & has[1]) - {ALL})
    gone = [7, TILE, ALL, N, both01]
    seg2 = synth.segment_from_lists(lists, N, layout, norms=norms)
    seg2.doc_mask = np.array(sorted(gone), np.uint32)
    sr2 = search.SegmentReader.from_synth(seg2, L=L)
    st2 = [parity.segment_stats(seg2)]
    for scorer in (BM25(), TFIDF(True)):
        sub = [named["conj16"], named["half"], named["shared"], named["mm2"], named["2+14"]]
        h, c, t, _ = _run(sr2, sub, scorer, 100, st2)
        for q, flt in enumerate(sub):
            sc, m = expected(seg2, flt, scorer)
            assert not m[gone].any()
            check(flt, 100, h[q], c[q], t[q], sc, m)
        assert int(t[0]) == 0
        assert int(t[1]) == int(expected(seg, named["half"], scorer)[1].sum()) - 2     # ALL and both01
    sr2.close()


def random_filters(n, seed, frequent=12):
    """Ors of 1 to 8 clauses with 2 to 16 entries in all, terms from the `frequent` most frequent
    ranks (so that conjunctions of them have docs), boosts at all three levels, min_match mostly 1."""
    rng = np.random.default_rng(seed)
    pick = [0.25, 0.5, 1.0, 1.0, 2.0, 4.0]
    out = []
    for i in range(n):
        n_ent = int(rng.integers(2, 17))
        n_cl = int(rng.integers(1, min(8, n_ent) + 1))
        if n_cl == n_ent:     # (at least one clause of two: a clause query)
            n_cl -= 1
        sizes = np.ones(n_cl, np.int64)
        for _ in range(n_ent - n_cl):
            small = np.nonzero(sizes < 3)[0]      # (clauses of up to 3: frequent terms still intersect)
            sizes[rng.choice(small) if small.size else rng.integers(n_cl)] += 1
        subs = []
        for s in sizes:
            terms = rng.choice(frequent, int(s), replace=False) if s <= frequent else rng.choice(frequent, int(s))
            members = [by_term(int(t), float(rng.choice(pick))) for t in terms]
            subs.append(members[0] if s == 1 else And(members, boost=float(rng.choice(pick))))
        mm = 1 if i % 3 else int(rng.integers(1, min(n_cl, 2) + 1))
        out.append(Or(subs, min_match=mm, boost=float(rng.choice(pick))))
    return out


PARITY_SEED = 5


def case_parity(L, num_docs, max_rank, layout, n_queries=24, seed=PARITY_SEED):
    seg = synth.build_segment(num_docs, max_rank, layout=layout)
    seg.doc_mask = np.arange(9, num_docs, 101, dtype=np.uint32)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    filters = random_filters(n_queries, seed)
    assert all(2 <= sum(len(c) for c in clauses_of(f)) <= 16 and 1 <= len(clauses_of(f)) <= 8 for f in filters)
    for scorer in (BM25(), TFIDF(True)):
        exp = [expected(seg, f, scorer) for f in filters]
        exact = [expected(seg, f, scorer, exact=True)[0] for f in filters]
        assert all(m.any() for _, m in exp), "every query has matches"
        for k in (64, 128):
            h, c, t, info = _run(sr, filters, scorer, k, st)
            assert info["clause"] == n_queries
            for q, flt in enumerate(filters):
                # the precondition: for the docs compared, the composed float32 sums are within
                # REL_TOL / 4 of the float64 sum — a failure below points at the kernel
                docs = h[q, :int(c[q])]["doc"].astype(np.int64)
                ref = exp[q][0][docs]
                err = np.abs(ref - exact[q][docs]) / np.maximum(exact[q][docs], 1e-30)
                assert docs.size == 0 or err.max() < parity.REL_TOL / 4, ("precondition", q, float(err.max()))
                check(flt, k, h[q], c[q], t[q], *exp[q])
    sr.close()


def case_mixed(L, num_docs, max_rank, layout):
    """Clause queries interleaved with ordinary ones: the ordinary ones are bit for bit what a batch
    without the clause queries gives, on the same path; the clause ones equal a batch of their own."""
    seg = synth.build_segment(num_docs, max_rank, layout=layout)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    rng = np.random.default_rng(17)
    cl = random_filters(4, 23)
    ordinary = [Or([by_term(int(t)) for t in rng.choice(max_rank, 8, replace=False)]) for _ in range(3)]
    ordinary += [And([by_term(int(t)) for t in rng.choice(16, 3, replace=False)]) for _ in range(2)]
    ordinary += [Or([by_term(int(t)) for t in rng.choice(24, 6, replace=False)], min_match=2)]
    ordinary += [And([by_term(1), Or([by_term(2), by_term(7)])])]        # a grouped And
    ordinary += [by_terms(list(range(3, 25)), 2)]
    mixed = [cl[0], ordinary[0], ordinary[3], cl[1], ordinary[1], ordinary[5], ordinary[6], cl[2],
             ordinary[2], ordinary[4], ordinary[7], cl[3]]
    at_c = [mixed.index(f) for f in cl]
    at_o = [mixed.index(f) for f in ordinary]
    for scorer in (BM25(), TFIDF(True)):
        for path in (None, _lib.PATH_JOINED, _lib.PATH_ITEMS):
            hm, cm, tm, im = _run(sr, mixed, scorer, 50, st, path=path)
            ho, co, to, io = _run(sr, ordinary, scorer, 50, st, path=path)
            hc, cc, tc, ic = _run(sr, cl, scorer, 50, st, path=path)
            assert im["clause"] == 4 and io["clause"] == 0 and ic["clause"] == 4
            assert im["wide"] == 1 and io["wide"] == 1 and ic["wide"] == 0
            assert im["path"] == io["path"] and im["paired"] == io["paired"], (path, im, io)
            assert np.array_equal(hm[at_o], ho) and np.array_equal(cm[at_o], co) and np.array_equal(tm[at_o], to)
            assert np.array_equal(hm[at_c], hc) and np.array_equal(cm[at_c], cc) and np.array_equal(tm[at_c], tc)
            for q in at_c:
                check(mixed[q], 50, hm[q], cm[q], tm[q], *expected(seg, mixed[q], scorer))
        parity.check_single_segment(seg, ordinary[:6], scorer, 50, ho[:6], co[:6], to[:6])
    sr.close()


def case_multi(L, sizes, max_rank=96, k=50):
    """create_multi: a clause term absent from one segment, statistics over all segments, units
    indexed segment * n_queries + query, the merged top k against the composed expectation."""
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    segs = [synth.build_segment(int(n), max_rank, first_doc=int(f)) for n, f in zip(sizes, first)]
    segs[1].metas[5]["docs_count"] = 0
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    stats = [parity.segment_stats(s) for s in segs]
    filters = random_filters(4, 41)
    filters.append(Or([And([T(5), T(1)]), And([T(2), T(3)], boost=2.0), T(40)]))     # segment 1: the first clause empty
    filters.append(Or([And([T(5, 2.0), T(0)]), And([T(5), T(4)])], min_match=1))     # segment 1: nothing
    filters.append(Or([And([T(0), T(1)]), And([T(0), T(2)]), T(5)], min_match=2))
    for scorer in (BM25(), TFIDF(True)):
        prep = search.prepare(filters, scorer, stats, and_clauses=True)
        dwf = sum(s.docs_with_field for s in segs)
        ttf = sum(s.total_term_freq for s in segs)
        dwt5 = sum(int(s.metas[5]["docs_count"]) for s in segs)
        assert prep[4].scorers[0] == scorer.term_scorer(scorer.collect(dwf, dwt5, ttf), 1.0)
        b = search.QueryBatch(readers, prep, k)
        assert b.clause_units() == len(filters) * len(segs)
        b.set_shared_threshold(True)       # (leaves every clause unit a threshold of its own)
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
    """The clause units' terms are streams of the batch's one set: shared with an ordinary query and
    between clauses, served by the device's stream cache, the same results without it."""
    seg = synth.build_segment(num_docs, max_rank)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    a, b_, c_, d = 2, 3, 4, 5
    clause = Or([And([T(a), T(b_)]), And([T(a), T(c_)])])
    plain = Or([T(a), T(b_), T(d)])
    flts = [clause, plain]
    search.set_stream_cache(0, L=L)
    try:
        h0, c0, t0, i0 = _run(sr, flts, BM25(), 20, st, path=_lib.PATH_JOINED)
        assert i0["path"] == _lib.PATH_JOINED and i0["clause"] == 1
        assert i0["streams"] == (4, 4), i0       # a, b, c, d: the union, all decoded by the run
        hc, cc, tc, ic = _run(sr, [clause], BM25(), 20, st)
        assert ic["streams"] == (3, 3), ic
        search.set_stream_cache(64 << 20, L=L)
        h1, c1, t1, i1 = _run(sr, flts, BM25(), 20, st, path=_lib.PATH_JOINED)
        h2, c2, t2, i2 = _run(sr, flts, BM25(), 20, st, path=_lib.PATH_JOINED)
        assert i1["streams"] == (4, 4) and i2["streams"] == (4, 0), (i1, i2)
        for h, c, t in ((h1, c1, t1), (h2, c2, t2)):
            assert np.array_equal(h, h0) and np.array_equal(c, c0) and np.array_equal(t, t0)
        assert np.array_equal(hc[0], h0[0])
        check(clause, 20, h0[0], c0[0], t0[0], *expected(seg, clause, BM25()))
    finally:
        search.set_stream_cache(0, L=L)
        L.irs_hip_device_trim(0)
    sr.close()


# --------------------------------------------------------------- host only --

def test_prepare_or_clauses():
    st = [search.SegmentStats(1000, 100_000, np.arange(64, dtype=np.int64) * 3 + 20),
          search.SegmentStats(500, 40_000, np.arange(32, dtype=np.int64) * 2 + 1)]
    sc = BM25()
    flt = Or([And([by_term(7, 0.5), And([by_term(9, 2.0)], boost=4.0)], boost=0.25), by_term(40, 2.0),
              Or([by_term(3), And([by_term(7), by_term(11)])], boost=0.5), And([by_term(12)])], boost=1.5)
    want = [[(7, f32(f32(f32(1.5) * f32(0.25)) * f32(0.5))), (9, f32(f32(f32(f32(1.5) * f32(0.25)) * f32(4.0)) * f32(2.0)))],
            [(40, f32(f32(1.5) * f32(2.0)))],
            [(3, f32(f32(1.5) * f32(0.5)))],
            [(7, f32(f32(1.5) * f32(0.5))), (11, f32(f32(1.5) * f32(0.5)))],
            [(12, f32(1.5))]]
    got = search.or_clauses(flt)
    assert got == want and got == clauses_of(flt)
    assert all(type(b) is np.float32 for c in got for _, b in c)
    p = search.prepare([flt], sc, st, and_clauses=True)[0]
    assert p.op == _lib.OP_OR and p.terms == [7, 9, 40, 3, 7, 11, 12] and p.merge == search.MERGE_SUM
    assert p.clause == [False, True, False, False, False, True, False]
    # statistics per term, as everywhere: the field's over all segments, the term's where it exists
    assert p.scorers[2] == sc.term_scorer(sc.collect(1500, int(st[0].docs_count[40]), 140_000), want[1][0][1])
    assert p.scorers[0] == sc.term_scorer(sc.collect(1500, int(st[0].docs_count[7] + st[1].docs_count[7]), 140_000), want[0][0][1])
    segs = [type("S", (), {"metas": np.zeros(n)})() for n in (64, 32)]
    arr = search.QueryArrays.from_prepared(segs, [p], 10)
    assert tuple(arr.queries[0]) == (_lib.OP_OR, 7, 0, 10, 1, search.MERGE_SUM)
    kinds = arr.terms[0, :7]["kind"].tolist()
    assert [k & _lib.CLAUSE_AND for k in kinds] == [0, _lib.CLAUSE_AND, 0, 0, 0, _lib.CLAUSE_AND, 0]
    assert all(k & ~_lib.CLAUSE_AND == _lib.SCORE_BM25 for k in kinds)
    assert arr.terms[1, :7]["term"].tolist() == [7, 9, _lib.NO_TERM, 3, 7, 11, 12]
    mm = search.prepare([Or([And([by_term(1), by_term(2)]), by_term(3), by_term(4)], min_match=2)], sc, st, and_clauses=True)[0]
    assert mm.op == _lib.OP_MINMATCH and mm.min_match == 2 and mm.clause == [False, True, False, False]
    # only single terms: a flat Or, and a flat Or's arrays are what they were, byte for byte
    flat = Or([by_term(1), by_term(2, 2.0), by_term(3)], boost=0.5)
    nested = Or([by_term(1), Or([by_term(2, 2.0), And([by_term(3)])])], boost=0.5)
    pf, pn = search.prepare([flat], sc, st)[0], search.prepare([nested], sc, st, and_clauses=True)[0]
    assert pf.clause is None and pn.clause is None and pf == pn
    a_f = search.QueryArrays.from_prepared(segs, [pf], 10)
    a_n = search.QueryArrays.from_prepared(segs, [pn], 10)
    fast = search.prepare_filters([flat], sc, st, segs, 10)
    assert a_f.queries.tobytes() == a_n.queries.tobytes() == fast.queries.tobytes()
    assert a_f.terms.tobytes() == a_n.terms.tobytes() == fast.terms.tobytes()
    assert not (a_f.terms["kind"] & _lib.CLAUSE_AND).any()
    # what is refused, and how it says so
    ab = And([by_term(1), by_term(2)])
    for bad, msg in (
            (Or([And([by_term(1), Or([by_term(2), by_term(3)])]), by_term(4)]), "with an Or inside"),
            (Or([And([by_term(1), Not(by_term(2))]), by_term(4)]), "with a Not inside"),
            (Or([And([by_term(1), by_phrase([2, 3])]), by_term(4)]), "with a by_phrase inside"),
            (Or([ab, by_phrase([2, 3])]), "by_phrase inside an Or"),
            (Or([ab, by_term(4)], merge=search.MERGE_MAX), "merges with SUM"),
            (Or([And([by_term(1), by_term(2)], merge=search.MERGE_MIN), by_term(4)]), "merges with SUM"),
            (Or([ab, Or([by_term(3), by_term(4)], merge=search.MERGE_MAX)]), "merges with SUM"),
            (Or([ab, Or([by_term(3), by_term(4)], min_match=2)]), "min_match <= 1"),
            (Or([ab, Or([by_term(3), by_term(4)]), by_term(5)], min_match=2), "min_match <= 1"),
            (Or([ab, Not(by_term(3))]), "zero-score fill"),
            (And([Or([ab, by_term(3)]), Not(by_term(4))]), "Not around an Or with And children"),
            (And([Or([ab, by_term(3)]), by_doc_set(0)]), "by_doc_set on an Or with And children"),
            (Or([And([by_term(t) for t in range(9)]), And([by_term(t) for t in range(8)])]), "at most 16 terms"),
            (Or([And([]), by_term(1)]), "without children")):
        with pytest.raises(ValueError, match=msg):
            search.prepare([bad], sc, st, and_clauses=True)
    with pytest.raises(ValueError, match=r"and_clauses=True"):
        search.prepare_filters([Or([ab, by_term(3)])], sc, st, segs, 10)
    # (an And with an Or child holding an And stays refused as it was)
    with pytest.raises(ValueError, match="And children"):
        search.prepare([And([by_term(1), Or([by_term(2), ab])])], sc, st, and_clauses=True)
    # without the keyword prepare() refuses the shape as it always did
    with pytest.raises(ValueError, match="only flat"):
        search.prepare([Or([ab, by_term(3)])], sc, st)
    with pytest.raises(ValueError, match="only flat"):
        search.prepare([nested], sc, st)


# ---------------------------------------------------------------- emulator --

def test_or_clauses_abi_emulated(simlib):
    case_abi(simlib)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_or_clauses_lists_emulated(simlib, layout):
    case_lists(simlib, layout)


def test_or_clauses_parity_emulated(simlib):
    case_parity(simlib, 30_000, 128, synth.LAYOUT_SIMD4)


def test_or_clauses_mixed_emulated(simlib):
    case_mixed(simlib, 26_000, 96, synth.LAYOUT_SIMD4)


def test_or_clauses_multi_emulated(simlib):
    case_multi(simlib, (3_000, 1_500, 4_000))


def test_or_clauses_streams_emulated(simlib):
    case_streams(simlib, 14_000, 64)


# --------------------------------------------------------------------- GPU --

@pytest.mark.gpu
def test_or_clauses_abi_gpu(gpulib):
    case_abi(gpulib)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_or_clauses_lists_gpu(gpulib, layout):
    case_lists(gpulib, layout)


@pytest.mark.gpu
def test_or_clauses_parity_gpu(gpulib):
    case_parity(gpulib, 60_000, 128, synth.LAYOUT_SIMD4)


@pytest.mark.gpu
def test_or_clauses_mixed_gpu(gpulib):
    case_mixed(gpulib, 60_000, 128, synth.LAYOUT_SIMD4)


@pytest.mark.gpu
def test_or_clauses_multi_gpu(gpulib):
    case_multi(gpulib, (30_000, 10_000, 45_000), max_rank=128, k=100)


@pytest.mark.gpu
def test_or_clauses_streams_gpu(gpulib):
    case_streams(gpulib, 60_000, 128)
