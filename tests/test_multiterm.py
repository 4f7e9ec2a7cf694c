"""by_terms and wide scored expansions — IRS_HIP_OP_MULTITERM: a scored set of up to 64 (term, boost)
with min_match (terms_filter.cpp:110-153, MultiTermQuery::execute multiterm_query.cpp:114-181), on
k_wide_pilot / k_wide_score (csrc/wide.h).

Expected values come from the oracle as it stands: oracle.score_all / oracle.search with OP_OR resp.
OP_MINMATCH | (min_match << 8) over the query's entries with their boosts (the oracle drops the
entries a segment lacks and empties a query with fewer present entries than min_match, as the ABI
states it).  One body per case runs on the emulator (CPU tier) and on the GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle
import parity
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, TFIDF, And, Or, by_term, by_terms

f32 = np.float32
TILE = 12288     # docs per accumulator tile of the wide kernels (kJoinTile)


# ------------------------------------------------------------- expectations --

def entries(flt):
    """[(term, boost as the ABI gets it)] of a by_terms, or of a flat Or / And / by_term."""
    if isinstance(flt, by_terms):
        return [(t, f32(b) if flt.boost == 1.0 else f32(f32(flt.boost) * f32(b))) for t, b in flt.pairs()]
    _, subs = search._terms_of(flt)
    return [(s.term, f32(s.boost)) for s in subs]


def oracle_op(flt):
    if isinstance(flt, by_terms):
        mm = int(flt.min_match)
        return oracle.OP_OR if mm <= 1 else oracle.OP_MINMATCH | (mm << 8)
    return parity.oracle_op(flt, search._terms_of(flt)[0])


def expected(seg, flt, scorer, all_segs=None):
    """(scores f32[num_docs + 1], matched bool[num_docs + 1]) of `flt` on `seg`; statistics over
    `all_segs` (default: this segment)."""
    all_segs = all_segs or [seg]
    ent = entries(flt)
    terms = [t for t, _ in ent]
    dwf = sum(s.docs_with_field for s in all_segs)
    ttf = sum(s.total_term_freq for s in all_segs)
    dwt = [sum(int(s.metas[t]["docs_count"]) if 0 <= t < len(s.metas) else 0 for s in all_segs) for t in terms]
    scores, matched = oracle.score_all(parity.oracle_view(seg), parity.metas_for(seg, terms), oracle_op(flt),
                                       parity.oracle_scorer(scorer), dwf, dwt, ttf, [b for _, b in ent])
    n1 = seg.num_docs + 1
    matched = matched[:n1].astype(bool)
    return np.where(matched, scores[:n1], f32(0)).astype(f32), matched


def check(flt, k, h, c, t, scores, matched):
    """As check() of test_phrase_or.py: total hits and doc sets exactly, scores to REL_TOL, order
    (score descending, doc ascending), membership around the k-th score."""
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
    prep = search.prepare(filters, scorer, stats)
    b = sr.batch(prep, k) if not isinstance(sr, list) else search.QueryBatch(sr, prep, k)
    if cand_cap:
        b.configure(cand_cap=cand_cap)
    if path is not None:
        b.set_path(path)
    h, c, t = (x.copy() for x in b.run().results())
    info = {"reruns": b.reruns(), "wide": b.wide_units(), "path": b.path(), "paired": b.paired_tiles(),
            "streams": b.stream_counts()}
    b.close()
    return h, c, t, info


# -------------------------------------------------------------------- cases --

def case_abi(L):
    """IRS_HIP_OP_MULTITERM at batch create: entry counts, min_match, merge, what is refused; the
    batch controls that are refused on such a batch, which afterwards still runs."""
    num_docs = 3000
    rng = np.random.default_rng(11)
    lists = []
    for t in range(70):
        docs = np.unique(rng.choice(num_docs, 200 + 5 * t, replace=False) + 1).astype(np.uint32)
        lists.append((docs, (1 + (docs + t) % 4).astype(np.uint32)))
    lists[66] = (lists[66][0], np.where(lists[66][0] % 50 == 0, 256, 1).astype(np.uint32))   # tf 256
    lists[67] = (lists[67][0], np.where(lists[67][0] % 50 == 0, 255, 1).astype(np.uint32))   # tf 255
    seg = synth.segment_from_lists(lists, num_docs, synth.LAYOUT_SIMD4)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]

    def prep_n(n, mm=1):
        p = search.prepare([by_terms(list(range(min(n, 64))), mm)], BM25(), st)
        while len(p[0].terms) < n:     # (past what by_terms itself takes)
            p[0].terms.append(len(p[0].terms) % 60)
            p[0].scorers.append(p[0].scorers[0])
        return p

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

    def query(**kw):
        def f(arr):
            for name, v in kw.items():
                arr.queries[0][name] = v
        return f

    assert _lib.OP_MULTITERM == 4 and _lib.MAX_WIDE_TERMS == 64
    assert search.prepare([by_terms([1, 2, 3], 2)], BM25(), st)[0].op == _lib.OP_MULTITERM
    for n in (1, 16, 17, 33, 64):
        assert create(prep_n(n)) == _lib.OK, n
    assert create(prep_n(65)) == _lib.EUNSUPPORTED
    for n in (1, 17, 64):
        assert create(prep_n(n), query(min_match=0)) == _lib.EINVAL, n
        assert create(prep_n(n), query(min_match=n + 1)) == _lib.EINVAL, n
        assert create(prep_n(n), query(min_match=n)) == _lib.OK, n
    forty = prep_n(48)
    assert create(forty, query(merge=search.MERGE_MAX)) == _lib.EUNSUPPORTED
    assert create(forty, query(merge=search.MERGE_MIN)) == _lib.EUNSUPPORTED
    assert create(forty, query(merge=3)) == _lib.EINVAL
    with_excl = prep_n(20)
    with_excl[0].excluded = [5]
    assert create(with_excl) == _lib.EUNSUPPORTED
    assert create(forty, edit(term={7: 66})) == _lib.EUNSUPPORTED      # a frequency of 256
    assert create(forty, edit(term={7: 67})) == _lib.OK                # 255 fits
    assert create(forty, edit(c0={40: -1.0})) == _lib.EINVAL
    assert create(forty, edit(c0={40: float("nan")})) == _lib.EINVAL
    assert create(forty, edit(kind={40: 7})) == _lib.EINVAL
    assert create(forty, edit(kind={40: _lib.SCORE_BM25 | _lib.GROUP_ALT})) == _lib.EINVAL
    assert create(forty, edit(term={40: len(lists)})) == _lib.EINVAL
    assert create(forty, edit(term={40: _lib.NO_TERM})) == _lib.OK
    assert create(forty, edit(c0={40: 0.0})) == _lib.OK
    # more than 4 distinct scorer signatures in one query
    five = edit(norm_const={j: 0.3 + 0.1 * j for j in range(5)})
    four = edit(norm_const={j: 0.3 + 0.1 * j for j in range(3)})
    assert create(forty, five) == _lib.EUNSUPPORTED and create(forty, four) == _lib.OK
    # a phrase batch holds phrases only
    # an Or of 17 by_terms fails as it always did
    many = [Or([by_term(i) for i in range(_lib.MAX_TERMS + 1)])]
    with pytest.raises(_lib.IrsHipError) as e:
        sr.batch(search.prepare(many, BM25(), st), 10)
    assert e.value.status == _lib.EINVAL
    for bad in (by_terms([]), by_terms(list(range(65))), by_terms([1, 2], 0), by_terms([1, 2], 3)):
        with pytest.raises(ValueError):
            search.prepare([bad], BM25(), st)

    # refused on a batch with such a query, which afterwards still runs correctly
    flts = [by_terms(list(range(20)), 2), Or([by_term(1), by_term(2)]), by_terms([(3, 2.0), 4])]
    b = sr.batch(search.prepare(flts, BM25(), st), 10)
    assert b.wide_units() == 2
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
        check(flt, 10, h[q], c[q], t[q], *expected(seg, flt, BM25()))
    b.close()
    plain = sr.batch(search.prepare(flts[1:2], BM25(), st), 10)
    assert plain.wide_units() == 0
    plain.close()
    sr.close()


N_HAND = 2 * TILE + 5     # three tiles, the last one nearly empty
ALL = 5000                # the doc every term holds
BORDER = (TILE, TILE + 1, N_HAND)   # the last doc of tile 0, the first of tile 1, the last doc
T128, T129, TTAIL, TONE, TBIG, TEMPTY = 10, 11, 12, 13, 2, 63
ABSENT = 10_000


def hand_lists():
    """Term t holds the docs d with d % (5 + t) == t % 5, frequencies 1 + (7 d + t) % 5 — except
    T128 / T129 / TTAIL / TONE: exactly 128 / 129 / 50 / 1 postings, and TBIG, whose frequencies run up
    to 255 (the general score form next to the table rows).  Every term holds doc ALL; the even terms
    below 40 hold the docs at the tile border and the last doc."""
    N = N_HAND
    lists = []
    for t in range(64):
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
        if t % 2 == 0 and t < 40 and t not in (T128, TTAIL):
            docs.update(BORDER)
        d = np.array(sorted(docs), np.uint32)
        f = (1 + (7 * d + t) % 5).astype(np.uint32)
        if t == TBIG:
            f = (1 + d % 255).astype(np.uint32)
        lists.append((d, f))
    assert len(lists[T128][0]) == 128 and len(lists[T129][0]) == 129 and len(lists[TTAIL][0]) == 50
    assert len(lists[TONE][0]) == 1 and int(lists[TBIG][1].max()) == 255
    return lists


def hand_queries():
    """(filter, what it is about).  Entry boosts 0.25 .. 4, one of them 0."""
    def boost(j):
        return (0.25, 0.5, 1.0, 2.0, 4.0)[j % 5] if j != 5 else 0.0
    sixty4 = [(t, boost(t)) for t in range(63)] + [(0, 1.5)]          # all present, term 0 twice
    gaps = list(sixty4)
    gaps[20], gaps[21] = (ABSENT, 1.0), (TEMPTY, 1.0)                  # 62 present entries
    seventeen = [(t, boost(t)) for t in range(14)] + [(0, 1.5), (ABSENT, 1.0), (TEMPTY, 2.0)]   # 15 present
    out = []
    for mm in (1, 2, 32, 63, 64):
        out.append((by_terms(sixty4, mm), "64 entries, min_match %d" % mm))
    out.append((by_terms(gaps, 1, boost=0.5), "62 of 64 present"))
    out.append((by_terms(gaps, 62), "62 of 64 present: their conjunction"))
    out.append((by_terms(gaps, 63), "too few present"))
    for mm in (1, 2, 8, 15, 16, 17):
        out.append((by_terms(seventeen, mm), "17 entries, min_match %d" % mm))
    out.append((by_terms([TONE, T128, T129, TTAIL] + list(range(20, 34)), 1), "the short lists"))
    return out


def case_lists(L, layout):
    lists = hand_lists()
    N = N_HAND
    norms = (np.arange(N, dtype=np.uint32) * 7 % 200 + 20).astype(np.uint8)
    seg = synth.segment_from_lists(lists, N, layout, norms=norms)
    seg.metas[TEMPTY]["docs_count"] = 0       # an ordinal whose range is empty here
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    cases = hand_queries()
    filters = [f for f, _ in cases]
    holders = {d: sum(int(d in set(lists[t][0].tolist())) for t in range(63)) for d in (ALL,) + BORDER}
    assert holders[ALL] == 63 and all(holders[d] >= 18 for d in BORDER)
    for scorer in (TFIDF(True), BM25(), BM25(0.0, 0.0)):
        exp = [expected(seg, f, scorer) for f in filters]
        # what the lists say: every term holds ALL (count 64 with term 0 twice), so the 64-entry
        # conjunction is that doc; 62 present entries cannot reach min_match 63
        assert set(np.nonzero(exp[4][1])[0].tolist()) == {ALL}
        assert ALL in set(np.nonzero(exp[6][1])[0].tolist()) and not exp[7][1].any()
        assert not exp[13][1].any() and exp[12][1].any() is not None
        assert all(exp[0][1][d] and exp[8][1][d] for d in BORDER)
        n_all = int(exp[0][1].sum())
        for k in (1, 10, 4096):
            h, c, t, info = _run(sr, filters, scorer, k, st)
            assert info["wide"] == len(filters)
            for q, flt in enumerate(filters):
                check(flt, k, h[q], c[q], t[q], *exp[q])
            assert int(t[0]) == n_all and int(t[4]) == 1 and int(t[7]) == 0
            if k == 4096:
                assert int(h[4, 0]["doc"]) == ALL
    # every score ties (BM1 with zero boosts): the candidates overflow a small buffer; exact re-run
    ties = [by_terms([(t, 0.0) for t in range(17)], 1), by_terms([(t, 0.0) for t in range(40)], 2), filters[0]]
    h, c, t, info = _run(sr, ties, BM25(0.0, 0.0), 64, st, cand_cap=64)
    assert info["reruns"] > 0
    for q, flt in enumerate(ties):
        sc, m = expected(seg, flt, BM25(0.0, 0.0))
        check(flt, 64, h[q], c[q], t[q], sc, m)
        if q < 2:
            assert (h[q, :64]["score"] == 0).all()
            assert np.array_equal(h[q, :64]["doc"], np.nonzero(m)[0][:64])
    sr.close()
    # deleted docs, a border doc and the doc of the conjunction among them
    seg2 = synth.segment_from_lists(lists, N, layout, norms=norms)
    seg2.doc_mask = np.array([7, TILE, ALL, N], np.uint32)
    sr2 = search.SegmentReader.from_synth(seg2, L=L)
    st2 = [parity.segment_stats(seg2)]
    for scorer in (BM25(), TFIDF(True)):
        sub = [filters[0], filters[1], filters[4], filters[8]]
        h, c, t, _ = _run(sr2, sub, scorer, 100, st2)
        for q, flt in enumerate(sub):
            sc, m = expected(seg2, flt, scorer)
            assert not m[[7, TILE, ALL, N]].any()
            check(flt, 100, h[q], c[q], t[q], sc, m)
        assert int(t[2]) == 0 and int(t[0]) == int(expected(seg, filters[0], scorer)[1].sum()) - 4
    sr2.close()


def random_filters(max_rank, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        nt = int(rng.integers(17, 65))
        terms = rng.choice(max_rank, nt, replace=False)
        boosts = rng.choice([0.25, 0.5, 1.0, 1.0, 2.0, 4.0], nt)
        mm = 1 if i % 3 == 0 else int(rng.integers(1, 5)) if i % 3 == 1 else int(rng.integers(2, nt // 4))
        out.append(by_terms([(int(t), float(b)) for t, b in zip(terms, boosts)], mm))
    return out


def float64_sums(seg, flt, scorer):
    """A float64 sum of the float32 scores the oracle gives every posting: one term at a time."""
    total = np.zeros(seg.num_docs + 1, np.float64)
    for t, b in entries(flt):
        one = by_terms([(t, float(b))], 1)
        sc, m = expected(seg, one, scorer)
        total += np.where(m, sc, 0).astype(np.float64)
    return total


PARITY_SEED = 3


def case_parity(L, num_docs, max_rank, layout, n_queries=24, seed=PARITY_SEED):
    seg = synth.build_segment(num_docs, max_rank, layout=layout)
    seg.doc_mask = np.arange(9, num_docs, 101, dtype=np.uint32)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    filters = random_filters(max_rank, n_queries, seed)
    for scorer in (BM25(), TFIDF(True)):
        exp = [expected(seg, f, scorer) for f in filters]
        exact = [float64_sums(seg, f, scorer) for f in filters]
        for k in (64, 128):
            h, c, t, info = _run(sr, filters, scorer, k, st)
            assert info["wide"] == n_queries
            for q, flt in enumerate(filters):
                # the precondition: for the docs compared, float32 summation in the oracle's order
                # is within REL_TOL / 4 of the float64 sum — a failure below points at the kernel
                docs = h[q, :int(c[q])]["doc"].astype(np.int64)
                ref = exp[q][0][docs].astype(np.float64)
                err = np.abs(ref - exact[q][docs]) / np.maximum(exact[q][docs], 1e-30)
                assert docs.size == 0 or err.max() < parity.REL_TOL / 4, ("precondition", q, float(err.max()))
                check(flt, k, h[q], c[q], t[q], *exp[q])
    sr.close()


def case_mixed(L, num_docs, max_rank, layout):
    """Wide queries interleaved with ordinary ones: the ordinary ones are bit for bit what a batch
    without the wide ones gives, on the same path; the wide ones equal a batch of their own."""
    seg = synth.build_segment(num_docs, max_rank, layout=layout)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    rng = np.random.default_rng(17)
    wide = random_filters(max_rank, 4, 23)
    ordinary = [Or([by_term(int(t)) for t in rng.choice(max_rank, 8, replace=False)]) for _ in range(3)]
    ordinary += [And([by_term(int(t)) for t in rng.choice(16, 3, replace=False)]) for _ in range(2)]
    ordinary += [Or([by_term(int(t)) for t in rng.choice(24, 6, replace=False)], min_match=2)]
    ordinary += [Or([by_term(0), by_term(1)])]       # upper / min_score is small
    mixed = [wide[0], ordinary[0], ordinary[3], wide[1], ordinary[1], ordinary[5], ordinary[6], wide[2],
             ordinary[2], ordinary[4], wide[3]]
    at_w = [mixed.index(f) for f in wide]
    at_o = [mixed.index(f) for f in ordinary]
    for scorer in (BM25(), TFIDF(True)):
        for path in (None, _lib.PATH_JOINED, _lib.PATH_ITEMS):
            hm, cm, tm, im = _run(sr, mixed, scorer, 50, st, path=path)
            ho, co, to, io = _run(sr, ordinary, scorer, 50, st, path=path)
            hw, cw, tw, iw = _run(sr, wide, scorer, 50, st, path=path)
            assert im["wide"] == 4 and io["wide"] == 0 and iw["wide"] == 4
            assert im["path"] == io["path"] and im["paired"] == io["paired"], (path, im, io)
            assert np.array_equal(hm[at_o], ho) and np.array_equal(cm[at_o], co) and np.array_equal(tm[at_o], to)
            assert np.array_equal(hm[at_w], hw) and np.array_equal(cm[at_w], cw) and np.array_equal(tm[at_w], tw)
            for q, flt in enumerate(mixed):
                if isinstance(flt, by_terms):
                    check(flt, 50, hm[q], cm[q], tm[q], *expected(seg, flt, scorer))
        parity.check_single_segment(seg, ordinary, scorer, 50, ho, co, to)
    sr.close()


def case_multi(L, sizes, max_rank=96, k=50):
    """create_multi: a term absent from one segment, statistics over all segments, units indexed
    segment * n_queries + query, the merged top k against the oracle's own harness run."""
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    segs = [synth.build_segment(int(n), max_rank, first_doc=int(f)) for n, f in zip(sizes, first)]
    segs[1].metas[5]["docs_count"] = 0
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    stats = [parity.segment_stats(s) for s in segs]
    filters = random_filters(max_rank, 5, 41)
    filters.append(by_terms([5] + list(range(20, 40)), 1))
    filters.append(by_terms([(5, 2.0)] + [(t, 1.0) for t in range(40, 60)], 3))
    filters.append(by_terms([5, max_rank + 7], 2))     # segment 1 holds neither, the others one of them
    for scorer in (BM25(), TFIDF(True)):
        prep = search.prepare(filters, scorer, stats)
        dwf = sum(s.docs_with_field for s in segs)
        ttf = sum(s.total_term_freq for s in segs)
        dwt5 = sum(int(s.metas[5]["docs_count"]) for s in segs)
        assert prep[5].scorers[0] == scorer.term_scorer(scorer.collect(dwf, dwt5, ttf), 1.0)
        b = search.QueryBatch(readers, prep, k)
        assert b.wide_units() == len(filters) * len(segs)
        b.set_shared_threshold(True)       # (leaves every wide unit a threshold of its own)
        h, c, t = b.run().results()
        assert h.shape[:2] == (len(segs), len(filters))
        for i, s in enumerate(segs):
            for q, flt in enumerate(filters):
                check(flt, k, h[i, q], c[i, q], t[i, q], *expected(s, flt, scorer, segs))
        assert not t[:, 7].any()
        merged = search.merge_topk_host([(h[i], c[i]) for i in range(len(segs))], k)
        for q, flt in enumerate(filters):
            ent = entries(flt)
            terms = [x for x, _ in ent]
            metas = np.stack([parity.metas_for(s, terms) for s in segs])
            ref, total = oracle.search([parity.oracle_view(s) for s in segs], metas, oracle_op(flt),
                                       parity.oracle_scorer(scorer), k, [x for _, x in ent])
            assert int(t[:, q].sum()) == int(total), q
            got = np.array([r[0] for r in merged[q]])
            assert len(got) == len(ref), (q, len(got), len(ref))
            assert np.allclose(got, ref["score"], rtol=parity.REL_TOL, atol=0), q
        b.close()
    for r in readers:
        r.close()


def case_streams(L, num_docs, max_rank):
    """The wide units' terms are streams of the batch's one set: shared with an ordinary query,
    served by the device's stream cache, the same results without it."""
    seg = synth.build_segment(num_docs, max_rank)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    wide = by_terms(list(range(4, 30)), 1)
    plain = Or([by_term(t) for t in (2, 3, 4, 5, 6, 7)])
    flts = [wide, plain]
    search.set_stream_cache(0, L=L)
    try:
        h0, c0, t0, i0 = _run(sr, flts, BM25(), 20, st, path=_lib.PATH_JOINED)
        assert i0["path"] == _lib.PATH_JOINED
        assert i0["streams"] == (28, 28), i0       # terms 2 .. 29: the union, all decoded by the run
        hw, cw, tw, iw = _run(sr, [wide], BM25(), 20, st)
        assert iw["streams"] == (26, 26) and iw["path"] == _lib.PATH_ITEMS
        search.set_stream_cache(64 << 20, L=L)
        h1, c1, t1, i1 = _run(sr, flts, BM25(), 20, st, path=_lib.PATH_JOINED)
        h2, c2, t2, i2 = _run(sr, flts, BM25(), 20, st, path=_lib.PATH_JOINED)
        assert i1["streams"] == (28, 28) and i2["streams"] == (28, 0), (i1, i2)
        for h, c, t in ((h1, c1, t1), (h2, c2, t2)):
            assert np.array_equal(h, h0) and np.array_equal(c, c0) and np.array_equal(t, t0)
        assert np.array_equal(hw[0], h0[0])
        check(wide, 20, h0[0], c0[0], t0[0], *expected(seg, wide, BM25()))
    finally:
        search.set_stream_cache(0, L=L)
        L.irs_hip_device_trim(0)
    sr.close()


def expansion_visits(segs, n_visited=300):
    """Two filters whose visitors yield 300 terms of every segment (ascending ordinals)."""
    n = min(len(s.metas) for s in segs)
    a = np.arange(n - n_visited, n, dtype=np.uint32)
    b = np.arange(40, 40 + 2 * n_visited, 2, dtype=np.uint32)
    return [[a for _ in segs], [b for _ in segs]]


def case_expansions(L, sizes, max_rank):
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    segs = [synth.build_segment(int(n), max_rank, first_doc=int(f)) for n, f in zip(sizes, first)]
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    stats = [parity.segment_stats(s) for s in segs]
    visits = expansion_visits(segs)
    for scorer in (BM25(), TFIDF(True)):
        prep = search.prepare_expansions(visits, 50, scorer, stats)
        assert all(16 < len(p.scored) <= 50 for p in prep)
        arr = search.expansion_arrays(readers, prep, 20)
        assert (arr.queries["op"] == _lib.OP_MULTITERM).all() and (arr.queries["min_match"] == 1).all()
        h, c, t = search.execute_expansions(readers, prep, 20)
        parity.check_expansions(segs, visits, 50, scorer, 20, h, c, t)
    for r in readers:
        r.close()


def test_expansion_arrays_unchanged_at_16():
    """Limit 16 on the same visit: the arrays are what they were — an Or per filter."""
    stats = [search.SegmentStats(5000, 400_000, (np.arange(700, dtype=np.int64) * 37 % 911) + 3),
             search.SegmentStats(3000, 250_000, (np.arange(700, dtype=np.int64) * 53 % 877) + 2)]
    segs = [type("S", (), {"metas": np.zeros(700)})() for _ in stats]
    visits = expansion_visits(segs)
    prep = search.prepare_expansions(visits, 16, BM25(), stats)
    arr = search.expansion_arrays(segs, prep, 10)
    assert all(0 < len(p.scored) <= 16 for p in prep)
    assert (arr.queries["op"] == _lib.OP_OR).all() and (arr.queries["merge"] == search.MERGE_SUM).all()
    assert arr.queries["n_terms"].tolist() == [len(p.scored) for p in prep]
    assert arr.queries["first_term"].tolist() == [0, len(prep[0].scored)]
    for q, p in enumerate(prep):
        lo = int(arr.queries["first_term"][q])
        for s in range(2):
            want = [t if t in p.scored_in[s] else _lib.NO_TERM for t in p.scored]
            assert arr.terms[s, lo:lo + len(p.scored)]["term"].tolist() == want
        assert np.array_equal(arr.terms[0, lo:lo + len(p.scored)]["c0"], p.c0)
    wide = search.expansion_arrays(segs, search.prepare_expansions(visits, 50, BM25(), stats), 10)
    assert (wide.queries["op"] == _lib.OP_MULTITERM).all()
    # (a limit above 64 is not taken: the Or of all its slots that batch create always refused)
    over = search.expansion_arrays(segs, search.prepare_expansions(visits, 65, BM25(), stats), 10)
    assert (over.queries["op"] == _lib.OP_OR).all() and int(over.queries["n_terms"].max()) == 65


def test_prepare_by_terms():
    st = [search.SegmentStats(1000, 100_000, np.arange(64, dtype=np.int64) * 3 + 20),
          search.SegmentStats(500, 40_000, np.arange(32, dtype=np.int64) * 2 + 1)]
    sc = BM25()
    flt = by_terms([7, (9, 2.0), (40, 0.5), 7], min_match=2, boost=1.5)
    p = search.prepare([flt], sc, st)[0]
    assert p.op == _lib.OP_MULTITERM and p.terms == [7, 9, 40, 7] and p.min_match == 2
    # statistics as for an Or of by_terms: the field's over all segments, the term's where it exists
    as_or = search.prepare([Or([by_term(7), by_term(9, 2.0), by_term(40, 0.5), by_term(7)], boost=1.5)], sc, st)[0]
    assert p.scorers == as_or.scorers
    want = sc.term_scorer(sc.collect(1500, int(st[0].docs_count[40]), 140_000), f32(f32(1.5) * f32(0.5)))
    assert p.scorers[2] == want
    segs = [type("S", (), {"metas": np.zeros(n)})() for n in (64, 32)]
    arr = search.QueryArrays.from_prepared(segs, [p], 10)
    assert tuple(arr.queries[0]) == (_lib.OP_MULTITERM, 4, 0, 10, 2, search.MERGE_SUM)
    assert arr.terms[1, :4]["term"].tolist() == [7, 9, _lib.NO_TERM, 7]
    fast = search.prepare_filters([flt, Or([by_term(1), by_term(2)])], sc, st, segs, 10)
    assert np.array_equal(fast.queries[:1], arr.queries) and np.array_equal(fast.terms[:, :4], arr.terms)
    assert search.replace(flt, min_match=1).min_match == 1


def _cpp(L, tmp_path, extra=()):
    """tests/cpp/test_multiterm.cpp: the C++ layer's scored multi-term filter."""
    import subprocess
    from pathlib import Path
    from iresearch_amd import _build
    root = Path(__file__).resolve().parents[1]
    synth_lib = _build.build_synth()
    exe = tmp_path / "test_multiterm"
    lib = Path(L._name)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall",
           "-I", str(root / "include"), "-I", str(root / "iresearch_amd" / "cpp"),
           "-I", str(root / "iresearch_amd" / "index"), "-I", str(root / "oracle"),
           str(root / "tests" / "cpp" / "test_multiterm.cpp"), "-o", str(exe), str(lib), str(synth_lib),
           str(oracle.build()), "-pthread", "-Wl,-rpath," + str(lib.parent),
           "-Wl,-rpath," + str(Path(synth_lib).parent), "-Wl,-rpath," + str(root / "oracle"), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "test_multiterm OK" in run.stdout, (run.stdout + run.stderr)[-3000:]


# ---------------------------------------------------------------- emulator --

def test_multiterm_abi_emulated(simlib):
    case_abi(simlib)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_multiterm_lists_emulated(simlib, layout):
    case_lists(simlib, layout)


def test_multiterm_parity_emulated(simlib):
    case_parity(simlib, 30_000, 128, synth.LAYOUT_SIMD4)


def test_multiterm_mixed_emulated(simlib):
    case_mixed(simlib, 26_000, 96, synth.LAYOUT_SIMD4)


def test_multiterm_multi_emulated(simlib):
    case_multi(simlib, (3_000, 1_500, 4_000))


def test_multiterm_streams_emulated(simlib):
    case_streams(simlib, 14_000, 64)


def test_multiterm_expansions_emulated(simlib):
    case_expansions(simlib, (6_000, 4_000), 700)


def test_cpp_multiterm_emulated(simlib, tmp_path):
    _cpp(simlib, tmp_path)


# --------------------------------------------------------------------- GPU --

@pytest.mark.gpu
def test_multiterm_abi_gpu(gpulib):
    case_abi(gpulib)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_multiterm_lists_gpu(gpulib, layout):
    case_lists(gpulib, layout)


@pytest.mark.gpu
def test_multiterm_parity_gpu(gpulib):
    case_parity(gpulib, 60_000, 128, synth.LAYOUT_SIMD4)


@pytest.mark.gpu
def test_multiterm_mixed_gpu(gpulib):
    case_mixed(gpulib, 60_000, 128, synth.LAYOUT_SIMD4)


@pytest.mark.gpu
def test_multiterm_multi_gpu(gpulib):
    case_multi(gpulib, (30_000, 10_000, 45_000), max_rank=128, k=100)


@pytest.mark.gpu
def test_multiterm_streams_gpu(gpulib):
    case_streams(gpulib, 60_000, 128)


@pytest.mark.gpu
def test_multiterm_expansions_gpu(gpulib):
    case_expansions(gpulib, (30_000, 20_000), 700)


@pytest.mark.gpu
def test_cpp_multiterm_gpu(gpulib, tmp_path):
    rocm = "/opt/rocm/lib"
    _cpp(gpulib, tmp_path, ["-Wl,-rpath," + rocm, "-Wl,-rpath-link," + rocm, "-Wl,--allow-shlib-undefined"])
