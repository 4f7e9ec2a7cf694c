"""And([by_phrase, by_term...]) — a phrase plus required terms (IRS_HIP_PHRASE_REQUIRED): the
reference's Conjunction over {PhraseIterator, term iterators} (boolean_filter.cpp:150-210,
boolean_query.cpp:60-145, conjunction.hpp:436-490).

The expected value is composed from the oracle as it stands: oracle.score_all_phrase gives the
phrase frequency and phrase score of every doc, oracle.score_all with OP_AND over the required terms
their conjunction and summed scores (boosts passed); a doc matches when pf > 0 and the terms hold it,
its score is the float32 sum of the two.  Deleted docs go through the segment's doc_mask (both oracle
calls apply it), excluded terms through the oracle's decoder.  One body runs on the emulator (CPU
tier) and on the GPU at a larger size."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle
import parity
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, TFIDF, And, Not, Or, by_phrase, by_term

f32 = np.float32


# ------------------------------------------------------------- expectations --

def split(flt):
    """(phrase, required by_terms, excluded term ordinals, And boost) of a filter of this file: a
    by_phrase alone, or an And of one by_phrase, by_terms and Not(by_term)s."""
    if isinstance(flt, by_phrase):
        return flt, [], [], 1.0
    ph = [s for s in flt.subs if isinstance(s, by_phrase)]
    assert len(ph) == 1
    return (ph[0], [s for s in flt.subs if isinstance(s, by_term)],
            [s.filter.term for s in flt.subs if isinstance(s, Not)], flt.boost)


def _present(seg, t):
    return 0 <= t < len(seg.metas) and int(seg.metas[t]["docs_count"]) > 0


def expected(seg, flt, scorer, all_segs=None):
    """(scores f32[num_docs + 1], matched bool[num_docs + 1]) of `flt` on `seg`; statistics over
    `all_segs` (default: this segment)."""
    all_segs = all_segs or [seg]
    ph, req, excl, mult = split(flt)
    osc = parity.oracle_scorer(scorer)
    view = parity.oracle_view(seg)
    dwf = sum(s.docs_with_field for s in all_segs)
    ttf = sum(s.total_term_freq for s in all_segs)
    n1 = seg.num_docs + 1
    terms = list(ph.terms) + [s.term for s in req]
    if not all(_present(seg, t) for t in terms):   # an absent word or required term: nothing
        return np.zeros(n1, f32), np.zeros(n1, bool)

    def dwt(ts):
        return [sum(int(s.metas[t]["docs_count"]) if 0 <= t < len(s.metas) else 0 for s in all_segs)
                for t in ts]
    sc, pf = oracle.score_all_phrase(view, parity.metas_for(seg, ph.terms), ph.offsets, osc, dwf,
                                     dwt(ph.terms), ttf, float(f32(f32(mult) * f32(ph.boost))))
    matched = pf[:n1] > 0
    scores = sc[:n1].astype(f32)
    if req:
        rt = [s.term for s in req]
        boosts = [f32(f32(mult) * f32(s.boost)) for s in req]
        ts, tm = oracle.score_all(view, parity.metas_for(seg, rt), oracle.OP_AND, osc, dwf, dwt(rt),
                                  ttf, boosts)
        matched = matched & tm[:n1].astype(bool)
        scores = (scores + ts[:n1].astype(f32)).astype(f32)
    wc = int(getattr(seg, "wand_count", 0))
    for t in excl:
        if _present(seg, t):
            d, _ = oracle.decode_term(seg.doc_file, seg.metas[t], seg.layout, wand_count=wc)
            matched[d.astype(np.int64)] = False
    scores[~matched] = 0
    return scores, matched


def check(flt, k, h, c, t, scores, matched):
    """As check() of test_variadic_phrase.py: total hits and doc sets exactly, scores to REL_TOL,
    order (score descending, doc ascending), membership above the k-th score."""
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


def _run(sr, filters, scorer, k, stats):
    prep = search.prepare(filters, scorer, stats, required_terms=True)
    b = sr.batch(prep, k)
    h, c, t = (x.copy() for x in b.run().results())
    b.close()
    return prep, h, c, t


# -------------------------------------------------------------------- cases --

def case_abi(L):
    """IRS_HIP_PHRASE_REQUIRED validation at batch create, absent required terms, and a plain
    phrase next to a unit with required terms."""
    num_docs = 3000
    rng = np.random.default_rng(5)
    lists = []
    for t in range(24):
        docs = np.unique(rng.choice(num_docs, 900, replace=False) + 1).astype(np.uint32)
        freqs = np.ones(docs.size, np.uint32) * 2
        pos = np.concatenate([np.sort(rng.choice(6, 2, replace=False)) + 1 for _ in docs]).astype(np.uint32)
        lists.append((docs, freqs, pos))
    seg = synth.segment_from_lists(lists, num_docs, synth.LAYOUT_SIMD4)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]

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

    R = _lib.PHRASE_REQUIRED
    good = search.prepare([And([by_phrase([1, 2, 3]), by_term(4), by_term(5, 2.0)])], BM25(), st, required_terms=True)
    assert good[0].required == [False, False, False, True, True]
    assert create(good) == _lib.OK
    kinds = search.QueryArrays.from_prepared([sr], good, 10).terms[0, :5]["kind"]
    assert list(kinds) == [_lib.SCORE_BM25] * 3 + [_lib.SCORE_BM25 | R] * 2

    def edit(**kw):
        def f(arr):
            for name, changes in kw.items():
                for j, v in changes.items():
                    arr.terms[0, j][name] = v
        return f
    B = _lib.SCORE_BM25
    # a required entry in front of a phrase entry
    assert create(good, edit(kind={2: B | R, 3: B})) == _lib.EINVAL    # w w R w R
    assert create(good, edit(kind={0: B | R})) == _lib.EINVAL          # R w w R R
    # fewer than 2 phrase entries in front of the first required one
    assert create(good, edit(kind={1: B | R, 2: B | R})) == _lib.EINVAL   # w R R R R
    # the flag outside a phrase
    for op in (_lib.OP_OR, _lib.OP_AND, _lib.OP_MINMATCH):
        def other_op(arr, op=op):
            arr.queries[0]["op"] = op
            arr.queries[0]["min_match"] = 2
        assert create(good, other_op) == _lib.EINVAL, op
    # ... and on an excluded entry
    with_not = search.prepare([And([by_phrase([1, 2]), by_term(4), Not(by_term(6))])], BM25(), st, required_terms=True)
    assert create(with_not) == _lib.OK
    assert create(with_not, edit(kind={3: _lib.EXCLUDE | R})) == _lib.EINVAL
    # its own scorer values, validated like a by_term's; the phrase offset ignored
    assert create(good, edit(c0={3: -1.0})) == _lib.EINVAL
    assert create(good, edit(c0={4: float("nan")})) == _lib.EINVAL
    assert create(good, edit(kind={3: 7 | R})) == _lib.EINVAL
    assert create(good, edit(kind={3: _lib.SCORE_TFIDF | R})) == _lib.OK
    assert create(good, edit(term={3: len(lists)})) == _lib.EINVAL
    assert create(good, edit(phrase_offset={3: 77, 4: 5})) == _lib.OK
    # the phrase's words still carry ONE scorer
    assert create(good, edit(c0={1: 0.5})) == _lib.EINVAL
    # merge stays SUM
    def merge_max(arr):
        arr.queries[0]["merge"] = search.MERGE_MAX
    assert create(good, merge_max) == _lib.EINVAL
    # 8 entries are fine, 9 are not supported
    eight = search.prepare([And([by_phrase([1, 2, 3])] + [by_term(t) for t in range(4, 9)])], BM25(), st, required_terms=True)
    assert create(eight) == _lib.OK
    nine = search.prepare([And([by_phrase([1, 2, 3])] + [by_term(t) for t in range(4, 9)])], BM25(), st, required_terms=True)
    nine[0].terms.append(9)
    nine[0].scorers.append(nine[0].scorers[-1])
    nine[0].offsets.append(0)
    nine[0].required.append(True)
    assert create(nine) == _lib.EUNSUPPORTED
    # a variadic part and required terms in one unit; variadic units next to units with required terms
    both = search.prepare([by_phrase([[1, 2], 3])], BM25(), st, required_terms=True)
    both[0].terms.append(4)
    both[0].scorers.append(both[0].scorers[0])
    both[0].offsets.append(0)
    both[0].alts.append(False)
    both[0].required = [False, False, False, True]
    assert create(both) == _lib.EUNSUPPORTED
    mixed = search.prepare([by_phrase([[1, 2], 3]), And([by_phrase([1, 2]), by_term(4)])], BM25(), st, required_terms=True)
    assert create(mixed) == _lib.EUNSUPPORTED
    assert create(mixed[::-1]) == _lib.EUNSUPPORTED

    # an absent required term empties the unit; a plain phrase in the batch is what it is alone
    flts = [And([by_phrase([1, 3]), by_term(4)]), And([by_phrase([1, 3]), by_term(10_000)]),
            by_phrase([1, 3]), And([by_phrase([1, 3]), by_term(4), by_term(7)]), by_phrase([2, 5, 1], [0, 1, 3]),
            by_phrase([6])]
    for scorer in (BM25(), TFIDF(True)):
        prep, h, c, t = _run(sr, flts, scorer, 10, st)
        for q, flt in enumerate(flts):
            check(flt, 10, h[q], c[q], t[q], *expected(seg, flt, scorer))
        assert int(t[1]) == 0 and int(c[1]) == 0
        assert int(t[0]) > 0 and int(t[2]) > int(t[0]) > int(t[3])
        _, h1, c1, t1 = _run(sr, [flts[2], flts[4], flts[5]], scorer, 10, st)
        assert int(t[5]) == 900
        for a, b in ((2, 0), (4, 1), (5, 2)):
            assert np.array_equal(h[a], h1[b]) and c[a] == c1[b] and t[a] == t1[b], (scorer, a)
    # the ignored phrase offset changes nothing
    arr = search.QueryArrays.from_prepared([sr], search.prepare(flts, BM25(), st, required_terms=True), 10)
    b0 = search.QueryBatch(sr, arr)
    ref = [x.copy() for x in b0.run().results()]
    b0.close()
    arr.terms[0, 2]["phrase_offset"] = 9
    b1 = search.QueryBatch(sr, arr)
    got = b1.run().results()
    assert all(np.array_equal(x, y) for x, y in zip(ref, got))
    b1.close()
    sr.close()


N_LISTS = 12_000
(NEW, YORK, HOTEL, THE, ONE_HIT, ONE_MISS, L127, L128, L129, L257, NINES, RARE, CITY) = range(13)


def hand_lists():
    """term -> (docs, freqs, positions), every list a rule of arithmetic on the doc id so that the
    matches can be written down: "new york" is in d % 12 == 0 (twice in d % 24 == 0); d % 6 == 0 has
    both words, but york 3 positions late unless d % 4 == 0."""
    N = N_LISTS
    T = {
        NEW: {d: [1, 10] for d in range(3, N + 1, 3)},
        YORK: {d: ([2, 11] if d % 24 == 0 else [2] if d % 4 == 0 else [5]) for d in range(2, N + 1, 2)},
        HOTEL: {d: list(range(30, 31 + d % 3)) for d in range(5, N + 1, 5)},       # 2400 docs, tf 1..3
        THE: {d: [20] for d in range(1, N + 1)},                                   # every doc: 93 blocks + tail
        ONE_HIT: {120: [40]},
        ONE_MISS: {7: [40]},
        L127: {6 * i: [40] for i in range(1, 128)},                                # tail only
        L128: {6 * i: [40] for i in range(1, 129)},                                # one block, no tail
        L129: {6 * i: [40] for i in range(1, 130)},                                # block + 1
        L257: {12 * i: [40, 41] for i in range(1, 258)},                           # 2 blocks + 1, 1536 ids per block
        NINES: {9 * i: [40] for i in range(1, 301)},                               # 1152 ids per block
        RARE: {90 * i: [40] for i in range(1, 134)},                               # one block over 11 520 ids + 5
        CITY: {d: ([3] if d % 36 == 0 else [7]) for d in range(12, N + 1, 12)},
    }
    lists = []
    for t in range(len(T)):
        items = sorted(T[t].items())
        lists.append((np.array([d for d, _ in items], np.uint32),
                      np.array([len(p) for _, p in items], np.uint32),
                      np.array([x for _, p in items for x in p], np.uint32)))
    return lists


def case_lists(L, layout):
    """Hand-built lists: the matching docs of every query written down from the rules of
    hand_lists(), the scores from the oracle."""
    N = N_LISTS
    lists = hand_lists()
    norms = (np.arange(N, dtype=np.uint32) * 7 % 200 + 20).astype(np.uint8)
    seg = synth.segment_from_lists(lists, N, layout, norms=norms)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    ny = by_phrase([NEW, YORK])
    docs = range(1, N + 1)
    phrase = {d for d in docs if d % 12 == 0}
    cases = [
        # (a) + (b): d % 30 == 0 holds new, york and hotel, the phrase only where d % 4 == 0; and
        # d % 12 == 0 without d % 5 == 0 has the phrase and no hotel.  (c): hotel (2400) leads
        (And([ny, by_term(HOTEL)]), {d for d in docs if d % 60 == 0}),
        # (d) + (j): "new" (4000) leads, the required term holds every doc; 1000 matches
        (And([by_term(THE), ny]), phrase),
        # (c) single-doc lists as the lead: one inside the phrase's docs, one outside
        (And([ny, by_term(ONE_HIT)]), {120}),
        (And([ny, by_term(ONE_MISS)]), set()),
        # (e) 127 / 128 / 129 postings at 6 i: the even i; 257 at 12 i: all of them; (f) these lead
        # blocks span 768 (s = 0), 1536 and 1152 doc ids (s > 0)
        (And([ny, by_term(L127)]), {6 * i for i in range(2, 128, 2)}),
        (And([ny, by_term(L128)]), {6 * i for i in range(2, 129, 2)}),
        (And([ny, by_term(L129)]), {6 * i for i in range(2, 130, 2)}),
        (And([ny, by_term(L257)]), {12 * i for i in range(1, 258)}),
        (And([ny, by_term(NINES)]), {9 * i for i in range(4, 301, 4)}),
        # (g) the lead block of RARE covers 11 520 doc ids: 90 directory entries of THE (a second
        # trip of the directory loop), 30 of "new", 45 of "york"; matches: 90 i with i even
        (And([ny, by_term(RARE), by_term(THE)]), {90 * i for i in range(2, 134, 2)}),
        # (h) york as a phrase word and as a required term
        (And([ny, by_term(YORK, 0.5)], boost=2.0), phrase),
        # (i) 3 entries are above; 8 entries: 3 phrase words + 5 required.  "new york city": d % 36
        # == 0; with hotel, the, york, rare (d % 180 == 0) and L257 (d <= 3084): 180 .. 3060
        (And([by_phrase([NEW, YORK, CITY]), by_term(HOTEL), by_term(THE), by_term(YORK), by_term(RARE),
              by_term(L257)]), set(range(180, 3085, 180))),
        (And([by_phrase([NEW, YORK, CITY]), by_term(NINES)]), {d for d in docs if d % 36 == 0 and d <= 2700}),
        # the phrase with a gap: new .. .. .. york@5 where d % 6 == 0 and d % 4 != 0 (york at 5, new at 1)
        (And([by_phrase([NEW, YORK], [0, 4]), by_term(HOTEL)]), {d for d in docs if d % 30 == 0 and d % 4 != 0}),
        (ny, phrase),
    ]
    filters = [f for f, _ in cases]
    assert len(cases[11][1]) == 17
    for scorer in (BM25(), TFIDF(True)):
        exp = [expected(seg, f, scorer) for f in filters]
        for (flt, want), (_, matched) in zip(cases, exp):
            assert set(np.nonzero(matched)[0].tolist()) == want, ("the oracle and the hand list differ", flt)
        for k in (1, 3, 1000):
            prep, h, c, t = _run(sr, filters, scorer, k, st)
            for q, (flt, want) in enumerate(cases):
                assert int(t[q]) == len(want), (flt, int(t[q]), len(want))
                if k == 1000:
                    assert set(h[q, :int(c[q])]["doc"].tolist()) == want, flt
                check(flt, k, h[q], c[q], t[q], *exp[q])
    # the phrase frequency is the scorer's tf: d % 24 == 0 holds the phrase twice
    prep, h, c, t = _run(sr, [And([ny, by_term(THE)])], TFIDF(False), 1000, st)
    by_doc = {int(x["doc"]): float(x["score"]) for x in h[0, :int(c[0])]}
    assert by_doc[24] > by_doc[12] and abs(by_doc[24] - by_doc[48]) <= 1e-6 * by_doc[24]
    # (k) deleted docs and a Not next to the phrase and the term
    seg2 = synth.segment_from_lists(lists, N, layout, norms=norms)
    seg2.doc_mask = np.array([7, 60, 1800], np.uint32)
    sr2 = search.SegmentReader.from_synth(seg2, L=L)
    flt = And([ny, by_term(HOTEL), Not(by_term(RARE))])
    want = {d for d in docs if d % 60 == 0 and d % 90 != 0} - {60, 1800}
    for scorer in (BM25(), TFIDF(True)):
        sc, matched = expected(seg2, flt, scorer)
        assert set(np.nonzero(matched)[0].tolist()) == want
        for k in (1, 1000):
            prep, h, c, t = _run(sr2, [flt, And([ny, by_term(HOTEL)])], scorer, k, st)
            assert prep[0].excluded == [RARE]
            check(flt, k, h[0], c[0], t[0], sc, matched)
            check(flt, k, h[1], c[1], t[1], *expected(seg2, And([ny, by_term(HOTEL)]), scorer))
            assert int(t[1]) == len({d for d in docs if d % 60 == 0}) - 2
    sr.close()
    sr2.close()


def random_queries(seg, max_rank, n, seed):
    """2-4 phrase words, offsets with gaps, 1-3 required terms from frequent and from rare ranks.
    -> (filters, [True where a required term is the lead])"""
    rng = np.random.default_rng(seed)
    out, req_leads = [], []
    dc = seg.metas["docs_count"]
    for i in range(n):
        nw = int(rng.integers(2, 5))
        words = [int(x) for x in rng.integers(0, 10, nw)]    # (frequent words: phrases that occur)
        offs = [0]
        for _ in range(nw - 1):
            offs.append(offs[-1] + int(rng.integers(1, 3)))
        nr = int(rng.integers(1, 4))
        lo, hi = (0, 10) if i % 2 else (max_rank // 2, max_rank)     # frequent / rare
        req = [int(x) for x in rng.choice(np.arange(lo, hi), nr, replace=False)]
        subs = [by_phrase(words, offs, boost=1.0 if i % 5 else 1.5)] + [by_term(t, 1.0 if i % 3 else 0.75) for t in req]
        order = rng.permutation(len(subs))
        out.append(And([subs[j] for j in order], boost=2.5 if i % 7 == 0 else 1.0))
        req_leads.append(min(int(dc[t]) for t in req) < min(int(dc[t]) for t in words))
    return out, req_leads


def case_parity(L, num_docs, max_rank, layout, seed=23):
    seg = synth.build_segment(num_docs, max_rank, layout=layout, with_positions=True)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    filters, req_leads = random_queries(seg, max_rank, 24, seed)
    assert sum(req_leads) >= 4 and len(req_leads) - sum(req_leads) >= 4, req_leads
    some = 0
    for scorer in (BM25(), TFIDF(True), TFIDF(False)):
        exp = [expected(seg, f, scorer) for f in filters]
        some += sum(int(m.sum()) > 0 for _, m in exp)
        for k in (1, 10, 1000):
            prep = search.prepare(filters, scorer, st, required_terms=True)
            b = sr.batch(prep, k)
            h, c, t = (x.copy() for x in b.run().results())
            for q, flt in enumerate(filters):
                check(flt, k, h[q], c[q], t[q], *exp[q])
            h2, c2, t2 = b.run().results()    # the batch once more: the same
            assert np.array_equal(h, h2) and np.array_equal(c, c2) and np.array_equal(t, t2), (scorer, k)
            b.close()
    assert some >= 3 * 8, "most queries match nothing: the case checks little"
    sr.close()


def _bits(row, n1):
    return np.unpackbits(row.view(np.uint8), bitorder="little")[:n1].astype(bool)


def case_match_sets(L, num_docs, max_rank, layout):
    """Rows = match_sets(the phrase alone) & bit_union([t]) for every required t, minus deleted and
    excluded docs; counts = the popcounts; sets=False the same counts."""
    seg = synth.build_segment(num_docs, max_rank, layout=layout, with_positions=True)
    seg.doc_mask = np.arange(3, num_docs, 11, dtype=np.uint32)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    hi = max_rank - 1
    shapes = [([1, 2], [0]), ([0, 3], [5, 2]), ([2, 1, 0], [4]), ([3, 0], [hi, 1]), ([1, 0], [hi - 1]),
              ([4, 2], [0, 1, 3, 5, 6, 7]), ([0, 1], [1])]
    filters = [And([by_phrase(w)] + [by_term(t) for t in r]) for w, r in shapes]
    filters.append(And([by_phrase([1, 2]), by_term(0), Not(by_term(3))]))
    filters.append(by_phrase([1, 2]))
    b = sr.batch(search.prepare(filters, BM25(), st, required_terms=True), 10)
    nw = b.match_words()
    sets, counts = b.match_sets()
    _, counts_only = b.match_sets(sets=False)
    alone = sr.batch(search.prepare([by_phrase(w) for w, _ in shapes], BM25(), st, required_terms=True), 10)
    psets, _ = alone.match_sets()
    n1 = num_docs + 1
    any_hit = 0
    for q, (w, r) in enumerate(shapes):
        want = psets[q].copy()
        for t in r:
            want &= sr.bit_union([t], nw)[0]
        assert np.array_equal(sets[q], want), (w, r)
        assert int(counts[q]) == int(_bits(want, n1).sum()), (w, r)
        any_hit += int(counts[q]) > 0
        # ... and the oracle's composition
        assert np.array_equal(_bits(sets[q], n1), expected(seg, filters[q], BM25())[1]), (w, r)
    assert any_hit >= 4
    q = len(shapes)
    want = psets[0] & sr.bit_union([0], nw)[0] & ~sr.bit_union([3], nw)[0]
    assert np.array_equal(sets[q], want) and int(counts[q]) == int(_bits(want, n1).sum())
    assert np.array_equal(sets[q + 1], psets[0])       # the plain phrase of the batch
    assert not _bits(sets[0], n1)[seg.doc_mask.astype(np.int64)].any()
    assert np.array_equal(counts, counts_only)
    # a scored run of the same batch afterwards agrees with the counts
    h, c, t = b.run().results()
    assert np.array_equal(t.astype(np.uint64), counts)
    b.close()
    alone.close()
    sr.close()


def case_multi(L, sizes, max_rank=64, k=50):
    """create_multi: a required term absent from one segment, index-global statistics, the merged top k."""
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    segs = [synth.build_segment(int(n), max_rank, first_doc=int(f), with_positions=True)
            for n, f in zip(sizes, first)]
    segs[1].metas[5]["docs_count"] = 0     # required term 5 absent from segment 1
    segs[2].metas[2]["docs_count"] = 0     # phrase word 2 absent from segment 2
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    stats = [parity.segment_stats(s) for s in segs]
    filters = [And([by_phrase([0, 1]), by_term(5)]), And([by_term(3), by_phrase([2, 0], [0, 2])]),
               And([by_phrase([1, 0, 3]), by_term(max_rank - 1), by_term(4)], boost=1.5), by_phrase([0, 1])]
    dwf = sum(s.docs_with_field for s in segs)
    ttf = sum(s.total_term_freq for s in segs)
    for scorer in (BM25(), TFIDF(True)):
        prep = search.prepare(filters, scorer, stats, required_terms=True)
        # statistics are index-global: the required term's scorer from the summed docs_count
        dwt5 = sum(int(s.metas[5]["docs_count"]) for s in segs)
        assert prep[0].scorers[2] == scorer.term_scorer(scorer.collect(dwf, dwt5, ttf), f32(1.0))
        b = search.QueryBatch(readers, prep, k)
        h, c, t = b.run().results()
        merged = search.merge_topk_host([(h[i], c[i]) for i in range(len(segs))], k)
        assert int(t[1, 0]) == 0 and int(t[2, 1]) == 0 and int(t[0, 0]) > 0 and int(t[2, 0]) > 0
        for q, flt in enumerate(filters):
            rows = []
            for i, s in enumerate(segs):
                sc, m = expected(s, flt, scorer, segs)
                check(flt, k, h[i, q], c[i, q], t[i, q], sc, m)
                rows += [(-float(sc[d]), i, int(d)) for d in np.nonzero(m)[0]]
            rows.sort()
            ref = np.array([-a for a, _, _ in rows[:k]])
            got = np.array([r[0] for r in merged[q]])
            assert len(got) == len(ref), (q, len(got), len(ref))
            assert np.allclose(got, ref, rtol=parity.REL_TOL, atol=0), q
        b.close()
    for r in readers:
        r.close()


# ------------------------------------------------------------------ host only --

def test_prepare_phrase_and():
    st = [search.SegmentStats(1000, 100_000, np.arange(64, dtype=np.int64) * 3 + 20)]
    sc = BM25()
    ph = by_phrase([1, 2], [0, 3], boost=1.5)
    p = search.prepare([And([by_term(7, 0.5), ph, Not(by_term(9)), by_term(4)], boost=2.0)], sc, st, required_terms=True)[0]
    assert p.op == _lib.OP_PHRASE and p.terms == [1, 2, 7, 4] and p.offsets == [0, 3, 0, 0]
    assert p.required == [False, False, True, True] and p.excluded == [9] and p.alts is None
    assert p.merge == search.MERGE_SUM
    # the phrase's blob from its own words, each by_term its own collect; the And's boost into both
    alone = search.prepare([by_phrase([1, 2], [0, 3], boost=float(f32(f32(2.0) * f32(1.5))))], sc, st, required_terms=True)[0]
    assert p.scorers[0] == p.scorers[1] == alone.scorers[0]
    for j, (t, boost) in ((2, (7, 0.5)), (3, (4, 1.0))):
        want = sc.term_scorer(sc.collect(1000, int(st[0].docs_count[t]), 100_000), f32(f32(2.0) * f32(boost)))
        assert p.scorers[j] == want, (j, p.scorers[j], want)
    arr = search.QueryArrays.from_prepared([type("S", (), {"metas": np.zeros(64)})()], [p], 10)
    R = _lib.PHRASE_REQUIRED
    assert list(arr.terms[0, :5]["kind"]) == [_lib.SCORE_BM25, _lib.SCORE_BM25, _lib.SCORE_BM25 | R,
                                               _lib.SCORE_BM25 | R, _lib.EXCLUDE]
    assert list(arr.terms[0, :4]["phrase_offset"]) == [0, 3, 0, 0] and int(arr.queries[0]["n_terms"]) == 5
    # without required terms nothing changes: such prepared queries compare equal to what they were
    plain = search.prepare([by_phrase([1, 2])], sc, st, required_terms=True)[0]
    assert plain.required is None
    assert plain == search.PreparedQuery(_lib.OP_PHRASE, [1, 2], plain.scorers, 0, [0, 1])
    assert _lib.PHRASE_REQUIRED == 0x400
    for bad, why in [(And([by_phrase([1, 2]), by_phrase([3, 4]), by_term(5)]), "two phrases"),
                     (And([by_phrase([[1, 2], 3]), by_term(5)]), "variadic by_phrase with required terms"),
                     (And([by_phrase([1, 2]), Or([by_term(3), by_term(4)])]), "Or group next to a by_phrase"),
                     (Or([by_phrase([1, 2]), by_term(3)]), "by_phrase inside an Or"),
                     (And([by_term(5), Or([by_term(3), by_phrase([1, 2])])]), "by_phrase inside an Or"),
                     (And([by_phrase([1, 2]), by_term(3)], merge=search.MERGE_MAX), "merges with SUM"),
                     (And([by_phrase([1, 2, 3])] + [by_term(t) for t in range(4, 10)]), "at most 8 entries"),
                     (And([And([by_phrase([1, 2]), by_term(3)]), by_term(4)]), "outermost And")]:
        with pytest.raises(ValueError, match=why):
            search.prepare([bad], sc, st, required_terms=True)
    # the shape is asked for: without required_terms=True prepare() refuses it as it always did
    with pytest.raises(ValueError, match="required_terms=True"):
        search.prepare([And([by_phrase([1, 2]), by_term(3)])], sc, st)
    with pytest.raises(ValueError, match="required_terms=True"):
        search.prepare([And([by_term(3), by_phrase([1, 2]), Not(by_term(4))])], sc, st)
    with pytest.raises(ValueError, match=r"IRS_HIP_PHRASE_REQUIRED\) is taken by prepare\(\)"):
        search.prepare_filters([And([by_phrase([1, 2]), by_term(3)])], sc, st, [], 10)


def _cpp(L, tmp_path, extra=()):
    """tests/cpp/test_phrase_and.cpp: the C++ layer's And of a by_phrase and by_terms."""
    import subprocess
    from pathlib import Path
    from iresearch_amd import _build
    root = Path(__file__).resolve().parents[1]
    synth_lib = _build.build_synth()
    exe = tmp_path / "test_phrase_and"
    lib = Path(L._name)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall",
           "-I", str(root / "include"), "-I", str(root / "iresearch_amd" / "cpp"),
           "-I", str(root / "iresearch_amd" / "index"),
           str(root / "tests" / "cpp" / "test_phrase_and.cpp"), "-o", str(exe), str(lib), str(synth_lib),
           "-pthread", "-Wl,-rpath," + str(lib.parent), "-Wl,-rpath," + str(Path(synth_lib).parent), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "test_phrase_and OK" in run.stdout, (run.stdout + run.stderr)[-3000:]


# ---------------------------------------------------------------- emulator --

def test_phrase_and_abi_emulated(simlib):
    case_abi(simlib)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_phrase_and_lists_emulated(simlib, layout):
    case_lists(simlib, layout)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_phrase_and_parity_emulated(simlib, layout):
    case_parity(simlib, 6_000, 48, layout)


def test_phrase_and_match_sets_emulated(simlib):
    case_match_sets(simlib, 6_000, 48, synth.LAYOUT_SIMD4)


def test_phrase_and_multi_emulated(simlib):
    case_multi(simlib, (3_000, 1_500, 4_000))


def test_cpp_phrase_and_emulated(simlib, tmp_path):
    _cpp(simlib, tmp_path)


# --------------------------------------------------------------------- GPU --

@pytest.mark.gpu
def test_phrase_and_abi_gpu(gpulib):
    case_abi(gpulib)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_phrase_and_lists_gpu(gpulib, layout):
    case_lists(gpulib, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_phrase_and_parity_gpu(gpulib, layout):
    case_parity(gpulib, 200_000, 256, layout)


@pytest.mark.gpu
def test_phrase_and_match_sets_gpu(gpulib):
    case_match_sets(gpulib, 200_000, 256, synth.LAYOUT_SIMD4)


@pytest.mark.gpu
def test_phrase_and_multi_gpu(gpulib):
    case_multi(gpulib, (60_000, 20_000, 90_000), max_rank=128, k=100)


@pytest.mark.gpu
def test_cpp_phrase_and_gpu(gpulib, tmp_path):
    rocm = "/opt/rocm/lib"
    _cpp(gpulib, tmp_path, ["-Wl,-rpath," + rocm, "-Wl,-rpath-link," + rocm, "-Wl,--allow-shlib-undefined"])
