"""And([by_phrase, by_phrase..., by_term...]) — several phrases in one And, plus required terms
(IRS_HIP_PHRASE_NEXT, k_phrases_and): the reference's Conjunction over {PhraseIterator...,
term iterators} (boolean_filter.cpp:150-210, boolean_query.cpp:60-145, conjunction.hpp:436-490).

The expected value is composed from the oracle as it stands, as test_phrase_and.py composes it for
one phrase: oracle.score_all_phrase once per phrase (boost = f32(And boost x phrase boost)),
oracle.score_all with OP_AND over the required terms; a doc matches when every phrase has pf > 0 and
the terms hold it, minus the excluded terms' docs and the docs outside the doc set; its score is the
float32 sum of the parts.  The order the kernel sums the children in (cost order) lies inside
parity.REL_TOL, so the expectation does not reproduce it.  One body per case runs on the emulator
(CPU tier) and on the GPU at a larger size."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle
import parity
import test_phrase_and as pa
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, TFIDF, And, Not, Or, by_doc_set, by_phrase, by_term
from test_phrase_and import check

f32 = np.float32
LAYOUTS = [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR]


# ------------------------------------------------------------- expectations --

def split(flt):
    """(phrases, required by_terms, excluded term ordinals, And boost, doc-set row or None) of a
    filter of this file: a by_phrase alone, or an And of by_phrases, by_terms, Not(by_term)s and a
    by_doc_set."""
    if isinstance(flt, by_phrase):
        return [flt], [], [], 1.0, None
    rows = [s.row for s in flt.subs if isinstance(s, by_doc_set)]
    return ([s for s in flt.subs if isinstance(s, by_phrase)], [s for s in flt.subs if isinstance(s, by_term)],
            [s.filter.term for s in flt.subs if isinstance(s, Not)], flt.boost, rows[0] if rows else None)


def expected(seg, flt, scorer, all_segs=None, doc_sets=None):
    """(scores f32[num_docs + 1], matched bool[num_docs + 1]) of `flt` on `seg`; statistics over
    `all_segs` (default: this segment); doc_sets: bool[rows][num_docs + 1]."""
    all_segs = all_segs or [seg]
    phrases, req, excl, mult, row = split(flt)
    osc = parity.oracle_scorer(scorer)
    view = parity.oracle_view(seg)
    dwf = sum(s.docs_with_field for s in all_segs)
    ttf = sum(s.total_term_freq for s in all_segs)
    n1 = seg.num_docs + 1
    terms = [t for ph in phrases for t in ph.terms] + [s.term for s in req]
    if not all(pa._present(seg, t) for t in terms):   # an absent word or required term: nothing
        return np.zeros(n1, f32), np.zeros(n1, bool)

    def dwt(ts):
        return [sum(int(s.metas[t]["docs_count"]) if 0 <= t < len(s.metas) else 0 for s in all_segs)
                for t in ts]
    matched = np.ones(n1, bool)
    scores = None
    for ph in phrases:
        sc, pf = oracle.score_all_phrase(view, parity.metas_for(seg, ph.terms), ph.offsets, osc, dwf,
                                         dwt(ph.terms), ttf, float(f32(f32(mult) * f32(ph.boost))))
        matched &= pf[:n1] > 0
        part = sc[:n1].astype(f32)
        scores = part if scores is None else (scores + part).astype(f32)
    if req:
        rt = [s.term for s in req]
        boosts = [f32(f32(mult) * f32(s.boost)) for s in req]
        ts, tm = oracle.score_all(view, parity.metas_for(seg, rt), oracle.OP_AND, osc, dwf, dwt(rt),
                                  ttf, boosts)
        matched &= tm[:n1].astype(bool)
        scores = (scores + ts[:n1].astype(f32)).astype(f32)
    wc = int(getattr(seg, "wand_count", 0))
    for t in excl:
        if pa._present(seg, t):
            d, _ = oracle.decode_term(seg.doc_file, seg.metas[t], seg.layout, wand_count=wc)
            matched[d.astype(np.int64)] = False
    if row is not None:
        matched &= doc_sets[row][:n1]
    scores = scores.copy()
    scores[~matched] = 0
    return scores, matched


def prepare(filters, scorer, stats):
    return search.prepare(filters, scorer, stats, required_terms=True, phrase_conjunctions=True)


def _run(sr, filters, scorer, k, stats, doc_sets=None):
    prep = prepare(filters, scorer, stats)
    b = search.QueryBatch(sr, prep, k, doc_sets=doc_sets if any(p.doc_set is not None for p in prep) else None)
    n = b.phrase_conj_units()
    h, c, t = (x.copy() for x in b.run().results())
    b.close()
    return prep, h, c, t, n


def n_conj(filters):
    return sum(1 for f in filters if isinstance(f, And) and sum(isinstance(s, by_phrase) for s in f.subs) > 1)


def set_rows(num_docs, rows):
    """(u64[rows][words] for the batch, bool[rows][num_docs + 1] for expected()) of lists of docs"""
    words = num_docs // 64 + 1
    bits = np.zeros((len(rows), words * 64), bool)
    for r, docs in enumerate(rows):
        bits[r, np.asarray(list(docs), np.int64)] = True
    packed = np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(len(rows), words)
    return np.ascontiguousarray(packed), bits[:, :num_docs + 1]


# -------------------------------------------------------------------- cases --

def case_abi(L):
    """IRS_HIP_PHRASE_NEXT validation at batch create — every refusal next to the same batch without
    the violation created and run —, the shapes that are taken, phrase_conj_units, and one-phrase
    units next to a unit of two phrases."""
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

    def create(prep, mutate=None, k=10, reader=sr, run=False):
        arr = search.QueryArrays.from_prepared([reader], prep, k)
        if mutate:
            mutate(arr)
        h = C.c_void_p()
        rc = L.irs_hip_batch_create(reader.handle, arr.queries.ctypes.data, len(arr.queries),
                                    arr.terms.ctypes.data, arr.terms.shape[1], C.byref(h))
        if rc == 0:
            if run:
                assert L.irs_hip_batch_run(h, None) == _lib.OK
            L.irs_hip_batch_destroy(h)
        return rc

    def edit(**kw):
        def f(arr):
            for name, changes in kw.items():
                for j, v in changes.items():
                    arr.terms[0, j][name] = v
        return f
    B, N, R = _lib.SCORE_BM25, _lib.PHRASE_NEXT, _lib.PHRASE_REQUIRED
    assert N == 0x2000
    p1, p2 = by_phrase([1, 2]), by_phrase([3, 4])
    good = prepare([And([p1, p2, by_term(5)])], BM25(), st)          # w w N w R
    two = prepare([And([p1, p2])], BM25(), st)                         # w w N w
    assert good[0].opens == [False, False, True, False, False] and two[0].required is None
    kinds = search.QueryArrays.from_prepared([sr], good, 10).terms[0, :5]["kind"]
    assert list(kinds) == [B, B, B | N, B, B | R]
    assert create(good, run=True) == _lib.OK and create(two, run=True) == _lib.OK
    # IRS_HIP_EINVAL ---------------------------------------------------------------------------
    for op in (_lib.OP_OR, _lib.OP_AND, _lib.OP_MINMATCH, _lib.OP_MULTITERM):   # the flag under another op
        def other_op(arr, op=op):
            arr.queries[0]["op"] = op
            arr.queries[0]["min_match"] = 2
        assert create(two, other_op) == _lib.EINVAL, op
    assert create(two, edit(kind={0: B | N})) == _lib.EINVAL                       # on entry 0
    for flag in (_lib.PHRASE_ALT, R, _lib.PHRASE_OPTIONAL):                        # next to another flag
        assert create(two, edit(kind={2: B | N | flag})) == _lib.EINVAL, flag
        assert create(good, edit(kind={2: B | N | flag})) == _lib.EINVAL, flag
    assert create(two, edit(kind={2: _lib.EXCLUDE | N})) == _lib.EINVAL
    with_not = prepare([And([p1, p2, Not(by_term(6))])], BM25(), st)              # w w N w X
    assert create(with_not, run=True) == _lib.OK
    assert create(with_not, edit(kind={4: _lib.EXCLUDE | N})) == _lib.EINVAL
    assert create(two, edit(phrase_offset={2: 1})) == _lib.EINVAL                  # a flagged entry's offset
    assert create(two, edit(phrase_offset={3: 4})) == _lib.OK                      # (its second word's is free)
    assert create(two, edit(kind={1: B | N, 2: B})) == _lib.EINVAL                 # w N w w: a phrase of one word
    assert create(two, edit(kind={3: B | N})) == _lib.EINVAL                       # w w N N
    assert create(good, edit(kind={3: B | R})) == _lib.EINVAL                      # w w N R R
    assert create(good, edit(kind={2: B | R, 3: B | N})) == _lib.EINVAL            # w w R N w: behind a required entry
    assert create(good, edit(kind={3: B | R, 4: B | N})) == _lib.EINVAL            # w w N R N
    assert create(two, edit(c0={3: 0.5})) == _lib.EINVAL                           # one phrase, two scorer values
    assert create(two, edit(c0={1: 0.5})) == _lib.EINVAL
    assert create(two, edit(kind={3: _lib.SCORE_TFIDF})) == _lib.EINVAL
    assert create(two, edit(c0={2: 0.5, 3: 0.5})) == _lib.OK                       # different phrases may differ
    assert create(two, edit(kind={2: _lib.SCORE_TFIDF | N, 3: _lib.SCORE_TFIDF})) == _lib.OK

    def merge_max(arr):
        arr.queries[0]["merge"] = search.MERGE_MAX
    assert create(two, merge_max) == _lib.EINVAL                                   # merge stays SUM
    # shapes that are taken ---------------------------------------------------------------------
    shapes = {
        "2+2": And([p1, p2]), "3+2": And([by_phrase([1, 2, 3]), by_phrase([4, 5])]),
        "2+2+2": And([p1, p2, by_phrase([5, 6])]),
        "2+2+2+2": And([p1, p2, by_phrase([5, 6]), by_phrase([7, 8])]),
        "2+2 with 4 required": And([p1, p2] + [by_term(t) for t in (5, 6, 7, 8)]),
        "3+3+2": And([by_phrase([1, 2, 3]), by_phrase([4, 5, 6]), by_phrase([7, 8])]),
    }
    for name, flt in shapes.items():
        assert create(prepare([flt], BM25(), st), run=True) == _lib.OK, name
    # IRS_HIP_EUNSUPPORTED ----------------------------------------------------------------------
    nine = prepare([shapes["2+2+2+2"]], BM25(), st)
    nine[0].terms.append(9)
    nine[0].scorers.append(good[0].scorers[-1])
    nine[0].offsets.append(0)
    nine[0].opens.append(False)
    nine[0].required = [False] * 8 + [True]
    assert create(nine) == _lib.EUNSUPPORTED                                       # 9 included entries
    three = prepare([And([by_phrase([1, 2, 3]), p2])], BM25(), st)                 # w w w N w
    assert create(three, run=True) == _lib.OK
    assert create(three, edit(kind={1: B | _lib.PHRASE_ALT}, phrase_offset={1: 0})) == _lib.EUNSUPPORTED
    assert create(good, edit(kind={4: B | _lib.PHRASE_OPTIONAL})) == _lib.EUNSUPPORTED
    for other, kw in ((by_phrase([[1, 2], 3]), {}), (Or([by_phrase([1, 2]), by_term(3)]), {"optional_terms": True})):
        mixed = search.prepare([other, And([p1, p2])], BM25(), st, phrase_conjunctions=True, **kw)
        assert create(mixed) == _lib.EUNSUPPORTED, other
        assert create(mixed[::-1]) == _lib.EUNSUPPORTED, other
        assert create(mixed[:1], run=True) == _lib.OK and create(mixed[1:], run=True) == _lib.OK
    bare = synth.segment_from_lists([(d, f) for d, f, _ in lists], num_docs, synth.LAYOUT_SIMD4)
    sr_bare = search.SegmentReader.from_synth(bare, L=L)
    assert create(two, reader=sr_bare) == _lib.EUNSUPPORTED                        # a segment without positions
    sr_bare.close()
    # which path ran; a unit with one phrase is what it is in a batch without the flag, bit for bit --
    flts = [by_phrase([1, 3]), And([by_phrase([1, 3]), by_term(4)]), And([by_phrase([1, 3]), by_phrase([2, 5])]),
            by_phrase([2, 5, 1], [0, 1, 3]), And([by_phrase([1, 3]), by_phrase([2, 5]), by_term(10_000)])]
    for scorer in (BM25(), TFIDF(True)):
        prep, h, c, t, n = _run(sr, flts, scorer, 10, st)
        assert n == 2
        for q, flt in enumerate(flts):
            check(flt, 10, h[q], c[q], t[q], *expected(seg, flt, scorer))
        assert int(t[4]) == 0 and int(c[4]) == 0 and int(t[2]) <= int(t[0]) and int(t[0]) > 0
        keep = [0, 1, 3]
        _, h1, c1, t1, n1 = _run(sr, [flts[q] for q in keep], scorer, 10, st)
        assert n1 == 0
        for at, q in enumerate(keep):
            assert np.array_equal(h[q], h1[at]) and c[q] == c1[at] and t[q] == t1[at], (scorer, q)
    sr.close()


N_LISTS = pa.N_LISTS
(NEW, YORK, HOTEL, THE, ONE_HIT, ONE_MISS, L127, L128, L129, L257, NINES, RARE, CITY) = range(13)
REAL, ESTATE, A, B_, ONE72 = range(13, 18)


def hand_lists():
    """test_phrase_and.hand_lists() — "new york" in d % 12 == 0, twice in d % 24 == 0 — and:
    "real estate": real in d % 4 == 0, estate in d % 6 == 0, next to each other three times in d % 36
    == 0, once in d % 36 == 24, estate two positions late in d % 36 == 12; a and b in d % 7 == 0 as
    "a b", in d % 14 == 0 also as "b a"; one doc, 72."""
    N = N_LISTS
    T = {
        REAL: {d: [50, 60, 70] for d in range(4, N + 1, 4)},
        ESTATE: {d: ([51, 61, 71] if d % 18 == 0 else [51] if d % 18 == 6 else [53]) for d in range(6, N + 1, 6)},
        A: {d: ([1, 4] if d % 14 == 0 else [1]) for d in range(7, N + 1, 7)},
        B_: {d: ([2, 3] if d % 14 == 0 else [2]) for d in range(7, N + 1, 7)},
        ONE72: {72: [40]},
    }
    lists = pa.hand_lists()
    for t in range(13, 18):
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
    dc = [len(x[0]) for x in lists]
    assert (dc[NEW], dc[YORK], dc[REAL], dc[ESTATE], dc[A]) == (4000, 6000, 3000, 2000, 1714)
    ny, re, ab, ba = by_phrase([NEW, YORK]), by_phrase([REAL, ESTATE]), by_phrase([A, B_]), by_phrase([B_, A])
    nc = by_phrase([NEW, CITY], [0, 2])          # new@1 city@3: d % 36 == 0
    docs = range(1, N + 1)
    both = {d for d in docs if d % 36 in (0, 24)}      # "new york" and "real estate"
    sets, set_bits = set_rows(N, [range(1, 5001), [36, 7200]])
    cases = [
        # the lead (estate, 2000 docs: 15 blocks and a tail; "new" spans 31 blocks, "the" 93) is a
        # word of phrase 2; d % 36 == 12 holds all four words and "new york", estate two late
        (And([ny, re]), both),
        # ... of phrase 1; the mirror: d % 36 == 12 matches phrase 2 and not phrase 1
        (And([re, ny]), both),
        # a required term leads: 257 docs (2 blocks + 1), 127 (a tail alone), one doc (a hit, a miss)
        (And([ny, re, by_term(L257)]), {d for d in both if d <= 3084}),
        (And([by_term(L127), ny, re]), {d for d in both if d <= 762}),
        (And([ny, re, by_term(ONE72)]), {72}),
        (And([ny, re, by_term(ONE_HIT)]), set()),                 # 120 % 36 == 12
        (And([ny, re, by_term(THE), by_term(HOTEL, 0.5)], boost=2.0), {d for d in both if d % 5 == 0}),
        # "a b" and "b a": the same two terms in four rows; the same phrase twice
        (And([ab, ba]), {d for d in docs if d % 14 == 0}),
        (And([ab, ab]), {d for d in docs if d % 7 == 0}),
        # a gap (new@1 .. york@5: d % 6 == 0 and d % 4 != 0) next to a consecutive phrase
        (And([by_phrase([NEW, YORK], [0, 4]), ab]), {d for d in docs if d % 42 == 0 and d % 4}),
        # three and four phrases (8 rows); a three-word phrase next to a two-word one
        (And([ny, re, ab]), {d for d in both if d % 7 == 0}),
        (And([ny, re, ab, nc]), {d for d in docs if d % 252 == 0}),
        (And([by_phrase([NEW, YORK, CITY]), re, by_term(NINES)]), {d for d in docs if d % 36 == 0 and d <= 2700}),
        # Not hitting matches (d % 180 == 0); an absent excluded term; an absent word
        (And([ny, re, Not(by_term(RARE))]), {d for d in both if d % 90}),
        (And([ny, re, Not(by_term(10_000))]), both),
        (And([ny, by_phrase([REAL, 10_000])]), set()),
        # doc sets: docs up to 5000 (the lead's blocks 7 .. 15 have no doc left); two docs
        (And([ny, re, by_doc_set(0)]), {d for d in both if d <= 5000}),
        (And([re, ny, by_term(THE), by_doc_set(1)]), {36, 7200}),
        (And([ny, by_term(HOTEL)]), {d for d in docs if d % 60 == 0}),
        (ny, {d for d in docs if d % 12 == 0}),
    ]
    filters = [f for f, _ in cases]
    small = [0, 1, 7, 8, 9, 19]      # at most 4 rows each: a batch of them runs the <4> instantiation
    k = 10
    for scorer in (BM25(), TFIDF(True)):
        exp = [expected(seg, f, scorer, doc_sets=set_bits) for f in filters]
        for (flt, want), (_, matched) in zip(cases, exp):
            assert set(np.nonzero(matched)[0].tolist()) == want, ("the oracle and the hand list differ", flt)
        for pick in (range(len(cases)), small):
            pick = list(pick)
            for kk in (k, 2000):
                prep, h, c, t, n = _run(sr, [filters[q] for q in pick], scorer, kk, st, doc_sets=sets)
                assert max(len(p.terms) for p in prep) == (8 if len(pick) > len(small) else 4)
                assert n == n_conj([filters[q] for q in pick])
                for at, q in enumerate(pick):
                    flt, want = cases[q]
                    assert int(t[at]) == len(want), (flt, int(t[at]), len(want))
                    if kk == 2000:
                        assert set(h[at, :int(c[at])]["doc"].tolist()) == want, flt
                    check(flt, kk, h[at], c[at], t[at], *exp[q])
    # each phrase's own frequency is its scorer's tf: new york twice in d % 24 == 0, real estate three
    # times in d % 36 == 0 — 72 has (2, 3), 36 (1, 3), 24 (2, 1), 60 (1, 1)
    _, h, c, t, _ = _run(sr, [And([ny, re]), ny, re, And([ab, ab]), ab], TFIDF(False), 2000, st)
    by = [{int(x["doc"]): float(x["score"]) for x in h[q, :int(c[q])]} for q in range(5)]
    assert by[0][72] > by[0][36] > by[0][60] and by[0][72] > by[0][24] > by[0][60]
    for d in (24, 36, 60, 72):
        assert abs(by[0][d] - float(f32(f32(by[1][d]) + f32(by[2][d])))) <= parity.REL_TOL * by[0][d], d
    # the same phrase twice: the phrase's docs, its score added to itself
    assert set(by[3]) == set(by[4])
    for d, s in by[4].items():
        assert abs(by[3][d] - float(f32(f32(s) + f32(s)))) <= parity.REL_TOL * by[3][d], d
    # deleted docs among the matches
    seg2 = synth.segment_from_lists(lists, N, layout, norms=norms)
    seg2.doc_mask = np.array([7, 36, 1824, 7200], np.uint32)
    sr2 = search.SegmentReader.from_synth(seg2, L=L)
    assert {36, 1824, 7200} <= both
    for scorer in (BM25(), TFIDF(True)):
        for flt, want in ((And([ny, re]), both - {36, 1824, 7200}),
                          (And([re, ny, Not(by_term(RARE))]), {d for d in both if d % 90} - {36, 1824, 7200})):
            sc, matched = expected(seg2, flt, scorer)
            assert set(np.nonzero(matched)[0].tolist()) == want
            for kk in (1, 2000):
                _, h, c, t, _ = _run(sr2, [flt], scorer, kk, st)
                check(flt, kk, h[0], c[0], t[0], sc, matched)
    sr.close()
    sr2.close()


def parity_filters(max_rank):
    pairs = [([0, 1], [2, 0]), ([0, 1], [1, 0]), ([1, 4, 0], [0, 2]), ([0, 1], [2, 3]),
             ([3, 1], [0, 2], [1, 0]), ([0, 1], [5, max_rank - 1]), ([0, 3], [1, 2])]
    listed = [And([by_phrase(w) for w in ws]) for ws in pairs]
    more = [And([by_phrase([0, 1], boost=1.5), by_term(4, 0.75), by_phrase([2, 0])], boost=2.5),
            And([by_term(max_rank // 2), by_phrase([0, 3]), by_phrase([1, 2], boost=0.5)], boost=0.8)]
    return listed, more


def case_parity(L, num_docs, max_rank, layout, counts):
    seg = synth.build_segment(num_docs, max_rank, layout=layout, with_positions=True)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    listed, more = parity_filters(max_rank)
    filters = listed + more
    k = 50
    for scorer in (BM25(), BM25(1.2, 0.0), TFIDF(False), TFIDF(True)):
        exp = [expected(seg, f, scorer) for f in filters]
        got = [int(m.sum()) for _, m in exp[:len(listed)]]
        # the condition of the case, from the oracle's arrays: every query matches, three beyond k
        assert all(n > 0 for n in got) and sum(n > k for n in got) >= 3, got
        assert got == list(counts), (got, counts)
        prep = prepare(filters, scorer, st)
        b = sr.batch(prep, k)
        assert b.phrase_conj_units() == len(filters)
        h, c, t = (x.copy() for x in b.run().results())
        for q, flt in enumerate(filters):
            check(flt, k, h[q], c[q], t[q], *exp[q])
        h2, c2, t2 = b.run().results()    # the batch once more: the same
        assert np.array_equal(h, h2) and np.array_equal(c, c2) and np.array_equal(t, t2), scorer
        b.close()
    sr.close()


def _bits(row, n1):
    return np.unpackbits(row.view(np.uint8), bitorder="little")[:n1].astype(bool)


def case_match_sets(L, num_docs, max_rank, layout):
    """Rows = the AND of match_sets(each phrase alone) & bit_union([t]) for every required t, minus
    deleted and excluded docs; counts = the popcounts; sets=False the same counts."""
    seg = synth.build_segment(num_docs, max_rank, layout=layout, with_positions=True)
    seg.doc_mask = np.arange(3, num_docs, 11, dtype=np.uint32)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    shapes = [(([0, 1], [2, 0]), []), (([0, 1], [1, 0]), [3]), (([1, 4, 0], [0, 2]), []), (([0, 3], [1, 2]), [4, 0]),
              (([3, 1], [0, 2], [1, 0]), []), (([0, 1], [2, 3], [0, 3], [1, 2]), [])]
    filters = [And([by_phrase(w) for w in ws] + [by_term(t) for t in r]) for ws, r in shapes]
    filters.append(And([by_phrase([0, 1]), by_phrase([2, 0]), Not(by_term(3))]))
    filters.append(by_phrase([0, 1]))
    b = sr.batch(prepare(filters, BM25(), st), 10)
    assert b.phrase_conj_units() == len(filters) - 1
    nw = b.match_words()
    sets, counts = b.match_sets()
    _, counts_only = b.match_sets(sets=False)
    words = sorted({tuple(w) for ws, _ in shapes for w in ws})
    alone = sr.batch(search.prepare([by_phrase(list(w)) for w in words], BM25(), st), 10)
    psets, _ = alone.match_sets()
    own = {w: psets[i] for i, w in enumerate(words)}
    n1 = num_docs + 1
    any_hit = 0
    for q, (ws, r) in enumerate(shapes):
        want = own[tuple(ws[0])].copy()
        for w in ws[1:]:
            want &= own[tuple(w)]
        for t in r:
            want &= sr.bit_union([t], nw)[0]
        assert np.array_equal(sets[q], want), (ws, r)
        assert int(counts[q]) == int(_bits(want, n1).sum()), (ws, r)
        any_hit += int(counts[q]) > 0
        assert np.array_equal(_bits(sets[q], n1), expected(seg, filters[q], BM25())[1]), (ws, r)
    assert any_hit >= 4
    q = len(shapes)
    want = own[(0, 1)] & own[(2, 0)] & ~sr.bit_union([3], nw)[0]
    assert np.array_equal(sets[q], want) and int(counts[q]) == int(_bits(want, n1).sum())
    assert np.array_equal(sets[q + 1], own[(0, 1)])       # the plain phrase of the batch
    assert not _bits(sets[0], n1)[seg.doc_mask.astype(np.int64)].any()
    assert np.array_equal(counts, counts_only)
    # a scored run of the same batch afterwards agrees with the counts
    h, c, t = b.run().results()
    assert np.array_equal(t.astype(np.uint64), counts)
    b.close()
    alone.close()
    sr.close()


def case_multi(L, sizes, max_rank=64, k=50):
    """create_multi: a word absent from one segment, index-global statistics, one threshold per
    query over the segments, the merged top k."""
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    segs = [synth.build_segment(int(n), max_rank, first_doc=int(f), with_positions=True)
            for n, f in zip(sizes, first)]
    segs[1].metas[2]["docs_count"] = 0     # word 2 absent from segment 1
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    stats = [parity.segment_stats(s) for s in segs]
    filters = [And([by_phrase([0, 1]), by_phrase([2, 0])]), And([by_phrase([0, 3]), by_phrase([1, 0])]),
               And([by_phrase([1, 0, 3]), by_term(4), by_phrase([0, 1], boost=0.5)], boost=1.5), by_phrase([0, 1])]
    dwf = sum(s.docs_with_field for s in segs)
    ttf = sum(s.total_term_freq for s in segs)
    for scorer in (BM25(), TFIDF(True)):
        prep = prepare(filters, scorer, stats)
        # statistics are index-global: each phrase's blob from the summed docs_count of its own words
        alone = search.prepare([by_phrase([2, 0])], scorer, stats)[0]
        assert prep[0].scorers[2] == prep[0].scorers[3] == alone.scorers[0] != prep[0].scorers[0]
        dwt4 = sum(int(s.metas[4]["docs_count"]) for s in segs)
        assert prep[2].terms == [1, 0, 3, 0, 1, 4]
        assert prep[2].scorers[5] == scorer.term_scorer(scorer.collect(dwf, dwt4, ttf), f32(1.5))
        for shared in (False, True):
            b = search.QueryBatch(readers, prep, k).set_shared_threshold(shared)
            assert b.phrase_conj_units() == 3 * len(segs)
            h, c, t = b.run().results()
            merged = search.merge_topk_host([(h[i], c[i]) for i in range(len(segs))], k)
            assert int(t[1, 0]) == 0 and int(t[0, 0]) > 0 and int(t[2, 0]) > 0
            for q, flt in enumerate(filters):
                rows = []
                for i, s in enumerate(segs):
                    sc, m = expected(s, flt, scorer, segs)
                    assert int(t[i, q]) == int(m.sum()), (q, i)
                    if not shared:
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


def case_misled(L, layout, capfd):
    """k_phrases_and on test_block_driven._misled_phrase_segment, as test_pilot_recovery builds its
    phrase-plus-required-terms case: And(["q 2", "q . 3"]) for q = 0, 1 (4 rows: the <4>
    instantiation) and the same with "2 3" and two required terms (8 rows).  Lead q is the rarest row:
    64 items, stride 16 samples 4, all hot — 512 docs on which both phrases have frequency 50, >= need
    = 188 and < k = 1000 of 8192 matches: one re-run, both units short of k, results bit for bit the
    stride-1 batch's.  Control: shift 8."""
    import test_pilot_recovery as pr
    from test_block_driven import MISLED_K, STRIDE, _misled_phrase_segment
    import sys
    k, scorer = MISLED_K, TFIDF(False)
    assert pr.pilot_need(k, 4, 64) == 188
    batches = [[And([by_phrase([q, 2]), by_phrase([q, 3], [0, 2])]) for q in range(2)],
               [And([by_phrase([q, 2]), by_phrase([q, 3], [0, 2]), by_phrase([2, 3]), by_term(3), by_term(2)])
                for q in range(2)]]
    me = sys.modules[__name__]
    for shift, reruns in ((0, 1), (STRIDE // 2, 0)):
        seg, sr = _misled_phrase_segment(L, layout, shift)
        for filters in batches:
            prep = prepare(filters, scorer, [parity.segment_stats(seg)])

            def checked(res):
                pr._check_family(me, [seg], filters, scorer, k)(res)
                assert (res[2] == 8192).all()
            pr._misled(pr._maker([sr], prep, k, STRIDE), False, checked,
                       lambda b: (b.path(), b.phrase_conj_units()), capfd, reruns, [2] * reruns,
                       listed=(512, 8192) if reruns else None, what=("phrases and", len(prep[0].terms), shift))
        sr.close()


# ------------------------------------------------------------------ host only --

def test_prepare_phrases_and():
    st = [search.SegmentStats(1000, 100_000, np.arange(64, dtype=np.int64) * 3 + 20)]
    sc = BM25()
    p1, p2 = by_phrase([1, 2], [0, 3], boost=1.5), by_phrase([5, 6, 2])
    flt = And([by_term(7, 0.5), p1, Not(by_term(9)), p2], boost=2.0)
    p = search.prepare([flt], sc, st, phrase_conjunctions=True)[0]
    assert p.op == _lib.OP_PHRASE and p.terms == [1, 2, 5, 6, 2, 7] and p.offsets == [0, 3, 0, 1, 2, 0]
    assert p.opens == [False, False, True, False, False, False]
    assert p.required == [False] * 5 + [True] and p.excluded == [9] and p.alts is None
    assert p.merge == search.MERGE_SUM
    # every phrase its own blob from its own words, the by_term its own collect; the And's boost into all
    a1 = search.prepare([by_phrase([1, 2], [0, 3], boost=float(f32(f32(2.0) * f32(1.5))))], sc, st)[0]
    a2 = search.prepare([by_phrase([5, 6, 2], boost=2.0)], sc, st)[0]
    assert p.scorers[0] == p.scorers[1] == a1.scorers[0]
    assert p.scorers[2] == p.scorers[3] == p.scorers[4] == a2.scorers[0] != a1.scorers[0]
    want = sc.term_scorer(sc.collect(1000, int(st[0].docs_count[7]), 100_000), f32(f32(2.0) * f32(0.5)))
    assert p.scorers[5] == want
    arr = search.QueryArrays.from_prepared([type("S", (), {"metas": np.zeros(64)})()], [p], 10)
    B, N, R = _lib.SCORE_BM25, _lib.PHRASE_NEXT, _lib.PHRASE_REQUIRED
    assert N == 0x2000
    assert list(arr.terms[0, :7]["kind"]) == [B, B, B | N, B, B, B | R, _lib.EXCLUDE]
    assert list(arr.terms[0, :6]["phrase_offset"]) == [0, 3, 0, 1, 2, 0] and int(arr.queries[0]["n_terms"]) == 7
    assert list(arr.terms[0, :6]["c0"]) == [f32(s[1]) for s in p.scorers]
    # a nested And under Nots, and a doc set, go the way they always went
    q = search.prepare([And([And([p1, p2], boost=2.0), Not(by_term(9))])], sc, st, phrase_conjunctions=True)[0]
    assert q.terms == [1, 2, 5, 6, 2] and q.excluded == [9] and q.required is None
    assert q.scorers == p.scorers[:5]
    d = search.prepare([And([p1, p2, by_doc_set(3)])], sc, st, phrase_conjunctions=True)[0]
    assert d.doc_set == 3 and d.opens == [False, False, True, False, False]
    # one phrase: nothing changes, such prepared queries compare equal to what they were
    one = search.prepare([And([p1, by_term(7)])], sc, st, required_terms=True, phrase_conjunctions=True)[0]
    assert one.opens is None and one == search.prepare([And([p1, by_term(7)])], sc, st, required_terms=True)[0]
    plain = search.prepare([by_phrase([1, 2])], sc, st, phrase_conjunctions=True)[0]
    assert plain == search.PreparedQuery(_lib.OP_PHRASE, [1, 2], plain.scorers, 0, [0, 1])
    # off by default: today's refusals, word for word
    with pytest.raises(ValueError, match="two phrases in one And are not on the GPU path"):
        search.prepare([And([p1, p2])], sc, st, required_terms=True)
    with pytest.raises(ValueError, match="required_terms=True"):
        search.prepare([And([p1, p2])], sc, st)
    with pytest.raises(ValueError, match=r"phrase_conjunctions=True\), not by the array path"):
        search.prepare_filters([And([p1, p2])], sc, st, [], 10)
    for bad, why in [(And([by_phrase([[1, 2], 3]), p2]), "variadic by_phrase next to another phrase"),
                     (And([p1, p2, Or([by_term(3), by_term(4)])]), "Or group next to by_phrase children"),
                     (And([p1, p2], merge=search.MERGE_MAX), "merges with SUM"),
                     (And([by_phrase([1, 2, 3]), by_phrase([4, 5, 6]), by_phrase([7, 8]), by_term(9)]),
                      "at most 8 entries"),
                     (And([p1, by_phrase([4])]), "by_phrase of one term is a by_term"),
                     (And([by_phrase([t, t + 1]) for t in range(1, 6)]), "more than four phrases"),
                     (Or([p1, p2]), "not on the GPU path")]:
        with pytest.raises(ValueError, match=why):
            search.prepare([bad], sc, st, required_terms=True, phrase_conjunctions=True)


def _cpp(L, tmp_path, extra=()):
    """tests/cpp/test_phrases_and.cpp: the C++ layer's And of several by_phrases."""
    import subprocess
    from pathlib import Path
    from iresearch_amd import _build
    root = Path(__file__).resolve().parents[1]
    synth_lib = _build.build_synth()
    exe = tmp_path / "test_phrases_and"
    lib = Path(L._name)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall",
           "-I", str(root / "include"), "-I", str(root / "iresearch_amd" / "cpp"),
           "-I", str(root / "iresearch_amd" / "index"),
           str(root / "tests" / "cpp" / "test_phrases_and.cpp"), "-o", str(exe), str(lib), str(synth_lib),
           "-pthread", "-Wl,-rpath," + str(lib.parent), "-Wl,-rpath," + str(Path(synth_lib).parent), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "test_phrases_and OK" in run.stdout, (run.stdout + run.stderr)[-3000:]


SMALL = (6_000, 48, (200, 365, 3, 48, 17, 5, 56))
LARGE = (200_000, 256, (7285, 12231, 114, 1713, 616, 17, 1816))


# ---------------------------------------------------------------- emulator --

def test_phrases_and_abi_emulated(simlib):
    case_abi(simlib)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrases_and_lists_emulated(simlib, layout):
    case_lists(simlib, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrases_and_parity_emulated(simlib, layout):
    case_parity(simlib, SMALL[0], SMALL[1], layout, SMALL[2])


def test_phrases_and_match_sets_emulated(simlib):
    case_match_sets(simlib, 6_000, 48, synth.LAYOUT_SIMD4)


def test_phrases_and_multi_emulated(simlib):
    case_multi(simlib, (3_000, 1_500, 4_000))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrases_and_misled_emulated(simlib, layout, capfd):
    case_misled(simlib, layout, capfd)


def test_cpp_phrases_and_emulated(simlib, tmp_path):
    _cpp(simlib, tmp_path)


# --------------------------------------------------------------------- GPU --

@pytest.mark.gpu
def test_phrases_and_abi_gpu(gpulib):
    case_abi(gpulib)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrases_and_lists_gpu(gpulib, layout):
    case_lists(gpulib, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrases_and_parity_gpu(gpulib, layout):
    case_parity(gpulib, LARGE[0], LARGE[1], layout, LARGE[2])


@pytest.mark.gpu
def test_phrases_and_match_sets_gpu(gpulib):
    case_match_sets(gpulib, 200_000, 256, synth.LAYOUT_SIMD4)


@pytest.mark.gpu
def test_phrases_and_multi_gpu(gpulib):
    case_multi(gpulib, (60_000, 20_000, 90_000), max_rank=128, k=100)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrases_and_misled_gpu(gpulib, layout, capfd):
    case_misled(gpulib, layout, capfd)


@pytest.mark.gpu
def test_cpp_phrases_and_gpu(gpulib, tmp_path):
    rocm = "/opt/rocm/lib"
    _cpp(gpulib, tmp_path, ["-Wl,-rpath," + rocm, "-Wl,-rpath-link," + rocm, "-Wl,--allow-shlib-undefined"])
