"""Or([by_phrase, by_phrase...]) — several phrases in one Or (IRS_HIP_PHRASE_OR, k_phrases_or): the
reference's disjunction over PhraseIterators (boolean_filter.cpp:150-210, disjunction.hpp:1411-1467,
:208-350, :374-).

The expected value is composed from the oracle as it stands: oracle.score_all_phrase once per phrase
(boost = f32(Or boost x phrase boost)); a doc matches when some phrase has pf > 0, minus the excluded
terms' docs and the docs outside the doc set; its score is the float32 sum, in entry order, of the
parts with pf > 0.  A phrase with a word the segment lacks is dropped there.  One body per case runs
on the emulator (CPU tier) and on the GPU at a larger size."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle
import parity
import test_phrase_and as pa
import test_phrases_and as tps
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, TFIDF, And, Not, Or, by_doc_set, by_phrase, by_term
from test_phrase_and import check
from test_phrases_and import (A, B_, CITY, ESTATE, L127, L129, L257, N_LISTS, NEW, ONE72, ONE_MISS, RARE, REAL, THE,
                              YORK, _bits, set_rows)

f32 = np.float32
LAYOUTS = [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR]


# ------------------------------------------------------------- expectations --

def split(flt):
    """(phrases, excluded term ordinals, Or boost, doc-set row or None) of a filter of this file: a
    by_phrase alone, an Or of by_phrases, or an And of one such Or, Not(by_term)s and a by_doc_set."""
    if isinstance(flt, by_phrase):
        return [flt], [], 1.0, None
    if type(flt) is Or:
        return list(flt.subs), [], flt.boost, None
    rows = [s.row for s in flt.subs if isinstance(s, by_doc_set)]
    inner = [s for s in flt.subs if type(s) is Or]
    assert len(inner) == 1 and flt.boost == 1.0
    return (list(inner[0].subs), [s.filter.term for s in flt.subs if isinstance(s, Not)], inner[0].boost,
            rows[0] if rows else None)


def expected_parts(seg, flt, scorer, all_segs=None):
    """Per phrase of `flt` (scores f32[num_docs + 1], pf > 0) on `seg`, None for a phrase with a
    word absent from `seg`; statistics over `all_segs` (default: this segment)."""
    all_segs = all_segs or [seg]
    phrases, _, mult, _ = split(flt)
    osc = parity.oracle_scorer(scorer)
    view = parity.oracle_view(seg)
    dwf = sum(s.docs_with_field for s in all_segs)
    ttf = sum(s.total_term_freq for s in all_segs)
    n1 = seg.num_docs + 1

    def dwt(ts):
        return [sum(int(s.metas[t]["docs_count"]) if 0 <= t < len(s.metas) else 0 for s in all_segs)
                for t in ts]
    parts = []
    for ph in phrases:
        if not all(pa._present(seg, t) for t in ph.terms):
            parts.append(None)
            continue
        sc, pf = oracle.score_all_phrase(view, parity.metas_for(seg, ph.terms), ph.offsets, osc, dwf,
                                         dwt(ph.terms), ttf, float(f32(f32(mult) * f32(ph.boost))))
        parts.append((sc[:n1].astype(f32), pf[:n1] > 0))
    return parts


def expected(seg, flt, scorer, all_segs=None, doc_sets=None):
    """(scores f32[num_docs + 1], matched bool[num_docs + 1]) of `flt` on `seg`; doc_sets:
    bool[rows][num_docs + 1]."""
    _, excl, _, row = split(flt)
    n1 = seg.num_docs + 1
    matched = np.zeros(n1, bool)
    scores = np.zeros(n1, f32)
    for part in expected_parts(seg, flt, scorer, all_segs):
        if part is None:
            continue
        sc, on = part
        first = on & ~matched          # the sum starts from the first matching phrase's value
        scores[first] = sc[first]
        more = on & matched
        scores[more] = (scores[more] + sc[more]).astype(f32)
        matched |= on
    wc = int(getattr(seg, "wand_count", 0))
    for t in excl:
        if pa._present(seg, t):
            d, _ = oracle.decode_term(seg.doc_file, seg.metas[t], seg.layout, wand_count=wc)
            matched[d.astype(np.int64)] = False
    if getattr(seg, "doc_mask", None) is not None and len(seg.doc_mask):
        assert not matched[np.asarray(seg.doc_mask, np.int64)].any(), "the oracle's view drops deleted docs"
    if row is not None:
        matched &= doc_sets[row][:n1]
    scores[~matched] = 0
    return scores, matched


def overlap(seg, flt, scorer):
    """Docs every phrase of `flt` matches."""
    parts = expected_parts(seg, flt, scorer)
    both = np.ones(seg.num_docs + 1, bool)
    for _, on in parts:
        both &= on
    return int(both.sum())


def prepare(filters, scorer, stats):
    return search.prepare(filters, scorer, stats, phrase_disjunctions=True)


def _run(sr, filters, scorer, k, stats, doc_sets=None):
    prep = prepare(filters, scorer, stats)
    b = search.QueryBatch(sr, prep, k, doc_sets=doc_sets if any(p.doc_set is not None for p in prep) else None)
    n = b.phrase_disj_units()
    h, c, t = (x.copy() for x in b.run().results())
    b.close()
    return prep, h, c, t, n


def n_disj(filters):
    return sum(1 for f in filters if not isinstance(f, by_phrase))


# -------------------------------------------------------------------- cases --

def case_abi(L):
    """IRS_HIP_PHRASE_OR validation at batch create — every refusal next to the same batch without
    the violation created and run —, the shapes that are taken, phrase_disj_units, and plain phrases
    next to a unit of two phrases."""
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
    B, O = _lib.SCORE_BM25, _lib.PHRASE_OR
    assert O == 0x4000
    p1, p2 = by_phrase([1, 2]), by_phrase([3, 4])
    two = prepare([Or([p1, p2])], BM25(), st)                         # w w O w
    assert two[0].or_opens == [False, False, True, False] and two[0].opens is None
    kinds = search.QueryArrays.from_prepared([sr], two, 10).terms[0, :4]["kind"]
    assert list(kinds) == [B, B, B | O, B]
    assert create(two, run=True) == _lib.OK
    # the flag is untouched under the default prepare: the shape is refused, a phrase is what it was
    with pytest.raises(ValueError):
        search.prepare([Or([p1, p2])], BM25(), st)
    plain = prepare([p1], BM25(), st)
    assert plain[0].or_opens is None and plain == search.prepare([p1], BM25(), st)
    assert list(search.QueryArrays.from_prepared([sr], plain, 10).terms[0, :2]["kind"]) == [B, B]
    # IRS_HIP_EINVAL ---------------------------------------------------------------------------
    for op in (_lib.OP_OR, _lib.OP_AND, _lib.OP_MINMATCH, _lib.OP_MULTITERM):   # the flag under another op
        def other_op(arr, op=op):
            arr.queries[0]["op"] = op
            arr.queries[0]["min_match"] = 2
        assert create(two, other_op) == _lib.EINVAL, op
    assert create(two, edit(kind={0: B | O})) == _lib.EINVAL                       # on entry 0
    assert create(two, edit(kind={2: _lib.EXCLUDE | O})) == _lib.EINVAL            # on an excluded entry
    with_not = prepare([And([Or([p1, p2]), Not(by_term(6))])], BM25(), st)         # w w O w X
    assert with_not[0].excluded == [6] and create(with_not, run=True) == _lib.OK
    assert create(with_not, edit(kind={4: _lib.EXCLUDE | O})) == _lib.EINVAL
    assert create(two, edit(phrase_offset={2: 1})) == _lib.EINVAL                  # a flagged entry's offset
    assert create(two, edit(phrase_offset={3: 4})) == _lib.OK                      # (its second word's is free)
    assert create(two, edit(kind={1: B | O, 2: B})) == _lib.EINVAL                 # w O w w: a phrase of one word
    assert create(two, edit(kind={3: B | O})) == _lib.EINVAL                       # w w O O
    assert create(two, edit(c0={3: 0.5})) == _lib.EINVAL                           # one phrase, two scorer values
    assert create(two, edit(c0={1: 0.5})) == _lib.EINVAL
    assert create(two, edit(kind={3: _lib.SCORE_TFIDF})) == _lib.EINVAL
    assert create(two, edit(c0={2: 0.5, 3: 0.5})) == _lib.OK                       # different phrases may differ
    assert create(two, edit(kind={2: _lib.SCORE_TFIDF | O, 3: _lib.SCORE_TFIDF})) == _lib.OK

    for merge in (search.MERGE_MAX, search.MERGE_MIN):
        def other_merge(arr, merge=merge):
            arr.queries[0]["merge"] = merge
        assert create(two, other_merge) == _lib.EINVAL                             # merge stays SUM
    # shapes that are taken ---------------------------------------------------------------------
    shapes = {
        "2+2": Or([p1, p2]), "3+2": Or([by_phrase([1, 2, 3]), by_phrase([4, 5])]),
        "2+2+2": Or([p1, p2, by_phrase([5, 6])]),
        "2+2+2+2": Or([p1, p2, by_phrase([5, 6]), by_phrase([7, 8])]),
        "3+3+2": Or([by_phrase([1, 2, 3]), by_phrase([4, 5, 6]), by_phrase([7, 8])]),
        "4+4": Or([by_phrase([1, 2, 3, 4]), by_phrase([4, 5, 6, 7])]),
    }
    for name, flt in shapes.items():
        assert create(prepare([flt], BM25(), st), run=True) == _lib.OK, name
    # IRS_HIP_EUNSUPPORTED ----------------------------------------------------------------------
    nine = prepare([shapes["2+2+2+2"]], BM25(), st)
    nine[0].terms.append(9)
    nine[0].scorers.append(nine[0].scorers[-1])
    nine[0].offsets.append(2)
    nine[0].or_opens.append(False)
    assert create(nine) == _lib.EUNSUPPORTED                                       # 9 included entries
    three = prepare([Or([by_phrase([1, 2, 3]), p2])], BM25(), st)                  # w w w O w
    assert create(three, run=True) == _lib.OK
    assert create(three, edit(kind={1: B | _lib.PHRASE_ALT}, phrase_offset={1: 0})) == _lib.EUNSUPPORTED
    for flag in (_lib.PHRASE_REQUIRED, _lib.PHRASE_OPTIONAL):                      # one of the other flags in the query
        assert create(three, edit(kind={4: B | flag})) == _lib.EUNSUPPORTED, flag
        assert create(three, edit(kind={3: B | O | flag})) == _lib.EUNSUPPORTED, flag
    assert create(prepare([shapes["2+2+2"]], BM25(), st), edit(kind={4: B | _lib.PHRASE_NEXT})) == _lib.EUNSUPPORTED
    assert create(three, edit(kind={3: B | O | _lib.PHRASE_NEXT})) == _lib.EUNSUPPORTED
    others = ((by_phrase([[1, 2], 3]), {}), (And([p1, by_term(5)]), {"required_terms": True}),
              (Or([by_phrase([1, 2]), by_term(3)]), {"optional_terms": True}),
              (And([p1, p2]), {"phrase_conjunctions": True}))
    for other, kw in others:                           # ... or in another query of the batch, in either order
        mixed = search.prepare([other, Or([p1, p2])], BM25(), st, phrase_disjunctions=True, **kw)
        assert create(mixed) == _lib.EUNSUPPORTED, other
        assert create(mixed[::-1]) == _lib.EUNSUPPORTED, other
        assert create(mixed[:1], run=True) == _lib.OK and create(mixed[1:], run=True) == _lib.OK
    bare = synth.segment_from_lists([(d, f) for d, f, _ in lists], num_docs, synth.LAYOUT_SIMD4)
    sr_bare = search.SegmentReader.from_synth(bare, L=L)
    assert create(two, reader=sr_bare) == _lib.EUNSUPPORTED                        # a segment without positions
    sr_bare.close()
    # which path ran; a plain phrase is what it is in a batch without the flag, bit for bit ------------
    flts = [by_phrase([1, 3]), Or([by_phrase([1, 3]), by_phrase([2, 5])]), by_phrase([2, 5, 1], [0, 1, 3]),
            Or([by_phrase([1, 3]), by_phrase([2, 10_000])]), Or([by_phrase([1, 10_000]), by_phrase([10_000, 2])])]
    for scorer in (BM25(), TFIDF(True)):
        prep, h, c, t, n = _run(sr, flts, scorer, 10, st)
        assert n == 3
        for q, flt in enumerate(flts):
            check(flt, 10, h[q], c[q], t[q], *expected(seg, flt, scorer))
        assert int(t[4]) == 0 and int(c[4]) == 0 and int(t[1]) >= int(t[0]) > 0 and int(t[3]) == int(t[0])
        keep = [0, 2]
        h1, c1, t1 = _plain(sr, [flts[q] for q in keep], scorer, 10, st)
        for at, q in enumerate(keep):
            assert np.array_equal(h[q], h1[at]) and c[q] == c1[at] and t[q] == t1[at], (scorer, q)
    sr.close()


def _plain(sr, filters, scorer, k, stats):
    """The plain phrases in a batch without a unit of several phrases: the default prepare."""
    b = search.QueryBatch(sr, search.prepare(filters, scorer, stats), k)
    assert b.phrase_disj_units() == 0
    res = tuple(x.copy() for x in b.run().results())
    b.close()
    return res


def case_lists(L, layout):
    """Hand-built lists (test_phrases_and.hand_lists): the matching docs of every query written down
    from their rules, the scores from the oracle."""
    N = N_LISTS
    lists = tps.hand_lists()
    norms = (np.arange(N, dtype=np.uint32) * 7 % 200 + 20).astype(np.uint8)
    seg = synth.segment_from_lists(lists, N, layout, norms=norms)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    ny, re, ab, ba = by_phrase([NEW, YORK]), by_phrase([REAL, ESTATE]), by_phrase([A, B_]), by_phrase([B_, A])
    nc = by_phrase([NEW, CITY], [0, 2])          # new@1 city@3: d % 36 == 0
    nyc = by_phrase([NEW, YORK, CITY])           # new@1 york@2 city@3: d % 36 == 0
    gap = by_phrase([NEW, YORK], [0, 4])         # new@1 .. york@5: d % 6 == 0 and d % 4 != 0
    # leads at their edges: "the" (every doc, @20) in front of a list whose docs carry @40 — one doc
    # (7, which nothing else matches; 72, which "new york" matches too), 127 docs (a tail alone), 129
    # (a block + 1) and 257 (two blocks + 1)
    t_miss, t_72 = by_phrase([THE, ONE_MISS], [0, 20]), by_phrase([THE, ONE72], [0, 20])
    t127, t129, t257 = (by_phrase([THE, t], [0, 20]) for t in (L127, L129, L257))
    docs = range(1, N + 1)
    NY = {d for d in docs if d % 12 == 0}
    RE = {d for d in docs if d % 36 in (0, 24)}
    AB = {d for d in docs if d % 7 == 0}
    BA = {d for d in docs if d % 14 == 0}
    NC = {d for d in docs if d % 36 == 0}
    GAP = {d for d in docs if d % 6 == 0 and d % 4}
    S127, S129, S257 = ({6 * i for i in range(1, 128)}, {6 * i for i in range(1, 130)},
                        {12 * i for i in range(1, 258)})
    assert RE < NY and BA < AB and (RE & AB) and (RE - AB) and (AB - RE)
    sets, set_bits = set_rows(N, [range(1, 5001), [252, 7]])
    cases = [
        # the two sets nest: d % 36 in {0, 24} is matched by both phrases and comes back once;
        # d % 36 == 12 holds all four words and matches "new york" only; both orders: ownership from
        # either side
        (Or([ny, re]), NY),
        (Or([re, ny]), NY),
        (Or([re, ab]), RE | AB),                   # sets that overlap only partly
        (Or([ab, ba]), AB),                        # the same two terms in four rows
        (Or([ab, ab]), AB),                        # the same phrase twice: counted once
        (Or([ny, re, ab, nc]), NY | AB),           # 8 rows
        (Or([nyc, ab]), NC | AB),                  # a three-word phrase next to a two-word one
        (Or([gap, ab]), GAP | AB),                 # a phrase with an offset gap
        (Or([ny, by_phrase([REAL, 10_000])]), NY),                              # an absent word: that phrase is dropped
        (Or([by_phrase([10_000, REAL]), ny], boost=2.0), NY),
        (Or([by_phrase([NEW, 10_000]), by_phrase([10_001, YORK])]), set()),     # both dropped
        (And([Or([ny, re]), Not(by_term(RARE))]), {d for d in NY if d % 90}),
        (And([Or([ny, re]), Not(by_term(10_000))]), NY),                        # an absent excluded term
        (And([Or([re, ab]), by_doc_set(0)]), {d for d in RE | AB if d <= 5000}),
        (And([Or([re, ab]), by_doc_set(1)]), {252, 7}),                         # 252: both phrases; 7: "a b"
        (Or([ny, t_miss]), NY | {7}),              # a lead of one doc that nothing else matches
        (Or([t_72, ny]), NY),                      # ... that the other phrase matches too, owned by the first
        (Or([re, t127]), RE | S127),               # a lead of 127 docs: a tail alone
        (Or([t129, ab]), S129 | AB),               # 128 + 1
        (Or([t257, t_72, t127]), S257 | {72} | S127),   # 2 * 128 + 1; every phrase leads with an edge list
        (ny, NY),
    ]
    filters = [f for f, _ in cases]
    small = [0, 1, 2, 3, 4, 8, 15, 16, 17, 18, 20]   # at most 4 rows each: a batch of them runs the <4> instantiation
    for scorer in (BM25(), TFIDF(True)):
        exp = [expected(seg, f, scorer, doc_sets=set_bits) for f in filters]
        for (flt, want), (_, matched) in zip(cases, exp):
            assert set(np.nonzero(matched)[0].tolist()) == want, ("the oracle and the hand list differ", flt)
        for pick in (range(len(cases)), small):
            pick = list(pick)
            for kk in (10, 2000):
                prep, h, c, t, n = _run(sr, [filters[q] for q in pick], scorer, kk, st, doc_sets=sets)
                assert max(len(p.terms) for p in prep) == (8 if len(pick) > len(small) else 4)
                assert n == n_disj([filters[q] for q in pick])
                for at, q in enumerate(pick):
                    flt, want = cases[q]
                    assert int(t[at]) == len(want), (flt, int(t[at]), len(want))
                    if kk == 2000 and len(want) <= kk:
                        assert set(h[at, :int(c[at])]["doc"].tolist()) == want, flt
                    check(flt, kk, h[at], c[at], t[at], *exp[q])
    # a doc both phrases match scores the sum of the two alone; each phrase's own frequency is its
    # scorer's tf: new york twice in d % 24 == 0, real estate three times in d % 36 == 0 — 72 has
    # (2, 3), 36 (1, 3), 24 (2, 1), 60 (1, 1); 12 matches "new york" alone
    _, h, c, t, _ = _run(sr, [Or([ny, re]), ny, re, Or([ab, ab]), ab, Or([re, ny])], TFIDF(False), 2000, st)
    by = [{int(x["doc"]): float(x["score"]) for x in h[q, :int(c[q])]} for q in range(6)]
    for o in (0, 5):
        assert by[o][72] > by[o][36] > by[o][60] and by[o][72] > by[o][24] > by[o][60] > by[o][12]
        for d in (24, 36, 60, 72):
            assert abs(by[o][d] - float(f32(f32(by[1][d]) + f32(by[2][d])))) <= parity.REL_TOL * by[o][d], d
        assert by[o][12] == by[1][12] and 12 not in by[2]
    assert set(by[3]) == set(by[4])
    for d, s in by[4].items():
        assert abs(by[3][d] - float(f32(f32(s) + f32(s)))) <= parity.REL_TOL * by[3][d], d
    # deleted docs among the matches: 36 matched by both phrases, 12 by "new york" alone, 7 by none
    seg2 = synth.segment_from_lists(lists, N, layout, norms=norms)
    seg2.doc_mask = np.array([7, 12, 36, 7200], np.uint32)
    sr2 = search.SegmentReader.from_synth(seg2, L=L)
    for scorer in (BM25(), TFIDF(True)):
        for flt, want in ((Or([ny, re]), NY - {12, 36, 7200}), (Or([re, ny]), NY - {12, 36, 7200}),
                          (And([Or([re, ab]), Not(by_term(RARE))]), {d for d in RE | AB if d % 90} - {7, 36, 7200})):
            sc, matched = expected(seg2, flt, scorer)
            assert set(np.nonzero(matched)[0].tolist()) == want
            for kk in (1, 2000):
                _, h, c, t, _ = _run(sr2, [flt], scorer, kk, st)
                check(flt, kk, h[0], c[0], t[0], sc, matched)
    sr.close()
    sr2.close()


def parity_filters(max_rank):
    """test_phrases_and.parity_filters with every And of phrases turned into an Or, and two boosted
    ones."""
    listed, _ = tps.parity_filters(max_rank)
    listed = [Or(list(f.subs)) for f in listed]
    more = [Or([by_phrase([0, 1], boost=1.5), by_phrase([2, 0])], boost=2.5),
            Or([by_phrase([0, 3]), by_phrase([1, 2], boost=0.5)], boost=0.8)]
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
        # the conditions of the case, from the oracle's arrays: every query has docs that all of its
        # phrases match — the counts test_phrases_and pins on the same segment —, three match beyond k
        both = [overlap(seg, f, scorer) for f in listed]
        assert both == list(counts), (both, counts)
        assert all(n > 0 for n in both)
        got = [int(m.sum()) for _, m in exp]
        assert sum(n > k for n in got) >= 3, got
        prep = prepare(filters, scorer, st)
        b = sr.batch(prep, k)
        assert b.phrase_disj_units() == len(filters)
        h, c, t = (x.copy() for x in b.run().results())
        for q, flt in enumerate(filters):
            check(flt, k, h[q], c[q], t[q], *exp[q])
        h2, c2, t2 = b.run().results()    # the batch once more: the same
        assert np.array_equal(h, h2) and np.array_equal(c, c2) and np.array_equal(t, t2), scorer
        b.close()
    sr.close()


def case_match_sets(L, num_docs, max_rank, layout):
    """Rows = the OR of match_sets(each phrase alone), minus deleted and excluded docs; counts = the
    popcounts; sets=False the same counts; a scored run afterwards agrees."""
    seg = synth.build_segment(num_docs, max_rank, layout=layout, with_positions=True)
    seg.doc_mask = np.arange(3, num_docs, 11, dtype=np.uint32)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    shapes = [([0, 1], [2, 0]), ([0, 1], [1, 0]), ([1, 4, 0], [0, 2]), ([0, 3], [1, 2]),
              ([3, 1], [0, 2], [1, 0]), ([0, 1], [2, 3], [0, 3], [1, 2]), ([0, 1], [0, 1])]
    filters = [Or([by_phrase(w) for w in ws]) for ws in shapes]
    filters.append(And([Or([by_phrase([0, 1]), by_phrase([2, 0])]), Not(by_term(3))]))
    filters.append(by_phrase([0, 1]))
    b = sr.batch(prepare(filters, BM25(), st), 10)
    assert b.phrase_disj_units() == len(filters) - 1
    nw = b.match_words()
    sets, counts = b.match_sets()
    _, counts_only = b.match_sets(sets=False)
    words = sorted({tuple(w) for ws in shapes for w in ws})
    alone = sr.batch(search.prepare([by_phrase(list(w)) for w in words], BM25(), st), 10)
    psets, _ = alone.match_sets()
    own = {w: psets[i] for i, w in enumerate(words)}
    n1 = num_docs + 1
    any_hit = 0
    for q, ws in enumerate(shapes):
        want = own[tuple(ws[0])].copy()
        for w in ws[1:]:
            want |= own[tuple(w)]
        assert np.array_equal(sets[q], want), ws
        assert int(counts[q]) == int(_bits(want, n1).sum()), ws
        any_hit += int(counts[q]) > 0
        assert np.array_equal(_bits(sets[q], n1), expected(seg, filters[q], BM25())[1]), ws
    assert any_hit >= 4
    q = len(shapes)
    want = (own[(0, 1)] | own[(2, 0)]) & ~sr.bit_union([3], nw)[0]
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
    """create_multi: a word absent from one segment — the query's other phrase goes on matching
    there —, index-global statistics, one threshold per query over the segments, the merged top k."""
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    segs = [synth.build_segment(int(n), max_rank, first_doc=int(f), with_positions=True)
            for n, f in zip(sizes, first)]
    segs[1].metas[2]["docs_count"] = 0     # word 2 absent from segment 1
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    stats = [parity.segment_stats(s) for s in segs]
    filters = [Or([by_phrase([0, 1]), by_phrase([2, 0])]), Or([by_phrase([0, 3]), by_phrase([1, 0])]),
               Or([by_phrase([1, 0, 3]), by_phrase([0, 2], boost=0.5)], boost=1.5), by_phrase([0, 1]),
               Or([by_phrase([2, 1]), by_phrase([3, 2])])]
    for scorer in (BM25(), TFIDF(True)):
        prep = prepare(filters, scorer, stats)
        # statistics are index-global: each phrase's blob from the summed docs_count of its own words
        alone = search.prepare([by_phrase([2, 0])], scorer, stats)[0]
        assert prep[0].scorers[2] == prep[0].scorers[3] == alone.scorers[0] != prep[0].scorers[0]
        for shared in (False, True):
            b = search.QueryBatch(readers, prep, k).set_shared_threshold(shared)
            assert b.phrase_disj_units() == 4 * len(segs)
            h, c, t = b.run().results()
            merged = search.merge_topk_host([(h[i], c[i]) for i in range(len(segs))], k)
            # segment 1 lacks word 2: "2 0" is dropped, "0 1" goes on matching; both phrases of the
            # last query are dropped
            assert int(t[1, 0]) == int(t[1, 3]) > 0 and int(t[1, 4]) == 0 and int(t[0, 4]) > 0
            assert int(t[0, 0]) > int(t[0, 3])
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
    """k_phrases_or on test_block_driven._misled_phrase_segment: Or(["q 2", "q . 3"]) for q = 0, 1 (4
    rows: the <4> instantiation) and Or(["q 2", "q . 3", "q 2", "q . 3"]) (8 rows).  Every phrase leads
    with q — 64 blocks —, so a unit has 64 lead items per phrase: 128 and 256.  Every lead doc matches
    every phrase, so phrase 1 owns them all and the items of the other phrases list nothing.  Stride
    16 from phase 7 * unit samples 8 (16) items: 4 of them phrase 1's, all hot — 512 docs on which
    every phrase has frequency 50, >= need = ceil(3 * 1000 * 8 / 128) = 188 and < k = 1000 of 8192
    matches: one re-run, both units short of k, results bit for bit the stride-1 batch's.  Control:
    shift 8 — the sampled blocks are cold, the threshold lets every doc through."""
    import sys

    import test_pilot_recovery as pr
    from test_block_driven import MISLED_K, STRIDE, _misled_phrase_segment
    k, scorer = MISLED_K, TFIDF(False)
    assert pr.pilot_need(k, 8, 128) == 188 and pr.pilot_need(k, 16, 256) == 188
    batches = [[Or([by_phrase([q, 2]), by_phrase([q, 3], [0, 2])]) for q in range(2)],
               [Or([by_phrase([q, 2]), by_phrase([q, 3], [0, 2]), by_phrase([q, 2]), by_phrase([q, 3], [0, 2])])
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
                       lambda b: (b.path(), b.phrase_disj_units()), capfd, reruns, [2] * reruns,
                       listed=(512, 8192) if reruns else None, what=("phrases or", len(prep[0].terms), shift))
        sr.close()


# ------------------------------------------------------------------ host only --

def test_prepare_phrases_or():
    st = [search.SegmentStats(1000, 100_000, np.arange(64, dtype=np.int64) * 3 + 20)]
    sc = BM25()
    p1, p2 = by_phrase([1, 2], [0, 3], boost=1.5), by_phrase([5, 6, 2])
    flt = Or([p1, p2], boost=2.0)
    p = search.prepare([flt], sc, st, phrase_disjunctions=True)[0]
    assert p.op == _lib.OP_PHRASE and p.terms == [1, 2, 5, 6, 2] and p.offsets == [0, 3, 0, 1, 2]
    assert p.or_opens == [False, False, True, False, False]
    assert p.opens is None and p.required is None and p.optional is None and p.alts is None and p.excluded == []
    assert p.merge == search.MERGE_SUM
    # every phrase its own blob from its own words; the Or's boost into each, in float32
    a1 = search.prepare([by_phrase([1, 2], [0, 3], boost=float(f32(f32(2.0) * f32(1.5))))], sc, st)[0]
    a2 = search.prepare([by_phrase([5, 6, 2], boost=2.0)], sc, st)[0]
    assert p.scorers[0] == p.scorers[1] == a1.scorers[0]
    assert p.scorers[2] == p.scorers[3] == p.scorers[4] == a2.scorers[0] != a1.scorers[0]
    arr = search.QueryArrays.from_prepared([type("S", (), {"metas": np.zeros(64)})()], [p], 10)
    B, O = _lib.SCORE_BM25, _lib.PHRASE_OR
    assert O == 0x4000
    assert list(arr.terms[0, :5]["kind"]) == [B, B, B | O, B, B]
    assert list(arr.terms[0, :5]["phrase_offset"]) == [0, 3, 0, 1, 2] and int(arr.queries[0]["n_terms"]) == 5
    assert list(arr.terms[0, :5]["c0"]) == [f32(s[1]) for s in p.scorers]
    # under Nots and a doc set: the way they always went
    q = search.prepare([And([flt, Not(by_term(9)), by_doc_set(3)])], sc, st, phrase_disjunctions=True)[0]
    assert q.terms == p.terms and q.excluded == [9] and q.doc_set == 3 and q.scorers == p.scorers
    assert q.or_opens == p.or_opens
    arr = search.QueryArrays.from_prepared([type("S", (), {"metas": np.zeros(64)})()], [q], 10)
    assert list(arr.terms[0, :6]["kind"]) == [B, B, B | O, B, B, _lib.EXCLUDE]
    # four phrases, 8 words
    four = search.prepare([Or([by_phrase([t, t + 1]) for t in (1, 3, 5, 7)])], sc, st, phrase_disjunctions=True)[0]
    assert four.or_opens == [False, False, True, False, True, False, True, False]
    # one phrase: nothing changes, such prepared queries compare equal to what they were
    plain = search.prepare([by_phrase([1, 2])], sc, st, phrase_disjunctions=True)[0]
    assert plain == search.PreparedQuery(_lib.OP_PHRASE, [1, 2], plain.scorers, 0, [0, 1])
    one = search.prepare([Or([p1, by_term(7)])], sc, st, optional_terms=True, phrase_disjunctions=True)[0]
    assert one.or_opens is None and one == search.prepare([Or([p1, by_term(7)])], sc, st, optional_terms=True)[0]
    # off by default: today's refusals, word for word
    with pytest.raises(ValueError, match="two phrases in one Or are not on the GPU path"):
        search.prepare([Or([p1, p2])], sc, st, optional_terms=True)
    with pytest.raises(ValueError, match="a by_phrase inside an Or is not on the GPU path"):
        search.prepare([Or([p1, p2])], sc, st)
    with pytest.raises(ValueError, match=r"phrase_disjunctions=True\), not by the array path"):
        search.prepare_filters([Or([p1, p2])], sc, st, [], 10)
    for bad, why in [(Or([by_phrase([[1, 2], 3]), p2]), "variadic by_phrase next to another phrase in an Or"),
                     (Or([p1, p2, by_term(3)]), "by_term next to several by_phrase children of an Or"),
                     (Or([p1, p2, And([by_term(3), by_term(4)])]), "And next to several by_phrase children of an Or"),
                     (Or([p1, p2, Or([by_term(3), by_term(4)])]), "Or next to several by_phrase children of an Or"),
                     (Or([p1, p2], min_match=2), "min_match > 1 is not on the GPU path"),
                     (Or([p1, p2], merge=search.MERGE_MAX), "merges with SUM"),
                     (Or([p1, p2], merge=search.MERGE_MIN), "merges with SUM"),
                     (Or([p1, by_phrase([4])]), "by_phrase of one term is a by_term"),
                     (Or([by_phrase([t, t + 1]) for t in range(1, 6)]), "more than four phrases in one Or"),
                     (Or([by_phrase([1, 2, 3]), by_phrase([4, 5, 6]), by_phrase([7, 8, 9])]),
                      "at most 8 words in all")]:
        with pytest.raises(ValueError, match=why):
            search.prepare([bad], sc, st, optional_terms=True, phrase_disjunctions=True)


def _cpp(L, tmp_path, extra=()):
    """tests/cpp/test_phrases_or.cpp: the C++ layer's Or of several by_phrases."""
    import subprocess
    from pathlib import Path
    from iresearch_amd import _build
    root = Path(__file__).resolve().parents[1]
    synth_lib = _build.build_synth()
    exe = tmp_path / "test_phrases_or"
    lib = Path(L._name)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall",
           "-I", str(root / "include"), "-I", str(root / "iresearch_amd" / "cpp"),
           "-I", str(root / "iresearch_amd" / "index"),
           str(root / "tests" / "cpp" / "test_phrases_or.cpp"), "-o", str(exe), str(lib), str(synth_lib),
           "-pthread", "-Wl,-rpath," + str(lib.parent), "-Wl,-rpath," + str(Path(synth_lib).parent), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "test_phrases_or OK" in run.stdout, (run.stdout + run.stderr)[-3000:]


SMALL = (6_000, 48, tps.SMALL[2])
LARGE = (200_000, 256, tps.LARGE[2])
assert SMALL[2] == (200, 365, 3, 48, 17, 5, 56) and LARGE[2] == (7285, 12231, 114, 1713, 616, 17, 1816)


# ---------------------------------------------------------------- emulator --

def test_phrases_or_abi_emulated(simlib):
    case_abi(simlib)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrases_or_lists_emulated(simlib, layout):
    case_lists(simlib, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrases_or_parity_emulated(simlib, layout):
    case_parity(simlib, SMALL[0], SMALL[1], layout, SMALL[2])


def test_phrases_or_match_sets_emulated(simlib):
    case_match_sets(simlib, 6_000, 48, synth.LAYOUT_SIMD4)


def test_phrases_or_multi_emulated(simlib):
    case_multi(simlib, (3_000, 1_500, 4_000))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrases_or_misled_emulated(simlib, layout, capfd):
    case_misled(simlib, layout, capfd)


def test_cpp_phrases_or_emulated(simlib, tmp_path):
    _cpp(simlib, tmp_path)


# --------------------------------------------------------------------- GPU --

@pytest.mark.gpu
def test_phrases_or_abi_gpu(gpulib):
    case_abi(gpulib)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrases_or_lists_gpu(gpulib, layout):
    case_lists(gpulib, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrases_or_parity_gpu(gpulib, layout):
    case_parity(gpulib, LARGE[0], LARGE[1], layout, LARGE[2])


@pytest.mark.gpu
def test_phrases_or_match_sets_gpu(gpulib):
    case_match_sets(gpulib, 200_000, 256, synth.LAYOUT_SIMD4)


@pytest.mark.gpu
def test_phrases_or_multi_gpu(gpulib):
    case_multi(gpulib, (60_000, 20_000, 90_000), max_rank=128, k=100)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrases_or_misled_gpu(gpulib, layout, capfd):
    case_misled(gpulib, layout, capfd)


@pytest.mark.gpu
def test_cpp_phrases_or_gpu(gpulib, tmp_path):
    rocm = "/opt/rocm/lib"
    _cpp(gpulib, tmp_path, ["-Wl,-rpath," + rocm, "-Wl,-rpath-link," + rocm, "-Wl,--allow-shlib-undefined"])
