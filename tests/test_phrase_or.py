"""Or([by_phrase, by_term...]) — a phrase or optional terms (IRS_HIP_PHRASE_OPTIONAL): the
reference's MakeDisjunction over {PhraseIterator, term iterators} (boolean_filter.cpp:150-210,
disjunction.hpp:1411-1467).

The expected value is composed from the oracle as it stands: oracle.score_all_phrase gives the
phrase frequency and phrase score of every doc, oracle.score_all with OP_OR over the optional terms
that the segment holds their union and summed scores (boosts passed); a doc matches when pf > 0 or a
term holds it, its score is the float32 sum of the two.  Deleted docs go through the segment's
doc_mask (both oracle calls apply it), excluded terms through the oracle's decoder.  One body runs on
the emulator (CPU tier) and on the GPU."""
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
    """(phrase, [(term, boost product)], excluded term ordinals) of a filter of this file: a by_phrase
    alone, an Or of one by_phrase and by_terms (SUM Ors of by_terms flattened), or
    And([that Or, Not(by_term)...])."""
    excl, mult = [], f32(1.0)
    if type(flt) is And:
        excl = [s.filter.term for s in flt.subs if isinstance(s, Not)]
        inner = [s for s in flt.subs if not isinstance(s, Not)]
        assert len(inner) == 1
        mult, flt = f32(flt.boost), inner[0]
    if isinstance(flt, by_phrase):
        return search.replace(flt, boost=float(f32(mult * f32(flt.boost)))), [], excl
    ph = [s for s in flt.subs if isinstance(s, by_phrase)]
    assert type(flt) is Or and len(ph) == 1
    mult = f32(mult * f32(flt.boost))
    rest = search.replace(flt, subs=[s for s in flt.subs if not isinstance(s, by_phrase)])
    members = search._or_members(rest, mult)
    return search.replace(ph[0], boost=float(f32(mult * f32(ph[0].boost)))), members, excl


def _present(seg, t):
    return 0 <= t < len(seg.metas) and int(seg.metas[t]["docs_count"]) > 0


def expected(seg, flt, scorer, all_segs=None):
    """(scores f32[num_docs + 1], matched bool[num_docs + 1]) of `flt` on `seg`; statistics over
    `all_segs` (default: this segment)."""
    all_segs = all_segs or [seg]
    ph, members, excl = split(flt)
    osc = parity.oracle_scorer(scorer)
    view = parity.oracle_view(seg)
    dwf = sum(s.docs_with_field for s in all_segs)
    ttf = sum(s.total_term_freq for s in all_segs)
    n1 = seg.num_docs + 1

    def dwt(ts):
        return [sum(int(s.metas[t]["docs_count"]) if 0 <= t < len(s.metas) else 0 for s in all_segs)
                for t in ts]
    scores, matched = np.zeros(n1, f32), np.zeros(n1, bool)
    if all(_present(seg, t) for t in ph.terms):   # (an absent word empties the phrase child only)
        sc, pf = oracle.score_all_phrase(view, parity.metas_for(seg, ph.terms), ph.offsets, osc, dwf,
                                         dwt(ph.terms), ttf, float(ph.boost))
        matched = pf[:n1] > 0
        scores = np.where(matched, sc[:n1].astype(f32), f32(0)).astype(f32)
    here = [(t, b) for t, b in members if _present(seg, t)]   # (an absent term adds nothing)
    if here:
        ot = [t for t, _ in here]
        ts, tm = oracle.score_all(view, parity.metas_for(seg, ot), oracle.OP_OR, osc, dwf, dwt(ot), ttf,
                                  [f32(b) for _, b in here])
        tm = tm[:n1].astype(bool)
        scores = (scores + np.where(tm, ts[:n1].astype(f32), f32(0))).astype(f32)
        matched = matched | tm
    wc = int(getattr(seg, "wand_count", 0))
    for t in excl:
        if _present(seg, t):
            d, _ = oracle.decode_term(seg.doc_file, seg.metas[t], seg.layout, wand_count=wc)
            matched[d.astype(np.int64)] = False
    matched[0] = False
    scores[~matched] = 0
    return scores, matched


def check(flt, k, h, c, t, scores, matched):
    """As check() of test_phrase_and.py: total hits and doc sets exactly, scores to REL_TOL, order
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


def _prep(filters, scorer, stats):
    return search.prepare(filters, scorer, stats, optional_terms=True)


def _run(sr, filters, scorer, k, stats, tile_docs=0, cand_cap=0):
    prep = _prep(filters, scorer, stats)
    b = sr.batch(prep, k)
    if tile_docs or cand_cap:
        b.configure(tile_docs=tile_docs, cand_cap=cand_cap)
    h, c, t = (x.copy() for x in b.run().results())
    reruns = b.reruns()
    b.close()
    return prep, h, c, t, reruns


# -------------------------------------------------------------------- cases --

def case_abi(L):
    """IRS_HIP_PHRASE_OPTIONAL validation at batch create, the flag's refusals, a plain phrase next
    to a unit with optional terms, Or([phrase]) alone, doc sets refused."""
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

    O, R, A = _lib.PHRASE_OPTIONAL, _lib.PHRASE_REQUIRED, _lib.PHRASE_ALT
    assert O == 0x800
    good = _prep([Or([by_phrase([1, 2, 3]), by_term(4), by_term(5, 2.0)])], BM25(), st)
    assert good[0].optional == [False, False, False, True, True]
    assert create(good) == _lib.OK
    kinds = search.QueryArrays.from_prepared([sr], good, 10).terms[0, :5]["kind"]
    assert list(kinds) == [_lib.SCORE_BM25] * 3 + [_lib.SCORE_BM25 | O] * 2

    def edit(**kw):
        def f(arr):
            for name, changes in kw.items():
                for j, v in changes.items():
                    arr.terms[0, j][name] = v
        return f
    B = _lib.SCORE_BM25
    # an unflagged entry behind a flagged one; the flag on the first entry; one word only
    assert create(good, edit(kind={2: B | O, 3: B})) == _lib.EINVAL    # w w O w O
    assert create(good, edit(kind={0: B | O})) == _lib.EINVAL          # O w w O O
    assert create(good, edit(kind={1: B | O, 2: B | O})) == _lib.EINVAL   # w O O O O
    # the flag on a non-phrase op
    for op in (_lib.OP_OR, _lib.OP_AND, _lib.OP_MINMATCH):
        def other_op(arr, op=op):
            arr.queries[0]["op"] = op
            arr.queries[0]["min_match"] = 2
        assert create(good, other_op) == _lib.EINVAL, op
    # ... and on an excluded entry
    with_not = _prep([And([Or([by_phrase([1, 2]), by_term(4)]), Not(by_term(6))])], BM25(), st)
    assert with_not[0].excluded == [6] and with_not[0].optional == [False, False, True]
    assert create(with_not) == _lib.OK
    assert create(with_not, edit(kind={3: _lib.EXCLUDE | O})) == _lib.EINVAL
    # its own scorer values, validated like a by_term's; the phrase offset ignored
    assert create(good, edit(c0={3: -1.0})) == _lib.EINVAL
    assert create(good, edit(c0={4: float("nan")})) == _lib.EINVAL
    assert create(good, edit(kind={3: 7 | O})) == _lib.EINVAL
    assert create(good, edit(kind={3: _lib.SCORE_TFIDF | O})) == _lib.OK
    assert create(good, edit(term={3: len(lists)})) == _lib.EINVAL
    assert create(good, edit(phrase_offset={3: 77, 4: 5})) == _lib.OK
    # the phrase's words still carry ONE scorer
    assert create(good, edit(c0={1: 0.5})) == _lib.EINVAL
    # merge stays SUM
    def merge_max(arr):
        arr.queries[0]["merge"] = search.MERGE_MAX
    assert create(good, merge_max) == _lib.EINVAL
    # 8 entries are fine, 9 are not supported
    eight = _prep([Or([by_phrase([1, 2, 3])] + [by_term(t) for t in range(4, 9)])], BM25(), st)
    assert create(eight) == _lib.OK
    nine = _prep([Or([by_phrase([1, 2, 3])] + [by_term(t) for t in range(4, 9)])], BM25(), st)
    nine[0].terms.append(9)
    nine[0].scorers.append(nine[0].scorers[-1])
    nine[0].offsets.append(0)
    nine[0].optional.append(True)
    assert create(nine) == _lib.EUNSUPPORTED
    # mixed with required terms or a variadic part: in one unit, and in one batch
    assert create(good, edit(kind={3: B | R})) == _lib.EUNSUPPORTED          # w w w R O
    assert create(good, edit(kind={3: B | R | O})) == _lib.EUNSUPPORTED
    assert create(good, edit(kind={1: B | A})) == _lib.EUNSUPPORTED          # w a w O O
    req = search.prepare([And([by_phrase([1, 2]), by_term(4)])], BM25(), st, required_terms=True)
    var = search.prepare([by_phrase([[1, 2], 3])], BM25(), st)
    for other in (req, var):
        assert create(good + other) == _lib.EUNSUPPORTED
        assert create(other + good) == _lib.EUNSUPPORTED

    # a plain phrase in the batch is bit for bit what it is in a batch without optional units;
    # Or([phrase]) alone is the phrase; an absent optional term adds nothing, an absent word leaves
    # the terms, everything absent is empty
    flts = [Or([by_phrase([1, 3]), by_term(4)]), Or([by_phrase([1, 3]), by_term(10_000)]),
            by_phrase([1, 3]), Or([by_phrase([1, 3]), by_term(4), by_term(7)]), by_phrase([2, 5, 1], [0, 1, 3]),
            Or([by_phrase([1, 3])]), Or([by_phrase([1, 10_000]), by_term(4)]),
            Or([by_phrase([10_000, 1]), by_term(10_001)])]
    for scorer in (BM25(), TFIDF(True)):
        prep, h, c, t, _ = _run(sr, flts, scorer, 10, st)
        assert prep[5].optional is None and prep[5] == prep[2]
        for q, flt in enumerate(flts):
            check(flt, 10, h[q], c[q], t[q], *expected(seg, flt, scorer))
        assert int(t[7]) == 0 and int(c[7]) == 0
        assert int(t[6]) == 900 and int(t[3]) > int(t[0]) > int(t[2]) > 0
        _, h1, c1, t1, _ = _run(sr, [flts[2], flts[4]], scorer, 10, st)
        for a, b in ((2, 0), (4, 1), (5, 0), (1, 0)):
            assert np.array_equal(h[a], h1[b]) and c[a] == c1[b] and t[a] == t1[b], (scorer, a)
    # doc sets on a batch with optional units: refused (the term pass's doc sets are the phrase pass's)
    b = sr.batch(_prep(flts[:3], BM25(), st), 10)
    rows = np.full((1, num_docs // 64 + 1), ~np.uint64(0), np.uint64)
    with pytest.raises(Exception, match="(?i)unsupported|not supported"):
        b.set_doc_sets(rows, np.zeros(3, np.uint32))
    h, c, t = b.run().results()      # (and the batch is what it was)
    check(flts[0], 10, h[0], c[0], t[0], *expected(seg, flts[0], BM25()))
    b.close()
    sr.close()


N_LISTS = 5004
(NEW, YORK, HOTEL, CHEAP, EXCL, SAME) = range(6)


def hand_lists():
    """term -> (docs, freqs, positions), every list a rule of arithmetic on the doc id so that the
    matches can be written down: "new york" is in d % 12 == 0 (twice in d % 24 == 0); d % 6 == 0 has
    both words, but york 3 positions late unless d % 4 == 0.  "new" (the lead: 1668 docs) ends in a
    tail of 4 docs, the last of them (5004) a phrase match; hotel has 7 blocks and a tail of 104."""
    N = N_LISTS
    T = {
        NEW: {d: [1, 10] for d in range(3, N + 1, 3)},
        YORK: {d: ([2, 11] if d % 24 == 0 else [2] if d % 4 == 0 else [5]) for d in range(2, N + 1, 2)},
        HOTEL: {d: list(range(30, 31 + d % 3)) for d in range(5, N + 1, 5)},     # 1000 docs, tf 1..3
        CHEAP: {d: [50] for d in range(7, N + 1, 7)},                            # 714 docs
        # excluded: a phrase-only doc (24), a term-only doc (10), one with both (120), one with neither
        EXCL: {10: [60], 24: [60], 120: [60], 4999: [60]},
        # (tie order) tf 1 where hotel has tf 1: d % 15 == 0 — given the phrase's scorer in case_lists
        SAME: {d: [70] for d in range(5, N + 1, 5)},
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
    hand_lists(), the scores from the oracle; the term pass on the smallest doc tile (4096: docs in
    two tiles)."""
    N = N_LISTS
    lists = hand_lists()
    norms = (np.arange(N, dtype=np.uint32) * 7 % 200 + 20).astype(np.uint8)
    seg = synth.segment_from_lists(lists, N, layout, norms=norms)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    ny = by_phrase([NEW, YORK])
    docs = range(1, N + 1)
    phrase = {d for d in docs if d % 12 == 0}
    hotel = {d for d in docs if d % 5 == 0}
    cheap = {d for d in docs if d % 7 == 0}
    assert 5004 in phrase and 6 not in phrase | hotel | cheap and 30 in hotel - phrase and 60 in hotel & phrase
    cases = [
        (Or([ny, by_term(HOTEL)]), phrase | hotel),
        (Or([by_term(CHEAP, 0.5), ny, Or([by_term(HOTEL)], boost=1.5)], boost=2.0), phrase | hotel | cheap),
        (Or([ny, by_term(HOTEL), by_term(10_000)]), phrase | hotel),            # an absent term
        (Or([by_phrase([NEW, 10_000]), by_term(HOTEL)]), hotel),                # an absent word
        (Or([by_phrase([NEW, 10_000]), by_term(10_001)]), set()),               # everything absent
        (Or([ny, by_term(YORK, 0.5)]), {d for d in docs if d % 2 == 0}),        # a word as a term
        (Or([by_phrase([NEW, YORK], [0, 4]), by_term(CHEAP)]), {d for d in docs if d % 6 == 0 and d % 4 != 0} | cheap),
        (And([Or([ny, by_term(HOTEL)]), Not(by_term(EXCL))], boost=1.25), (phrase | hotel) - {10, 24, 120}),
        (ny, phrase),
    ]
    filters = [f for f, _ in cases]
    n_phrase, n_all = len(phrase), len(phrase | hotel)
    assert n_phrase == 417 and n_all == 1334
    for scorer in (BM25(), TFIDF(True)):
        exp = [expected(seg, f, scorer) for f in filters]
        for (flt, want), (_, matched) in zip(cases, exp):
            assert set(np.nonzero(matched)[0].tolist()) == want, ("the oracle and the hand list differ", flt)
        # 30: every word, not adjacent, and hotel: the term's score alone
        alone = expected(seg, Or([by_phrase([NEW, 10_000]), by_term(HOTEL)]), scorer)[0]
        assert exp[0][0][30] == alone[30] > 0 and exp[0][0][60] > alone[60] > 0
        # k below the phrase's matches, between them and all matches, above all matches
        for k in (5, 1000, 2000):
            assert k < n_phrase or n_phrase < k < n_all or k > n_all
            prep, h, c, t, _ = _run(sr, filters, scorer, k, st, tile_docs=4096)
            for q, (flt, want) in enumerate(cases):
                assert int(t[q]) == len(want), (flt, int(t[q]), len(want))
                if k == 2000 and len(want) <= k:
                    assert set(h[q, :int(c[q])]["doc"].tolist()) == want, flt
                check(flt, k, h[q], c[q], t[q], *exp[q])
        # candidate overflow in both passes: as many slots as k, re-run, the same results
        prep, h, c, t, reruns = _run(sr, filters[:2], scorer, 64, st, tile_docs=4096, cand_cap=64)
        assert reruns >= 1
        for q in range(2):
            check(filters[q], 64, h[q], c[q], t[q], *exp[q])
    # deleted docs of each kind (phrase only, term only, both) next to excluded ones
    seg2 = synth.segment_from_lists(lists, N, layout, norms=norms)
    seg2.doc_mask = np.array([5, 12, 60, 5004], np.uint32)
    sr2 = search.SegmentReader.from_synth(seg2, L=L)
    flt = And([Or([ny, by_term(HOTEL)]), Not(by_term(EXCL))])
    want = (phrase | hotel) - {10, 24, 120} - {5, 12, 60, 5004}
    for scorer in (BM25(), TFIDF(True)):
        sc, matched = expected(seg2, flt, scorer)
        assert set(np.nonzero(matched)[0].tolist()) == want
        for k in (5, 2000):
            prep, h, c, t, _ = _run(sr2, [flt, Or([ny, by_term(HOTEL)])], scorer, k, st, tile_docs=4096)
            assert prep[0].excluded == [EXCL]
            check(flt, k, h[0], c[0], t[0], sc, matched)
            check(flt, k, h[1], c[1], t[1], *expected(seg2, Or([ny, by_term(HOTEL)]), scorer))
            assert int(t[1]) == n_all - 4
    sr2.close()
    # equal scores, one doc from each pass: the term SAME given the phrase's own scorer (TF-IDF
    # without norms: c0 * sqrt(tf)) — a doc with the phrase once and no term (12) and a doc with the
    # term once and no phrase (5) score alike, bit for bit; ties go by doc id across the two passes
    prep = _prep([Or([ny, by_term(SAME)])], TFIDF(False), st)
    prep[0].scorers[2] = prep[0].scorers[0]
    b = sr.batch(prep, 2000).configure(tile_docs=4096)
    h, c, t = b.run().results()
    b.close()
    n = int(c[0])
    assert n == n_all == int(t[0])
    d, s = h[0, :n]["doc"].astype(np.int64), h[0, :n]["score"]
    assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (d[:-1] < d[1:]))).all()
    c0 = f32(prep[0].scorers[0][1])
    once = (d % 24 != 0) & ((d % 12 == 0) != (d % 5 == 0))    # the phrase once, or the term: c0
    assert (s[once] == c0).all() and int(once.sum()) > 800
    tied = d[once]
    assert (np.diff(tied) > 0).all() and {5, 12} <= set(tied[:4].tolist())
    from_phrase = tied % 12 == 0
    assert (from_phrase[:-1] != from_phrase[1:]).sum() > 100    # the passes' docs interleave
    sr.close()


def random_queries(seg, max_rank, n, seed):
    """2-3 phrase words (frequent: phrases that occur), offsets with gaps, 1-4 optional terms from
    frequent and from rare ranks, some nested in a SUM Or, some excluded terms."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        nw = int(rng.integers(2, 4))
        words = [int(x) for x in rng.integers(0, 10, nw)]
        offs = [0]
        for _ in range(nw - 1):
            offs.append(offs[-1] + int(rng.integers(1, 3)))
        no = int(rng.integers(1, 5))
        lo, hi = (0, 12) if i % 2 else (max_rank // 2, max_rank)     # frequent / rare
        opt = [int(x) for x in rng.choice(np.arange(lo, hi), no, replace=False)]
        subs = [by_phrase(words, offs, boost=1.0 if i % 5 else 1.5)] + [by_term(t, 1.0 if i % 3 else 0.75) for t in opt]
        if no >= 3 and i % 4 == 0:
            subs = subs[:2] + [Or(subs[2:], boost=0.5)]
        order = rng.permutation(len(subs))
        flt = Or([subs[j] for j in order], boost=2.5 if i % 7 == 0 else 1.0)
        if i % 6 == 0:
            flt = And([flt, Not(by_term(int(rng.integers(0, max_rank))))])
        out.append(flt)
    return out


def case_parity(L, num_docs, max_rank, layout, n_queries=64, seed=29):
    seg = synth.build_segment(num_docs, max_rank, layout=layout, with_positions=True)
    seg.doc_mask = np.arange(5, num_docs, 97, dtype=np.uint32)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    filters = random_queries(seg, max_rank, n_queries, seed)
    both = 0
    for scorer in (BM25(), TFIDF(True)):
        exp = [expected(seg, f, scorer) for f in filters]
        alone = [expected(seg, split(f)[0], scorer)[1] for f in filters]
        both += sum(int(a.sum()) > 0 and int(m.sum()) > int(a.sum()) for a, (_, m) in zip(alone, exp))
        for k in (10, 100):
            b = sr.batch(_prep(filters, scorer, st), k)
            h, c, t = (x.copy() for x in b.run().results())
            for q, flt in enumerate(filters):
                check(flt, k, h[q], c[q], t[q], *exp[q])
            h2, c2, t2 = b.run().results()    # the batch once more: the same
            assert np.array_equal(h, h2) and np.array_equal(c, c2) and np.array_equal(t, t2), (scorer, k)
            b.close()
    assert both >= n_queries, "few queries match through both children: the case checks little"
    sr.close()


def _bits(row, n1):
    return np.unpackbits(row.view(np.uint8), bitorder="little")[:n1].astype(bool)


def case_match_sets(L, num_docs, max_rank, layout):
    """Rows = match_sets(the phrase alone) | bit_union(optional terms), minus deleted and excluded
    docs = the oracle's `matched`; counts = the popcounts; sets=False the same counts; the totals of
    a scored run the same — before the first run and after it."""
    seg = synth.build_segment(num_docs, max_rank, layout=layout, with_positions=True)
    seg.doc_mask = np.arange(3, num_docs, 11, dtype=np.uint32)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    hi = max_rank - 1
    shapes = [([1, 2], [0]), ([0, 3], [5, 2]), ([2, 1, 0], [4]), ([3, 0], [hi, 1]), ([1, 0], [hi - 1]),
              ([4, 2], [0, 1, 3, 5, 6, 7]), ([0, 1], [1]), ([1, 10_000], [hi]), ([1, 2], [10_000])]
    filters = [Or([by_phrase(w)] + [by_term(t) for t in r]) for w, r in shapes]
    filters.append(And([Or([by_phrase([1, 2]), by_term(hi)]), Not(by_term(3))]))
    filters.append(by_phrase([1, 2]))
    b = sr.batch(_prep(filters, BM25(), st), 10)
    nw = b.match_words()
    n1 = num_docs + 1
    exp = [expected(seg, f, BM25())[1] for f in filters]
    alone = sr.batch(_prep([by_phrase([1, 2])], BM25(), st), 10)
    psets, _ = alone.match_sets()
    alone.close()
    for turn in range(2):
        sets, counts = b.match_sets()
        _, counts_only = b.match_sets(sets=False)
        for q, flt in enumerate(filters):
            assert np.array_equal(_bits(sets[q], n1), exp[q]), (turn, flt)
            assert int(counts[q]) == int(exp[q].sum()), (turn, flt)
        assert np.array_equal(counts, counts_only)
        assert np.array_equal(sets[len(filters) - 1], psets[0])       # the plain phrase of the batch
        assert np.array_equal(sets[8], psets[0])                      # an absent term: the phrase
        assert not _bits(sets[0], n1)[seg.doc_mask.astype(np.int64)].any()
        # a scored run of the same batch agrees with the counts (and the sets after it with the above)
        h, c, t = b.run().results()
        assert np.array_equal(t.astype(np.uint64), counts)
    b.close()
    sr.close()


def case_multi(L, sizes, max_rank=64, k=50):
    """create_multi: a word absent from one segment, an optional term from another, index-global
    statistics, the merged top k — with a threshold per unit and with one per query."""
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    segs = [synth.build_segment(int(n), max_rank, first_doc=int(f), with_positions=True)
            for n, f in zip(sizes, first)]
    segs[1].metas[5]["docs_count"] = 0     # optional term 5 absent from segment 1
    segs[2].metas[2]["docs_count"] = 0     # phrase word 2 absent from segment 2
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    stats = [parity.segment_stats(s) for s in segs]
    filters = [Or([by_phrase([0, 1]), by_term(5)]), Or([by_term(max_rank - 2), by_phrase([2, 0], [0, 2])]),
               Or([by_phrase([1, 0, 3]), by_term(max_rank - 1), by_term(5)], boost=1.5), by_phrase([0, 1]),
               And([Or([by_phrase([2, 1]), by_term(5)]), Not(by_term(7))])]
    dwf = sum(s.docs_with_field for s in segs)
    ttf = sum(s.total_term_freq for s in segs)
    for scorer in (BM25(), TFIDF(True)):
        prep = _prep(filters, scorer, stats)
        # statistics are index-global: the optional term's scorer from the summed docs_count
        dwt5 = sum(int(s.metas[5]["docs_count"]) for s in segs)
        assert prep[0].scorers[2] == scorer.term_scorer(scorer.collect(dwf, dwt5, ttf), f32(1.0))
        exp = [[expected(s, flt, scorer, segs) for s in segs] for flt in filters]
        # segment 2 lacks word 2: queries 1 and 4 match there through their term alone; segment 1
        # lacks term 5: query 4 is its phrase there
        for q in (1, 4):
            gone = Or([by_phrase([10_000, 10_001]), by_term(split(filters[q])[1][0][0])])
            assert np.array_equal(exp[q][2][1] | expected(segs[2], gone, scorer, segs)[1], expected(segs[2], gone, scorer, segs)[1])
            assert exp[q][2][1].any()
        assert np.array_equal(exp[4][1][1], expected(segs[1], And([by_phrase([2, 1]), Not(by_term(7))]), scorer, segs)[1])
        for shared in (False, True):
            b = search.QueryBatch(readers, prep, k)
            if shared:
                b.set_shared_threshold(True)
            h, c, t = b.run().results()
            merged = search.merge_topk_host([(h[i], c[i]) for i in range(len(segs))], k)
            for q, flt in enumerate(filters):
                rows = []
                for i, s in enumerate(segs):
                    sc, m = exp[q][i]
                    if shared:   # (a unit lists what may reach the query's top k: the totals stay exact)
                        assert int(t[i, q]) == int(m.sum()), (q, i)
                    else:
                        check(flt, k, h[i, q], c[i, q], t[i, q], sc, m)
                    rows += [(-float(sc[d]), i, int(d)) for d in np.nonzero(m)[0]]
                rows.sort()
                ref = np.array([-a for a, _, _ in rows[:k]])
                got = np.array([r[0] for r in merged[q]])
                assert len(got) == len(ref), (q, shared, len(got), len(ref))
                assert np.allclose(got, ref, rtol=parity.REL_TOL, atol=0), (q, shared)
            b.close()
    for r in readers:
        r.close()


# ------------------------------------------------------------------ host only --

def test_prepare_phrase_or():
    st = [search.SegmentStats(1000, 100_000, np.arange(64, dtype=np.int64) * 3 + 20)]
    sc = BM25()
    ph = by_phrase([1, 2], [0, 3], boost=1.5)
    flt = Or([by_term(7, 0.5), ph, Or([by_term(4), by_term(6, 3.0)], boost=0.25)], boost=2.0)
    p = search.prepare([flt], sc, st, optional_terms=True)[0]
    assert p.op == _lib.OP_PHRASE and p.terms == [1, 2, 7, 4, 6] and p.offsets == [0, 3, 0, 0, 0]
    assert p.optional == [False, False, True, True, True] and p.required is None and p.alts is None
    assert p.merge == search.MERGE_SUM and p.excluded == []
    # the phrase's blob from its own words, each by_term its own collect; the boosts multiplied down
    # the tree in float32
    alone = search.prepare([by_phrase([1, 2], [0, 3], boost=float(f32(f32(2.0) * f32(1.5))))], sc, st)[0]
    assert p.scorers[0] == p.scorers[1] == alone.scorers[0]
    inner = f32(f32(2.0) * f32(0.25))
    for j, t, boost in ((2, 7, f32(f32(2.0) * f32(0.5))), (3, 4, f32(inner * f32(1.0))), (4, 6, f32(inner * f32(3.0)))):
        want = sc.term_scorer(sc.collect(1000, int(st[0].docs_count[t]), 100_000), boost)
        assert p.scorers[j] == want, (j, p.scorers[j], want)
    # under And([Or, Not...]): the And's boost into the Or's, the Nots as excluded entries
    q = search.prepare([And([Not(by_term(9)), Or([ph, by_term(7)], boost=2.0)], boost=0.5)], sc, st,
                       optional_terms=True)[0]
    assert q.terms == [1, 2, 7] and q.excluded == [9] and q.optional == [False, False, True]
    assert q.scorers[2] == sc.term_scorer(sc.collect(1000, int(st[0].docs_count[7]), 100_000),
                                          f32(f32(f32(0.5) * f32(2.0)) * f32(1.0)))
    arr = search.QueryArrays.from_prepared([type("S", (), {"metas": np.zeros(64)})()], [q], 10)
    O = _lib.PHRASE_OPTIONAL
    assert O == 0x800
    assert list(arr.terms[0, :4]["kind"]) == [_lib.SCORE_BM25, _lib.SCORE_BM25, _lib.SCORE_BM25 | O, _lib.EXCLUDE]
    assert list(arr.terms[0, :3]["phrase_offset"]) == [0, 3, 0] and int(arr.queries[0]["n_terms"]) == 4
    # an Or of the phrase alone is the phrase; other queries are what they were
    one = search.prepare([Or([by_phrase([1, 2])])], sc, st, optional_terms=True)[0]
    assert one.optional is None and one == search.prepare([by_phrase([1, 2])], sc, st)[0]
    plain = [Or([by_term(1), by_term(2)]), And([by_term(1), by_term(2)]), by_phrase([1, 2])]
    assert search.prepare(plain, sc, st, optional_terms=True) == search.prepare(plain, sc, st)
    for bad, why in [(Or([by_phrase([[1, 2], 3]), by_term(5)]), "variadic by_phrase with optional terms"),
                     (Or([by_phrase([1, 2]), by_phrase([3, 4]), by_term(5)]), "two phrases"),
                     (Or([by_phrase([1, 2]), And([by_term(3), by_term(4)])]), "And child"),
                     (Or([by_phrase([1, 2]), by_term(3), by_term(4)], min_match=2), "min_match > 1"),
                     (Or([by_phrase([1, 2]), by_term(3)], merge=search.MERGE_MAX), "merges with SUM"),
                     (Or([by_phrase([1, 2, 3])] + [by_term(t) for t in range(4, 10)]), "at most 8 entries"),
                     (Or([by_phrase([1, 2]), Or([by_term(3), by_phrase([4, 5])])]), "by_phrase inside an Or"),
                     (Or([by_phrase([1, 2]), Not(by_term(3))]), "Not child")]:
        with pytest.raises(ValueError, match=why):
            search.prepare([bad], sc, st, optional_terms=True)
    # the shape is asked for: without optional_terms=True prepare() refuses it as it always did
    for kw in ({}, {"required_terms": True}):
        with pytest.raises(ValueError, match="by_phrase inside an Or is not on the GPU path"):
            search.prepare([Or([by_phrase([1, 2]), by_term(3)])], sc, st, **kw)
        with pytest.raises(ValueError, match="by_phrase inside an Or is not on the GPU path"):
            search.prepare([And([Or([by_phrase([1, 2]), by_term(3)]), Not(by_term(4))])], sc, st, **kw)


def _cpp(L, tmp_path, extra=()):
    """tests/cpp/test_phrase_or.cpp: the C++ layer's Or of a by_phrase and by_terms."""
    import subprocess
    from pathlib import Path
    from iresearch_amd import _build
    root = Path(__file__).resolve().parents[1]
    synth_lib = _build.build_synth()
    exe = tmp_path / "test_phrase_or"
    lib = Path(L._name)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall",
           "-I", str(root / "include"), "-I", str(root / "iresearch_amd" / "cpp"),
           "-I", str(root / "iresearch_amd" / "index"),
           str(root / "tests" / "cpp" / "test_phrase_or.cpp"), "-o", str(exe), str(lib), str(synth_lib),
           "-pthread", "-Wl,-rpath," + str(lib.parent), "-Wl,-rpath," + str(Path(synth_lib).parent), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "test_phrase_or OK" in run.stdout, (run.stdout + run.stderr)[-3000:]


# ---------------------------------------------------------------- emulator --

def test_phrase_or_abi_emulated(simlib):
    case_abi(simlib)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_phrase_or_lists_emulated(simlib, layout):
    case_lists(simlib, layout)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_phrase_or_parity_emulated(simlib, layout):
    case_parity(simlib, 20_000, 64, layout)


def test_phrase_or_match_sets_emulated(simlib):
    case_match_sets(simlib, 6_000, 48, synth.LAYOUT_SIMD4)


def test_phrase_or_multi_emulated(simlib):
    case_multi(simlib, (3_000, 1_500, 4_000))


def test_cpp_phrase_or_emulated(simlib, tmp_path):
    _cpp(simlib, tmp_path)


# --------------------------------------------------------------------- GPU --

@pytest.mark.gpu
def test_phrase_or_abi_gpu(gpulib):
    case_abi(gpulib)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_phrase_or_lists_gpu(gpulib, layout):
    case_lists(gpulib, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_phrase_or_parity_gpu(gpulib, layout):
    case_parity(gpulib, 60_000, 128, layout)


@pytest.mark.gpu
def test_phrase_or_match_sets_gpu(gpulib):
    case_match_sets(gpulib, 60_000, 128, synth.LAYOUT_SIMD4)


@pytest.mark.gpu
def test_phrase_or_multi_gpu(gpulib):
    case_multi(gpulib, (30_000, 10_000, 45_000), max_rank=128, k=100)


@pytest.mark.gpu
def test_cpp_phrase_or_gpu(gpulib, tmp_path):
    rocm = "/opt/rocm/lib"
    _cpp(gpulib, tmp_path, ["-Wl,-rpath," + rocm, "-Wl,-rpath-link," + rocm, "-Wl,--allow-shlib-undefined"])
