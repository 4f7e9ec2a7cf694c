"""The device's cache of decoded posting streams (stream_cache.h): k_join's output for a (segment,
term) is kept across batches, a batch that references a held stream decodes nothing for it.

Every comparison is np.array_equal on hits, counts and totals against the SAME batch run with the
cache off (budget 0), and that cache-off run is first checked against the oracle.  Every batch is
forced onto PATH_JOINED.  Segments: 60 000 docs x 256 ranks (five doc tiles), plus 9 000 docs where
a second one is needed.  One body per case, on the emulator (CPU tier) and on the GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import parity
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, TFIDF, And, Or, by_term

K = 50
_SEGS = {}   # built once for both tiers


def _seg(n_docs=60_000, first_doc=0):
    key = (n_docs, first_doc)
    if key not in _SEGS:
        _SEGS[key] = synth.build_segment(n_docs, 256, first_doc=first_doc)
    return _SEGS[key]


class _Budget:
    """The cache emptied and its budget set for a case; the budget the process had comes back."""

    def __init__(self, L, nbytes=None):
        self.L, self.nbytes = L, nbytes

    def __enter__(self):
        self.before = search.stream_cache_stats(self.L)["budget"]
        _lib.check(self.L, self.L.irs_hip_device_trim(0), "irs_hip_device_trim")
        assert search.stream_cache_stats(self.L)["bytes_held"] == 0
        if self.nbytes is not None:
            search.set_stream_cache(self.nbytes, self.L)
        return self

    def __exit__(self, *exc):
        search.set_stream_cache(self.before, self.L)
        return False


def _terms(filters):
    out = set()
    for f in filters:
        out |= {s.term for s in search._terms_of(f)[1]}
    return out


def _run(readers, prep, k=K, stream=None, shared=None):
    b = search.QueryBatch(readers, prep, k).set_path(_lib.PATH_JOINED)
    if shared is not None:
        b.set_shared_threshold(shared)
    return b.run(stream)


def _same(a, b, what=None):
    for x, y, name in zip(a, b, ("hits", "counts", "totals")):
        assert np.array_equal(x, y), (name, what)


def _read(b):
    out = [x.copy() for x in b.results()]
    assert b.path() == _lib.PATH_JOINED
    return out


def _off_reference(L, sr, seg, filters, scorer, k=K):
    """The batch with the cache off, checked against the oracle; decodes every stream itself."""
    prep = search.prepare(filters, scorer, [parity.segment_stats(seg)])
    before = search.stream_cache_stats(L)
    search.set_stream_cache(0, L)
    b = _run(sr, prep, k)
    ref = _read(b)
    distinct, decoded = b.stream_counts()
    assert decoded == distinct == len(_terms(filters))
    _same(ref, b.run().results(), "off, replayed")
    assert b.stream_counts() == (distinct, distinct)
    b.close()
    after = search.stream_cache_stats(L)
    assert (after["hits"], after["misses"], after["bytes_held"]) == (before["hits"], before["misses"], 0)
    search.set_stream_cache(before["budget"], L)
    parity.check_single_segment(seg, filters, scorer, k, *ref)
    return prep, ref


def _query_sets():
    """A and B share about half their terms; a conjunction and a min-match unit of each share
    streams with its disjunctions."""
    a = [Or([by_term(t) for t in row]) for row in ((10, 3, 5, 40, 90, 130), (11, 7, 40, 64, 200), (12, 3, 90, 17))]
    a += [And([by_term(3), by_term(40)]), Or([by_term(5), by_term(7), by_term(90)], min_match=2), by_term(64)]
    b = [Or([by_term(t) for t in row]) for row in ((10, 3, 6, 41, 90, 131), (11, 8, 40, 65, 201), (9, 3, 91, 17))]
    b += [And([by_term(3), by_term(41)]), Or([by_term(6), by_term(8), by_term(90)], min_match=2), by_term(65)]
    return a, b


def case_warm_cold_off(L):
    seg = _seg()
    sr = search.SegmentReader.from_synth(seg, L=L)
    fa, fb = _query_sets()
    ta, tb = _terms(fa), _terms(fb)
    assert len(ta & tb) * 2 >= len(tb) - 2 and len(tb - ta) >= 4
    with _Budget(L, 64 << 20):
        prep_a, ref_a = _off_reference(L, sr, seg, fa, BM25())
        prep_b, ref_b = _off_reference(L, sr, seg, fb, BM25())
        prep_t, ref_t = _off_reference(L, sr, seg, fa, TFIDF(True))
        s0 = search.stream_cache_stats(L)
        looked = 0
        # cold A decodes everything, B only what A lacked, A again nothing
        for what, prep, ref, terms, decodes in (("cold A", prep_a, ref_a, ta, len(ta)),
                                                ("B", prep_b, ref_b, tb, len(tb - ta)),
                                                ("warm A", prep_a, ref_a, ta, 0),
                                                # the entries are scorer-independent
                                                ("TF-IDF A", prep_t, ref_t, ta, 0),
                                                ("warm B", prep_b, ref_b, tb, 0)):
            b = _run(sr, prep)
            _same(ref, _read(b), what)
            assert b.stream_counts() == (len(terms), decodes), (what, b.stream_counts())
            _same(ref, b.run().results(), what + ", replayed")      # a replay decodes nothing
            assert b.stream_counts() == (len(terms), 0), what
            b.close()
            looked += len(terms)
        s1 = search.stream_cache_stats(L)
        assert s1["hits"] - s0["hits"] + s1["misses"] - s0["misses"] == looked
        assert s1["misses"] - s0["misses"] == len(ta | tb)
        assert s1["streams"] == len(ta | tb) and 0 < s1["bytes_held"] <= s1["budget"]
        assert s1["evictions"] == s0["evictions"]
    sr.close()


def case_eviction_and_pins(L):
    seg = _seg()
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    sets = []
    for i in range(4):   # four sets of 30 terms each, about equal in bytes, no term in two of them
        rows = [[4 + i + 4 * ((7 * q + 3 * j) % 60) for j in range(6)] for q in range(5)]
        filters = [Or([by_term(t) for t in sorted(set(row))]) for row in rows]
        filters += [And([by_term(rows[0][0]), by_term(rows[1][1])])]
        sets.append(filters)
    with _Budget(L, 64 << 20):
        refs = [_off_reference(L, sr, seg, f, BM25()) for f in sets]
        for prep, ref in refs:
            b = _run(sr, prep)
            _same(ref, _read(b), "sizing")
            b.close()
        total = search.stream_cache_stats(L)["bytes_held"]
        _lib.check(L, L.irs_hip_device_trim(0), "irs_hip_device_trim")
        budget = total // 2
        search.set_stream_cache(budget, L)
        ev0 = search.stream_cache_stats(L)["evictions"]
        for rnd in range(2):
            held = _run(sr, refs[rnd][0])     # alive across the whole rotation
            pending = None
            for i in (2, 0, 3, 1, 1, 3, 0, 2):
                b = _run(sr, refs[i][0])
                if pending is not None:       # read after the next one was queued
                    j, pb = pending
                    _same(refs[j][1], _read(pb), (rnd, j))
                    pb.close()
                pending = (i, b)
                assert search.stream_cache_stats(L)["bytes_held"] <= budget
            j, pb = pending
            _same(refs[j][1], _read(pb), (rnd, j))
            pb.close()
            _same(refs[rnd][1], _read(held), (rnd, "held"))
            _same(refs[rnd][1], held.run().results(), (rnd, "held, replayed"))
            held.close()
            s = search.stream_cache_stats(L)      # no batch is alive
            assert s["bytes_held"] <= budget == s["budget"]
        assert search.stream_cache_stats(L)["evictions"] > ev0
    sr.close()


def case_claimed_never_filled(L):
    seg = _seg()
    sr = search.SegmentReader.from_synth(seg, L=L)
    fa, fb = _query_sets()
    with _Budget(L, 64 << 20):
        prep_a, ref_a = _off_reference(L, sr, seg, fa, BM25())
        prep_b, ref_b = _off_reference(L, sr, seg, fb, BM25())
        # planned (the streams claimed, the decode queued), never run
        b = search.QueryBatch(sr, prep_a, K).set_path(_lib.PATH_JOINED).plan()
        b.close()
        b = _run(sr, prep_a)
        _same(ref_a, _read(b), "after a plan without a run")
        b.close()
        # planned, re-dealt to another path (what the plan claimed is given up), destroyed
        b = search.QueryBatch(sr, prep_b, K).set_path(_lib.PATH_JOINED).plan()
        b.set_path(_lib.PATH_ITEMS)
        b.close()
        # created and destroyed untouched
        search.QueryBatch(sr, prep_b, K).close()
        search.QueryBatch(sr, prep_b, K).set_path(_lib.PATH_JOINED).close()
        b = _run(sr, prep_b)
        _same(ref_b, _read(b), "after batches that never ran")
        _same(ref_b, b.run().results(), "replayed")
        b.close()
        s = search.stream_cache_stats(L)
        assert s["bytes_held"] <= s["budget"]
    sr.close()


def case_two_streams(L, streams=(None, None)):
    """A on one stream; B, every stream of which A decodes, on another: no host synchronisation in
    between (B's run waits for A's decode by an event)."""
    seg = _seg()
    sr = search.SegmentReader.from_synth(seg, L=L)
    fa, _ = _query_sets()
    fb = [fa[1], fa[0], Or([by_term(3), by_term(200), by_term(17)]), fa[4]]
    with _Budget(L, 64 << 20):
        prep_a, ref_a = _off_reference(L, sr, seg, fa, BM25())
        prep_b, ref_b = _off_reference(L, sr, seg, fb, BM25())
        a = _run(sr, prep_a, stream=streams[0])
        b = _run(sr, prep_b, stream=streams[1])
        _same(ref_b, _read(b), "B")
        assert b.stream_counts() == (len(_terms(fb)), 0)
        _same(ref_a, _read(a), "A")
        a.close()
        b.close()
    sr.close()


def case_deleted_docs_and_segments(L):
    seg, seg2 = _seg(), _seg(9_000, 60_000)
    rng = np.random.default_rng(77)
    import copy
    masked = copy.copy(seg)
    masked.doc_mask = (rng.choice(seg.num_docs, seg.num_docs // 20, replace=False) + 1).astype(np.uint32)
    sr = search.SegmentReader.from_synth(seg, L=L)
    srm = search.SegmentReader.from_synth(masked, L=L)
    sr2 = search.SegmentReader.from_synth(seg2, L=L)
    fa, _ = _query_sets()
    with _Budget(L, 64 << 20):
        # the same postings with and without deleted docs: two segments, nothing shared
        prep, ref = _off_reference(L, sr, seg, fa, BM25())
        prepm, refm = _off_reference(L, srm, masked, fa, BM25())
        assert (refm[2] < ref[2]).any()
        for what, reader, p, r in (("plain", sr, prep, ref), ("masked", srm, prepm, refm)) * 2:
            b = _run(reader, p)
            _same(r, _read(b), what)
            b.close()
        assert search.stream_cache_stats(L)["streams"] == 2 * len(_terms(fa))
        # two segments in one batch, one threshold per query
        both = [seg, seg2]
        st = [parity.segment_stats(s) for s in both]
        prep2 = search.prepare(fa, BM25(), st)
        search.set_stream_cache(0, L)
        b = _run([sr, sr2], prep2)
        h, c, t = _read(b)
        b.close()
        for i, s in enumerate(both):
            parity.check_single_segment(s, fa, BM25(), K, h[i], c[i], t[i], both)
        b = _run([sr, sr2], prep2, shared=True)
        ref2 = _read(b)
        b.close()
        search.set_stream_cache(64 << 20, L)
        _lib.check(L, L.irs_hip_device_trim(0), "irs_hip_device_trim")
        b = _run([sr, sr2], prep2, shared=True)
        _same(ref2, _read(b), "two segments, cold")
        n, decoded = b.stream_counts()
        assert decoded == n
        b.close()
        b = _run([sr, sr2], prep2, shared=True)
        _same(ref2, _read(b), "two segments, warm")
        assert b.stream_counts() == (n, 0)
        b.close()
    for r in (sr, srm, sr2):
        r.close()


def case_trim_and_close(L):
    seg = _seg()
    sr = search.SegmentReader.from_synth(seg, L=L)
    fa, _ = _query_sets()
    n = len(_terms(fa))
    with _Budget(L, 64 << 20):
        prep, ref = _off_reference(L, sr, seg, fa, BM25())
        for rnd in range(2):
            b = _run(sr, prep)
            _same(ref, _read(b), rnd)
            assert b.stream_counts() == (n, n)        # cold after the trim
            b.close()
            assert search.stream_cache_stats(L)["bytes_held"] > 0
            _lib.check(L, L.irs_hip_device_trim(0), "irs_hip_device_trim")
            s = search.stream_cache_stats(L)
            assert s["bytes_held"] == 0 and s["streams"] == 0
        # a batch alive keeps what it references through a trim
        b = _run(sr, prep)
        _lib.check(L, L.irs_hip_device_trim(0), "irs_hip_device_trim")
        _same(ref, _read(b), "trimmed while alive")
        _same(ref, b.run().results(), "trimmed while alive, replayed")
        b.close()
        # closing a populated segment drops its streams: the reopened one starts cold
        b = _run(sr, prep)
        _same(ref, _read(b), "populate")
        b.close()
        assert search.stream_cache_stats(L)["streams"] == n
        sr.close()
        s = search.stream_cache_stats(L)
        assert s["bytes_held"] == 0 and s["streams"] == 0
        sr = search.SegmentReader.from_synth(seg, L=L)
        b = _run(sr, prep)
        _same(ref, _read(b), "reopened")
        assert b.stream_counts() == (n, n)
        b.close()
    sr.close()


CASES = (case_warm_cold_off, case_eviction_and_pins, case_claimed_never_filled, case_two_streams,
         case_deleted_docs_and_segments, case_trim_and_close)


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_stream_cache_emulated(simlib, case):
    case(simlib)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_stream_cache_gpu(gpulib, case):
    if case is case_two_streams:
        import torch
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        case(gpulib, (C.c_void_p(s1.cuda_stream), C.c_void_p(s2.cuda_stream)))
        torch.cuda.synchronize()
    else:
        case(gpulib)
