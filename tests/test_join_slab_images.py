"""k_join_score<kJKHalf> on SLAB-ALIGNED bound images with INTEGER contributions (join.h
k_join_bound_tiles / k_join_bound / join_half_term): every (term, image tile) piece
of an image starts at a multiple of 64 entries and is padded to a multiple of 64 with entries that
add to a dummy word; a posting adds ((u k) >> 16) + 2 with k = ceil(ks 2^16) in place of
uint(fma(ks, u, 2)).  The 16-bit sums only pick docs: every reported figure must stay what the
32-bit tiles and the oracle give.

The segment has 3 x 16320 + 7000 docs (four image tiles, a lone tile in the last pair, 12288- and
16320-doc tilings that disagree).  Lists: pieces of exactly 0, 1, 63, 64, 65, 127, 128, 129, 255,
256, 257 and 320 postings (slab and group edges), each with a posting on the first and on the last
doc of its tile; a term absent from whole tiles; a term present only in the lone tile; 16 short
lists whose pieces cycle through the same counts.  Queries of 1, 2, 8 and 16 terms; BM25, BM15,
TF-IDF with norms; k = 3, 100, 1000.  Boosts: the library keeps 32-bit accumulators — and with them
the joined path — only while a query's score bound stays within 1000 x its smallest term score, so
inside a PAIRED query the boosts spread over one decade (half a decade with 16 terms: k from a few
hundred to near 32768); the queries with boosts over six decades run too, on whatever path the library deals them
to (work items, 64-bit accumulators), against the oracle and with pairing asked for and refused
alike.  k = 1 .. 3 and every other small weight reach the kernel's helper through the probe.

Every batch: paired against set_paired_tiles(0) bit for bit and against the oracle, replayed; the
same with the share split over 1, 4 and 16 wavefronts and with chunks of 1 and 3 tiles.  A ties
batch reaches both full look-up entries of the rescore.  The cache: cold, warm, a budget for the
streams only, off, trim, close, and what the images hold against the allocation bound.  The
contribution rule exhaustively in Python integers, the weight rule, the device helper through the
probe.  One body per case, emulator and GPU; under 300 k postings."""
from __future__ import annotations

import math
import os

import numpy as np
import pytest

import cases
import parity
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, TFIDF, Or, by_term

BT = 16320                      # docs per image tile (kJoinBoundTile)
N_DOCS = 3 * BT + 7000
TILE_DOCS = (BT, BT, BT, 7000)
N_TILES = 4
PIECES = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320)
EDGE_TERMS = ((1, 63, 64, 65), (127, 128, 129, 255), (256, 257, 320, 0))
SLAB = 64
SLACK = 1024                    # kJoinSlack


def _piece(rng, t, n):
    """n docs of image tile t, its first and its last doc among them (n >= 2)."""
    if n == 0:
        return np.zeros(0, np.int64)
    if n == 1:
        off = np.array([0 if t % 2 == 0 else TILE_DOCS[t] - 1])
    else:
        inner = 1 + np.sort(rng.choice(TILE_DOCS[t] - 2, n - 2, replace=False))
        off = np.concatenate(([0], inner, [TILE_DOCS[t] - 1]))
    return 1 + t * BT + off


def _list(rng, per_tile, tf_hi=4):
    d = np.concatenate([_piece(rng, t, n) for t, n in enumerate(per_tile)]).astype(np.uint32)
    return d, rng.integers(1, tf_hi, d.size).astype(np.uint32)


def _segment():
    rng = np.random.default_rng(2011)
    lists, terms, sizes = [], {}, []

    def add(name, per_tile):
        terms[name] = len(lists)
        lists.append(_list(rng, per_tile))
        sizes.append(sum(per_tile))

    for i, per_tile in enumerate(EDGE_TERMS):
        add(("edge", i), per_tile)
    add("absent", (0, 500, 0, 0))
    add("lone", (0, 0, 0, 900))
    add("big", (3000, 2500, 2000, 1500))
    for j in range(16):
        add(("or16", j), tuple(PIECES[(j + 3 * t) % len(PIECES)] for t in range(N_TILES)))
    seen = {n for name, i in terms.items() if name not in ("absent", "lone", "big")
            for t in range(N_TILES)
            for n in [int(np.count_nonzero((lists[i][0] - 1) // BT == t))]}
    assert seen == set(PIECES), sorted(seen)
    assert sum(sizes) < 300_000
    norms = rng.integers(40, 60, N_DOCS).astype(np.uint8)
    return lists, norms, terms, sizes


_SEGMENT = []


def _open(L):
    if not _SEGMENT:
        _SEGMENT.append(_segment())
    lists, norms, terms, sizes = _SEGMENT[0]
    seg, sr = cases.open_lists(L, lists, N_DOCS, synth.LAYOUT_SIMD4, norms=norms)
    return seg, sr, terms, sizes


def _decades(n, decades=1.0):
    """n boosts spread evenly over `decades` decades around 1."""
    return [10.0 ** (decades * (0.5 - i / max(n - 1, 1))) for i in range(n)]


def _filters(t):
    or16 = [t["or16", j] for j in range(16)]
    edges = [t["edge", i] for i in range(len(EDGE_TERMS))]
    one = [by_term(j) for j in edges] + [by_term(t["absent"]), by_term(t["lone"]), by_term(t["big"])]
    two = [Or([by_term(edges[0]), by_term(t["lone"])]), Or([by_term(t["absent"]), by_term(edges[2])]),
           Or([by_term(t["big"], 5.0), by_term(edges[1], 0.2)])]
    eight = [Or([by_term(j) for j in or16[:8]]),
             Or([by_term(j, w) for j, w in zip(or16[8:], _decades(8))]),
             Or([by_term(j, w) for j, w in zip(edges + [t["absent"], t["lone"], t["big"]] + or16[:2],
                                               reversed(_decades(8)))])]
    sixteen = [Or([by_term(j) for j in or16]),
               Or([by_term(j, w) for j, w in zip(or16, _decades(16, 0.5))]),
               Or([by_term(j, w) for j, w in zip(or16, reversed(_decades(16, 0.5)))])]
    return one + two + eight + sixteen


class _Env:
    """A batch knob of the library (read when a batch is created), for the batches made inside."""

    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        return False


def _run(sr, prep, k, paired=True):
    b = sr.batch(prep, k).set_path(_lib.PATH_JOINED).set_paired_tiles(2 if paired else 0)
    out = [x.copy() for x in b.run().results()]
    assert b.path() == _lib.PATH_JOINED and b.paired_tiles() == paired
    assert b.reruns() == 0
    return b, out


def _same(a, b, what):
    for x, y, name in zip(a, b, ("hits", "counts", "totals")):
        assert np.array_equal(x, y), (name, what)


def _both(sr, prep, k, check, what):
    """Paired and on 32-bit tiles: each checked and replayed, the two compared bit for bit."""
    got = {}
    for paired in (True, False):
        b, out = _run(sr, prep, k, paired)
        assert (b.image_counts()[0] > 0) == paired, (what, paired)
        check(*out)
        _same(out, b.run().results(), (what, paired, "replayed"))
        got[paired] = out
        b.close()
    _same(got[True], got[False], what)
    return got[True]


def case_scorers(L):
    seg, sr, terms, sizes = _open(L)
    filters = _filters(terms)
    st = [parity.segment_stats(seg)]
    for scorer in (BM25(), BM25(1.2, 0.0), TFIDF(True)):
        prep = search.prepare(filters, scorer, st)
        for k in (3, 100, 1000):
            _, _, totals = _both(sr, prep, k, lambda h, c, t: parity.check_single_segment(
                seg, filters, scorer, k, h, c, t), (type(scorer).__name__, k))
            assert [int(x) for x in totals[:3]] == [sum(p) for p in EDGE_TERMS]
            assert [int(x) for x in totals[3:6]] == [500, 900, 9000]
    sr.close()


def case_six_decades(L):
    """Boosts over six decades inside a query: beyond what 32-bit accumulators resolve, so the
    library deals these queries to its other kernels whatever is asked for — the results are the
    oracle's, with pairing asked for and with 32-bit tiles asked for alike."""
    seg, sr, terms, sizes = _open(L)
    or16 = [terms["or16", j] for j in range(16)]
    filters = [Or([by_term(j, w) for j, w in zip(or16, _decades(16, 6.0))]),
               Or([by_term(j, w) for j, w in zip(or16[:8], reversed(_decades(8, 6.0)))]),
               Or([by_term(terms["big"], 1.0e3), by_term(terms["edge", 1], 1.0e-3)])]
    st = [parity.segment_stats(seg)]
    for scorer in (BM25(), TFIDF(True)):
        prep = search.prepare(filters, scorer, st)
        for k in (3, 1000):
            got = []
            for paired in (2, 0):
                b = sr.batch(prep, k).set_path(_lib.PATH_JOINED).set_paired_tiles(paired)
                out = [x.copy() for x in b.run().results()]
                parity.check_single_segment(seg, filters, scorer, k, *out)
                _same(out, b.run().results(), ("six decades", k, paired, "replayed"))
                b.close()
                got.append(out)
            _same(got[0], got[1], ("six decades", k))
    sr.close()


def case_splits_and_chunks(L):
    """Share boundaries (the wavefronts a tile's slabs are dealt to) and chunk boundaries (the
    tiles a work item covers) on every slab edge: the same batches with the share split over 1, 4
    and 16 wavefronts and with chunks of 1 and 3 tiles, against the default's results."""
    seg, sr, terms, sizes = _open(L)
    filters = _filters(terms)
    st = [parity.segment_stats(seg)]
    for scorer, k in ((BM25(), 100), (TFIDF(True), 1000), (BM25(1.2, 0.0), 3)):
        prep = search.prepare(filters, scorer, st)
        b, ref = _run(sr, prep, k)
        b.close()
        parity.check_single_segment(seg, filters, scorer, k, *ref)
        for env in ({"IRS_HIP_JOIN_SPLIT_LOG2": 0}, {"IRS_HIP_JOIN_SPLIT_LOG2": 2},
                    {"IRS_HIP_JOIN_SPLIT_LOG2": 4}, {"IRS_HIP_JOIN_CHUNK": 1},
                    {"IRS_HIP_JOIN_CHUNK": 3, "IRS_HIP_JOIN_SPLIT_LOG2": 1}):
            with _Env(**env):
                b, out = _run(sr, prep, k)
            _same(ref, out, (env, k))
            _same(ref, b.run().results(), (env, k, "replayed"))
            b.close()
    sr.close()


def case_ties(L):
    """Thousands of docs with one sum at the k-th score: the rescore's "window over kRescoreMax"
    entry (k = 1000 of 5000 ties) and its "no more than k staged" entry (k >= the hits), each seen
    through irs_hip_batch_rescore_paths; 12 terms, so the window is join_half_slack(8) + 1 wide
    for the Or of eight."""
    rng = np.random.default_rng(53)

    def term(n, tf):
        d = np.sort(rng.choice(N_DOCS, n, replace=False)).astype(np.uint32) + 1
        return d, np.full(n, tf, np.uint32)
    lists = [term(5000, 3), term(3000, 3), term(2000, 2), term(2000, 2)]
    lists += [term(1500, 1) for _ in range(8)]
    seg, sr = cases.open_lists(L, lists, N_DOCS, synth.LAYOUT_SIMD4, norms=np.full(N_DOCS, 9, np.uint8))
    filters = [by_term(0), by_term(1), Or([by_term(2), by_term(3)]),
               Or([by_term(j) for j in range(4, 12)])]
    scorer = BM25()
    prep = search.prepare(filters, scorer, [parity.segment_stats(seg)])
    seen_over = seen_few = 0
    for k in (1000, 3000):
        def check(h, c, t):
            parity.check_single_segment(seg, filters, scorer, k, h, c, t)
            cases._exact_ties(seg, filters, scorer, k, h, c)
        _, _, t = _both(sr, prep, k, check, ("ties", k))
        assert int(t[0]) == 5000 and int(t[1]) == 3000
        b, _ = _run(sr, prep, k)
        window, over, few = b.rescore_paths()
        b.close()
        assert window + over + few == len(filters), (k, window, over, few)
        seen_over += over
        seen_few += few
    assert seen_over >= 1 and seen_few >= 1, (seen_over, seen_few)
    sr.close()


class _Budget:
    """The cache emptied and its budget set for a case; the budget the process had comes back."""

    def __init__(self, L, nbytes):
        self.L, self.nbytes = L, nbytes

    def __enter__(self):
        self.before = search.stream_cache_stats(self.L)["budget"]
        _lib.check(self.L, self.L.irs_hip_device_trim(0), "irs_hip_device_trim")
        assert search.stream_cache_stats(self.L)["bytes_held"] == 0
        assert search.cached_images(self.L) == 0
        search.set_stream_cache(self.nbytes, self.L)
        return self

    def __exit__(self, *exc):
        search.set_stream_cache(self.before, self.L)
        return False


def _size_class(n):
    """pool.h size_class: what the pool rounds an allocation up to."""
    step = 4096
    while step * 16 <= n:
        step <<= 1
    return (max(n, 1) + step - 1) // step * step


def case_cache(L):
    seg, sr, terms, sizes = _open(L)
    filters = _filters(terms)
    used = sorted({s.term for f in filters for s in search._terms_of(f)[1]})
    n = len(used)
    st = [parity.segment_stats(seg)]
    k = 100
    prep = search.prepare(filters, BM25(), st)
    held = lambda: search.stream_cache_stats(L)["bytes_held"]   # noqa: E731
    with _Budget(L, 64 << 20) as bud:
        # off: streams and images private, made in every run
        search.set_stream_cache(0, L)
        b, ref = _run(sr, prep, k)
        parity.check_single_segment(seg, filters, BM25(), k, *ref)
        assert b.stream_counts() == (n, n) and b.image_counts() == (n, n)
        _same(ref, b.run().results(), "off, replayed")
        assert b.image_counts() == (n, n)
        b.close()
        assert held() == 0 and search.cached_images(L) == 0
        search.set_stream_cache(bud.nbytes, L)
        # the streams alone (a run on 32-bit tiles), then cold: the images are made once
        b, out = _run(sr, prep, k, paired=False)
        _same(ref, out, "32-bit tiles")
        b.close()
        streams_only = held()
        assert streams_only > 0 and search.cached_images(L) == 0
        b, out = _run(sr, prep, k)
        _same(ref, out, "cold")
        assert b.stream_counts() == (n, 0) and b.image_counts() == (n, n)
        _same(ref, b.run().results(), "cold, replayed")
        assert b.image_counts() == (n, 0)
        b.close()
        assert search.cached_images(L) == n
        # what the images hold: positive, at most the allocation bound — per image
        # n + 63 min(n, tiles) entries in whole slabs and two boundary tables, the slack of their
        # one slab, as the pool rounds it
        images = held() - streams_only
        entries = sum((sizes[j] + 63 * min(sizes[j], N_TILES) + SLAB - 1) // SLAB * SLAB for j in used)
        bound = _size_class(4 * (entries + SLACK + n * 2 * (N_TILES + 1)))
        assert 0 < images <= bound, (images, bound)
        # warm: no k_join_bound work
        b, out = _run(sr, prep, k)
        _same(ref, out, "warm")
        assert b.stream_counts() == (n, 0) and b.image_counts() == (n, 0)
        b.close()
        # trim drops images with the streams
        _lib.check(L, L.irs_hip_device_trim(0), "irs_hip_device_trim")
        assert held() == 0 and search.cached_images(L) == 0
        # a budget that holds the streams and not the images: private images, every run
        b, out = _run(sr, prep, k, paired=False)
        b.close()
        assert held() == streams_only
        search.set_stream_cache(streams_only, L)
        for what in ("tight", "tight, again"):
            b, out = _run(sr, prep, k)
            _same(ref, out, what)
            assert b.stream_counts() == (n, 0) and b.image_counts() == (n, n), what
            _same(ref, b.run().results(), what + ", replayed")
            assert b.image_counts() == (n, n)
            assert held() <= streams_only and search.cached_images(L) == 0
            b.close()
        # closing the segment drops its images
        search.set_stream_cache(bud.nbytes, L)
        b, out = _run(sr, prep, k)
        _same(ref, out, "before close")
        b.close()
        assert search.cached_images(L) == n and held() > 0
        sr.close()
        assert search.cached_images(L) == 0 and held() == 0


# ---- the contribution rule ------------------------------------------------------------------

RULE_K = (1, 2, 3, 127, 128, 255, 256, 257, 4095, 4096, 32767, 32768, 32769)


def case_half_rule(L):
    u = np.arange(65536, dtype=np.int64)
    entries = (u | (np.int64(0x1234) << 16)).astype(np.uint32)    # (the address bits must not matter)
    rng = np.random.default_rng(8)
    ks_all = list(RULE_K) + [int(x) for x in rng.integers(1, 32770, 1000)]
    for k in ks_all:
        want = ((u * k) >> 16) + 2                                 # Python / int64: exact
        # strictly between ks u + 1 and ks u + 3 with ks = k / 2^16, in integers:
        # (want - 1) 2^16 > k u  and  (want - 3) 2^16 < k u
        assert ((want - 1) * 65536 > u * k).all() and ((want - 3) * 65536 < u * k).all(), k
        lo = search.join_half_probe(entries, k, 0, L)
        assert np.array_equal(lo.astype(np.int64), want), k
        if k in RULE_K or k % 16 == 0:
            hi = search.join_half_probe(entries, k, 1, L)
            assert np.array_equal(hi.astype(np.int64), want << 16), k
    # the weight: k = ceil(cs 2^-15 / U 2^16) for weights up to what fx_mul allows (cs Tsup < 2^30)
    for _ in range(2000):
        tsup = float(rng.uniform(0.125, 40.0))
        U = float(np.float32(65471.0 / tsup))
        cs = float(np.float32(rng.uniform(1.0, 2.0 ** 30 / tsup * (1 - 1e-6))))
        k = search.join_half_rule(cs, U, L)
        assert k == max(1, math.ceil(cs * 2.0 ** -15 / U * 2.0 ** 16)), (cs, U, k)
        assert 1 <= k <= 32801
    assert search.join_half_rule(1.0e-3, 524288.0, L) == 1


CASES = (case_scorers, case_six_decades, case_splits_and_chunks, case_ties, case_cache, case_half_rule)


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_slab_images_emulated(simlib, case):
    case(simlib)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_slab_images_gpu(gpulib, case):
    case(gpulib)
