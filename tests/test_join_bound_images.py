"""k_join_score<kJKHalf> on BOUND IMAGES (join.h k_join_bound): per (segment, term,
scorer signature) a second entry array in posting order, cut into tiles of 16320 docs, whose
entries carry a 16-bit upper bound u of the posting's score factor instead of (tf, norm); the
paired kernel adds uint(fma(cs 2^-15 / U, u, 2)) per posting — no table — and k_join_rescore forms
the reported sums from the exact streams (12288-doc tiles) as before.

The segment has 3 x 16320 + 7000 docs: four image tiles, so the last pair has one tile, and the
12288- and 16320-doc tilings disagree everywhere past tile 0.  Lists: postings at the first and
last doc of every image tile and on both sides of every 12288 boundary; one list holding every doc
of pair 0; lists entirely in the second tile of pair 0 and in the last, lone tile; single terms
with the share sizes of test_join_stream_groups.py (N entries in pair 0, about 1/3 : 2/3 over its
tiles); an Or of 8 and an Or of 16 short lists, with and without boosts; a list whose frequencies
reach 255 (the v_rcp / v_sqrt forms of the exact path) mixed with table-row lists.  BM25, BM15 (no
norms), TF-IDF with norms, a batch whose queries use two norm signatures, queries whose terms use
two table slots; k = 3, 100 and 1000.

Every batch: paired against set_paired_tiles(0) bit for bit (hits, scores, order, counts,
totals), each against the oracle, path() == PATH_JOINED and paired_tiles(), reruns() == 0, a
replayed run() equal to the first.  A ties batch (thousands of docs with one sum at the k-th
score) reaches the rescore's "window over kRescoreMax" and "no more than k staged" entries.  The
cache: what is and is not rebuilt, budgets too small for the images, the cache off, trim and
close.  The bound rule itself, exhaustively on the host.  One body per case, on the emulator (CPU
tier) and on the GPU; under 300 k postings."""
from __future__ import annotations

import copy

import numpy as np
import pytest

import cases
import parity
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, TFIDF, Or, by_term

BT = 16320                      # docs per image tile (kJoinBoundTile)
ET = 12288                      # docs per tile of the exact streams (kJoinTile)
N_DOCS = 3 * BT + 7000
TILE_DOCS = (BT, BT, BT, 7000)
SINGLE_N = (1, 15, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16384)
OR8_N = (8193, 4097, 1025, 257, 65, 17, 3, 1)
OR16_PER_TILE = 257
# types.h Kind, as the library resolves the scorers below against a segment with 1-byte norms
K_BM15, K_BM25_TINY, K_TFIDF, K_TFIDF_TINY = 1, 2, 5, 6


def _list(rng, per_tile, tf_hi=4):
    """A posting list with exactly per_tile[t] docs in image tile t, frequencies 1 .. tf_hi - 1."""
    docs = [1 + t * BT + np.sort(rng.choice(TILE_DOCS[t], n, replace=False))
            for t, n in enumerate(per_tile) if n]
    d = np.concatenate(docs).astype(np.uint32)
    return d, rng.integers(1, tf_hi, d.size).astype(np.uint32)


def _split(n, lo_docs=BT, hi_docs=BT):
    lo = min(n // 3, lo_docs)
    return lo, min(n - lo, hi_docs)


def _segment():
    rng = np.random.default_rng(193)
    lists, terms = [], {}

    def add(name, item):
        terms[name] = len(lists)
        lists.append(item)

    edge = {0, N_DOCS - 1}
    for t in range(4):
        edge |= {t * BT, min(t * BT + BT - 1, N_DOCS - 1)}
    for b in range(1, (N_DOCS + ET - 1) // ET):
        edge |= {b * ET - 1, b * ET}
    d = np.array(sorted(edge), np.uint32) + 1
    add("edges", (d, rng.integers(1, 4, d.size).astype(np.uint32)))
    d = np.arange(1, 2 * BT + 1, dtype=np.uint32)           # every doc of pair 0
    add("full", (d, rng.integers(1, 4, d.size).astype(np.uint32)))
    add("second", _list(rng, (0, 700, 0, 0)))
    add("lone", _list(rng, (0, 0, 0, 900)))
    for n in SINGLE_N:
        add(("single", n), _list(rng, _split(n) + (0, 0)))
    for n in OR8_N:
        add(("or8", n), _list(rng, _split(n) + _split(n, BT, 7000)[:1] + (min(n, 2500),)))
    for j in range(16):
        add(("or16", j), _list(rng, (OR16_PER_TILE,) * 4))
    d, f = _list(rng, (700, 650, 600, 550), tf_hi=256)       # frequencies up to 255: no table row
    f[::7] = 255
    add("general", (d, f))
    assert sum(d.size for d, _ in lists) < 300_000
    norms = rng.integers(40, 60, N_DOCS).astype(np.uint8)
    return lists, norms, terms


_SEGMENT = []   # the lists, built once for both tiers


def _batches(t):
    or8 = [t["or8", n] for n in OR8_N]
    or16 = [t["or16", j] for j in range(16)]
    plain = [by_term(t["single", n]) for n in SINGLE_N]
    plain += [by_term(t["edges"]), by_term(t["full"]), by_term(t["second"]), by_term(t["lone"]),
              Or([by_term(t["edges"]), by_term(t["lone"]), by_term(t["second"])]),
              Or([by_term(t["full"]), by_term(t["edges"])]),
              Or([by_term(j) for j in or8]), Or([by_term(j) for j in or16]),
              Or([by_term(j, 2.0 - 0.15 * i) for i, j in enumerate(or8)]),
              Or([by_term(j, 3.0 - 0.125 * i) for i, j in enumerate(or16)])]
    g = t["general"]
    general = [by_term(g), Or([by_term(g), by_term(t["single", 8193])]),
               Or([by_term(t["single", 4097]), by_term(g, 2.0), by_term(t["lone"])]),
               Or([by_term(j) for j in or16[:15]] + [by_term(g)])]
    return plain, general


def _both(sr, prep, k, check):
    """The batch paired and on 32-bit tiles: each checked, replayed, compared bit for bit."""
    got = {}
    for paired in (True, False):
        b = sr.batch(prep, k).set_path(_lib.PATH_JOINED).set_paired_tiles(2 if paired else 0)
        h, c, t = (x.copy() for x in b.run().results())
        assert b.path() == _lib.PATH_JOINED, (k, paired)
        assert b.paired_tiles() == paired, (k, paired)
        assert b.reruns() == 0, (k, paired, b.reruns())
        n_img, _ = b.image_counts()
        assert (n_img > 0) == paired, (k, paired, n_img)
        check(h, c, t)
        h2, c2, t2 = b.run().results()          # replayed
        assert np.array_equal(h, h2) and np.array_equal(c, c2) and np.array_equal(t, t2), (k, paired)
        got[paired] = (h, c, t)
        b.close()
    for x, y, what in zip(got[True], got[False], ("hits", "counts", "totals")):
        assert np.array_equal(x, y), (what, k)
    return got[True]


def _open(L, layout=synth.LAYOUT_SIMD4):
    if not _SEGMENT:
        _SEGMENT.append(_segment())
    lists, norms, terms = _SEGMENT[0]
    seg, sr = cases.open_lists(L, lists, N_DOCS, layout, norms=norms)
    return seg, sr, terms


def case_scorers(L):
    seg, sr, terms = _open(L)
    plain, general = _batches(terms)
    st = [parity.segment_stats(seg)]
    for scorer in (BM25(), BM25(1.2, 0.0), TFIDF(True)):
        for k in (3, 100, 1000):
            for filters in (plain, general):
                prep = search.prepare(filters, scorer, st)
                _, _, totals = _both(sr, prep, k, lambda h, c, t: parity.check_single_segment(
                    seg, filters, scorer, k, h, c, t))
                if filters is plain:
                    assert [int(x) for x in totals[:len(SINGLE_N)]] == list(SINGLE_N)
    sr.close()


def case_two_signatures(L):
    """Queries of two norm signatures in one batch (the same terms: two images per stream), and
    queries whose own terms use two table slots (two cache_ids: eight rows per slot, so
    frequencies from 8 on take the exact path's general forms)."""
    seg, sr, terms = _open(L)
    plain, general = _batches(terms)
    st = [parity.segment_stats(seg)]
    s1, s2 = BM25(), BM25(2.0, 0.4)
    fa, fb = plain[-6:] + general, plain[-4:] + general[:2]
    pa, pb = search.prepare(fa, s1, st), search.prepare(fb, s2, st)
    for k in (3, 100, 1000):
        def check(h, c, t):
            parity.check_single_segment(seg, fa, s1, k, h[:len(fa)], c[:len(fa)], t[:len(fa)])
            parity.check_single_segment(seg, fb, s2, k, h[len(fa):], c[len(fa):], t[len(fa):])
        _both(sr, pa + pb, k, check)
    # two slots inside a query: every other term scored under the second signature (no oracle for
    # a query of mixed scorers: paired against 32-bit tiles, and against the work-item path)
    mixed = []
    for qa, qb in zip(search.prepare(fa, s1, st), search.prepare(fa, s2, st)):
        q = copy.copy(qa)
        q.scorers = [sb if j % 2 else sa for j, (sa, sb) in enumerate(zip(qa.scorers, qb.scorers))]
        mixed.append(q)
    for k in (3, 100, 1000):
        got = _both(sr, mixed, k, lambda h, c, t: None)
        b = sr.batch(mixed, k).set_path(_lib.PATH_ITEMS)
        for x, y in zip(got, b.run().results()):
            assert np.array_equal(x, y)
        b.close()
    sr.close()


def case_ties(L):
    """The shape of cases.case_paired_ties on the image tiling: 5 000 docs of one sum at k = 1000
    (the window holds more than kRescoreMax docs: every staged doc is looked up, three passes),
    3 000 at k = 2 999, and k >= the hits (no more than k staged: the full path directly) — each
    observed through the rescore's path counters."""
    rng = np.random.default_rng(47)

    def term(n, tf):
        d = np.sort(rng.choice(N_DOCS, n, replace=False)).astype(np.uint32) + 1
        return d, np.full(n, tf, np.uint32)
    lists = [term(5000, 3), term(3000, 3), term(2000, 2), term(2000, 2)]
    lists += [term(1500, 1) for _ in range(8)]
    seg, sr = cases.open_lists(L, lists, N_DOCS, synth.LAYOUT_SIMD4, norms=np.full(N_DOCS, 9, np.uint8))
    filters = [by_term(0), by_term(1), Or([by_term(2), by_term(3)]),
               Or([by_term(j) for j in range(4, 12)])]
    for scorer in (BM25(), TFIDF(True)):
        prep = search.prepare(filters, scorer, [parity.segment_stats(seg)])
        for k in (1000, 2999, 3000):
            def check(h, c, t):
                parity.check_single_segment(seg, filters, scorer, k, h, c, t)
                cases._exact_ties(seg, filters, scorer, k, h, c)
            _, _, t = _both(sr, prep, k, check)
            assert int(t[0]) == 5000 and int(t[1]) == 3000
            # which entries of the rescore the units took (irs_hip_batch_rescore_paths): the 5 000
            # and the 3 000 tied docs are a window of more than kRescoreMax = 2048 docs wherever
            # more than k of them are staged; with no more than k staged the full path directly
            b = sr.batch(prep, k).set_path(_lib.PATH_JOINED).set_paired_tiles(2)
            b.run()
            window, over, few = b.rescore_paths()
            b.close()
            assert window + over + few == len(filters), (k, window, over, few)
            assert over >= (2 if k < 3000 else 1), (k, window, over, few)
            assert few >= (1 if k >= 3000 else 0), (k, window, over, few)
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


def _run(sr, prep, k, paired=True):
    b = sr.batch(prep, k).set_path(_lib.PATH_JOINED).set_paired_tiles(2 if paired else 0)
    out = [x.copy() for x in b.run().results()]
    assert b.path() == _lib.PATH_JOINED and b.paired_tiles() == paired
    return b, out


def _same(a, b, what):
    for x, y, name in zip(a, b, ("hits", "counts", "totals")):
        assert np.array_equal(x, y), (name, what)


def case_cache(L):
    seg, sr, terms = _open(L)
    plain, general = _batches(terms)
    filters = plain[-8:] + general
    n = len({s.term for f in filters for s in search._terms_of(f)[1]})
    st = [parity.segment_stats(seg)]
    k = 100
    p_bm, p_tf, p_b2 = (search.prepare(filters, s, st) for s in (BM25(), TFIDF(True), BM25(2.0, 0.4)))
    held = lambda: search.stream_cache_stats(L)["bytes_held"]   # noqa: E731
    with _Budget(L, 64 << 20) as bud:
        # the references: the cache off — streams and images made privately, in every run
        search.set_stream_cache(0, L)
        refs = {}
        for name, prep, scorer in (("bm", p_bm, BM25()), ("tf", p_tf, TFIDF(True)), ("b2", p_b2, BM25(2.0, 0.4))):
            b, ref = _run(sr, prep, k)
            parity.check_single_segment(seg, filters, scorer, k, *ref)
            assert b.stream_counts() == (n, n) and b.image_counts() == (n, n)
            _same(ref, b.run().results(), "off, replayed")
            assert b.stream_counts() == (n, n) and b.image_counts() == (n, n)
            b.close()
            b, unpaired = _run(sr, prep, k, paired=False)
            _same(ref, unpaired, "off, 32-bit tiles")
            assert b.image_counts() == (0, 0)
            b.close()
            assert held() == 0 and search.cached_images(L) == 0
            refs[name] = ref
        search.set_stream_cache(bud.nbytes, L)
        # cold: streams and images made once; the same terms and signature again: neither kernel
        b, out = _run(sr, p_bm, k)
        _same(refs["bm"], out, "cold")
        assert b.stream_counts() == (n, n) and b.image_counts() == (n, n)
        _same(refs["bm"], b.run().results(), "cold, replayed")
        assert b.stream_counts() == (n, 0) and b.image_counts() == (n, 0)
        b.close()
        assert search.cached_images(L) == n and search.stream_cache_stats(L)["streams"] == n
        with_images = held()
        b, out = _run(sr, p_bm, k)
        _same(refs["bm"], out, "warm")
        assert b.stream_counts() == (n, 0) and b.image_counts() == (n, 0)
        b.close()
        # another scorer, another signature of the same scorer: images only, the streams are hits
        s0 = search.stream_cache_stats(L)
        for name, prep in (("tf", p_tf), ("b2", p_b2)):
            b, out = _run(sr, prep, k)
            _same(refs[name], out, name)
            assert b.stream_counts() == (n, 0) and b.image_counts() == (n, n), name
            b.close()
        s1 = search.stream_cache_stats(L)
        assert s1["hits"] - s0["hits"] == 2 * n and s1["misses"] == s0["misses"]
        assert search.cached_images(L) == 3 * n and s1["streams"] == n
        assert with_images < s1["bytes_held"] <= s1["budget"]
        # trim drops images with the streams
        _lib.check(L, L.irs_hip_device_trim(0), "irs_hip_device_trim")
        assert held() == 0 and search.cached_images(L) == 0
        # a budget that holds the streams and not the images: the images are private, every run
        b, out = _run(sr, p_bm, k, paired=False)
        b.close()
        streams_only = held()
        assert 0 < streams_only < with_images
        search.set_stream_cache(streams_only, L)
        for what in ("tight", "tight, again"):
            b, out = _run(sr, p_bm, k)
            _same(refs["bm"], out, what)
            assert b.stream_counts() == (n, 0) and b.image_counts() == (n, n), what
            _same(refs["bm"], b.run().results(), what + ", replayed")
            assert b.image_counts() == (n, n)
            assert held() <= streams_only and search.cached_images(L) == 0
            b.close()
        # closing the segment drops its images
        search.set_stream_cache(bud.nbytes, L)
        b, out = _run(sr, p_tf, k)
        _same(refs["tf"], out, "before close")
        b.close()
        assert search.cached_images(L) == n and held() > 0
        sr.close()
        assert search.cached_images(L) == 0 and held() == 0


# ---- the bound rule on the host ------------------------------------------------------------

f32 = np.float32


def _table_value(kind, nc, nl, n):
    """score.h table_value in float32, operation by operation."""
    n = n.astype(np.float32)
    with np.errstate(divide="ignore"):
        if kind == K_BM25_TINY:
            return np.where(n > 0, f32(1) / (f32(nc) + f32(nl) * n), f32(0)).astype(np.float32)
        if kind == K_BM15:
            return np.full(n.shape, f32(1) / f32(nc), np.float32)
        if kind == K_TFIDF:
            return np.ones(n.shape, np.float32)
        return np.where(n > 0, f32(1) / np.sqrt(n), f32(0)).astype(np.float32)


def _factors(kind, nc, nl, tf, norm):
    """(the table row's float, the largest value the general form can give): what join_post
    multiplies by cs for a posting, for tf, norm arrays.  v_rcp / v_sqrt are within 1 ulp."""
    t = _table_value(kind, nc, nl, norm)
    tff = tf.astype(np.float32)
    if kind in (K_TFIDF, K_TFIDF_TINY):
        row = (np.sqrt(tff) * t).astype(np.float32)
        # fast_sqrt(tf) * cs * t: 1 ulp of the root, two roundings of the products
        gen = np.sqrt(tff.astype(np.float64)) * t.astype(np.float64) * (1 + 2.0 ** -23) * (1 + 2.0 ** -23)
        return row, gen
    d = (f32(1) + tff * t).astype(np.float32)
    row = (f32(1) - f32(1) / d).astype(np.float32)
    df = np.float32(tff.astype(np.float64) * t.astype(np.float64) + 1.0).astype(np.float64)   # fma, rounded once
    gen = (1.0 - (1.0 / df) * (1 - 2.0 ** -23)) * (1 + 2.0 ** -24)   # fma(-cs, rcp, cs) / cs
    return row, gen


def case_bound_rule(L):
    seg, sr, terms = _open(L)
    st = parity.segment_stats(seg)
    sr.close()
    rng = np.random.default_rng(5)
    sigs = []
    for scorer, kind in ((BM25(), K_BM25_TINY), (BM25(2.0, 0.4), K_BM25_TINY), (BM25(1.2, 0.0), K_BM15),
                         (TFIDF(True), K_TFIDF_TINY), (TFIDF(False), K_TFIDF)):
        ts = scorer.collect(st.docs_with_field, 1000, st.total_term_freq)
        sigs.append((kind, float(ts.norm_const), float(ts.norm_length)))
    tf, norm = np.meshgrid(np.arange(1, 256), np.arange(256), indexing="ij")
    for kind, nc, nl in sigs:
        for tf_bound in ((255,) if kind in (K_BM25_TINY, K_BM15) else (1, 3, 15, 200, 255)):
            rule = search.join_bound_rule(kind, nc, nl, tf_bound, L)
            assert rule is not None, (kind, nc, nl)
            u, U, c, tile = rule
            assert tile == BT and 0 < c <= 3.0
            keep = tf <= tf_bound
            row, gen = _factors(kind, nc, nl, tf, norm)
            got = u[1:].astype(np.float64)
            top = np.maximum(row.astype(np.float64), gen)
            assert (got[keep] >= top[keep] * U).all(), (kind, tf_bound)           # u / U >= T
            assert (got[keep] <= row.astype(np.float64)[keep] * U + c).all(), (kind, tf_bound)
            assert got[keep].max() <= 65535
            # the 16-bit contribution against the exact contribution's 16-bit image, for weights up
            # to what fx_mul allows (cs Tsup < 2^30): above it, by no more than 2 + 2^-6 + cs16 c / U
            tsup = 65471.0 / U
            for _ in range(4):
                cs = f32(rng.uniform(2.0 ** 18, 2.0 ** 30 / tsup * (1 - 1e-6)))
                ks = f32(f32(cs * f32(2.0 ** -15)) / f32(U))
                img = np.floor(np.float32(np.float64(ks) * got + 2.0).astype(np.float64))
                exact = np.floor(np.float32(np.float64(cs) * row.astype(np.float64) + 1.0).astype(np.float64))
                hi = np.floor(np.float64(cs) * gen) + 1.0            # static_cast<uint32_t>(scaled) | 1
                x = np.maximum(exact, hi) / 2.0 ** 15
                assert (img[keep] > x[keep]).all(), (kind, tf_bound, cs)
                lo = np.minimum(exact, np.floor(np.float64(cs) * row.astype(np.float64))) / 2.0 ** 15
                slack = 2.0 + 2.0 ** -6 + float(cs) * 2.0 ** -15 * c / U
                assert (img[keep] <= lo[keep] + slack).all(), (kind, tf_bound, cs)
                assert img[keep].max() < 2.0 ** 15 + 8
    # a reciprocal form so flat that 1 - 1/x would not fit the slack gets no image
    assert search.join_bound_rule(K_BM15, 1.0e6, 0.0, 255, L) is None


CASES = (case_scorers, case_two_signatures, case_ties, case_cache, case_bound_rule)


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_bound_images_emulated(simlib, case):
    case(simlib)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_bound_images_gpu(gpulib, case):
    case(gpulib)
