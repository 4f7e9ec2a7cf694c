"""k_join_score<kJKHalf>: a wavefront's share of a pair visit as ONE sequence of groups
(join.h join_finish_pairs).  A group is up to 256 entries of one (term, half) piece; the sequence
is what join_begin prefetched, then the rest of that piece, then the other pieces; group n + 1 is
requested before group n is accumulated, through two alternating register sets.

The segment has 4 x 12288 + 5000 docs: five tiles, so the last pair has one tile.  The lists are
made so that the entry count of a (term, pair) is exact: with 16 wavefronts per workgroup a
single-term query of N entries in pair 0 gives every wavefront N / 16 of them (+- 1), so

    N        share             what a wavefront streams
    1, 15    0 or 1            empty shares; one entry
    17       1 or 2
    1023..5  63 / 64 / 65      the prefetched group only, around a slab boundary
    4095..7  255 / 256 / 257   prefetch short of a group / exactly one group / group + tail of 1
    5120     320               prefetch + tail
    8191..3  511 / 512 / 513   prefetch + exactly one more full group, no tail / + tail of 1
    12293    768 +             three groups and a tail
    16432    1027              four groups and a tail

each N split about 1/3 : 2/3 between the pair's tiles (two pieces; the boundary falls inside some
wavefront's share), one list entirely in the second tile of its pair, one in pair 1 and tile 4
only.  Piece boundaries inside a share: an Or of 8 terms with 8193, 4097, 1025, 257, 65, 17, 3
and 1 entries per pair, an Or of 16 terms with 257 entries per tile (every share spans two or
more pieces, each shorter than a group), both also with boosts (another cs per piece),
Or(big, tiny) and Or(tiny, big).  Everything under BM25 (table form: the simple instantiation) and
TF-IDF with norms (square-root form); a list whose frequencies reach 200 puts its queries on the
general forms (the instantiation with per-term forms).  k = 3 (a high threshold) and 1000.

Every batch: paired tiles against 32-bit tiles bit for bit (hits, counts, totals), each against
the oracle, the path and pairing asserted, a replayed run() equal to the first.  One body, on the
emulator (CPU tier) and on the GPU; under 200 k postings."""
from __future__ import annotations

import numpy as np
import pytest

import cases
import parity
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, TFIDF, Or, by_term

TILE = 12288
N_DOCS = 4 * TILE + 5000
TILE_DOCS = (TILE, TILE, TILE, TILE, 5000)
SINGLE_N = (1, 15, 17, 1023, 1024, 1025, 4095, 4096, 4097, 5120, 8191, 8192, 8193, 12293, 16432)
OR8_N = (8193, 4097, 1025, 257, 65, 17, 3, 1)
OR16_PER_TILE = 257


def _list(rng, per_tile, tf_hi=4):
    """A posting list with exactly per_tile[t] docs in tile t, frequencies 1 .. tf_hi - 1."""
    docs = [1 + t * TILE + np.sort(rng.choice(TILE_DOCS[t], n, replace=False))
            for t, n in enumerate(per_tile) if n]
    d = np.concatenate(docs).astype(np.uint32)
    return d, rng.integers(1, tf_hi, d.size).astype(np.uint32)


def _pair_split(n, docs_lo=TILE, docs_hi=TILE):
    """n entries of a pair, about 1/3 in its first tile."""
    lo = min(n // 3, docs_lo)
    hi = min(n - lo, docs_hi)
    return lo, hi


def _segment():
    rng = np.random.default_rng(71)
    lists, terms = [], {}
    for n in SINGLE_N:                                  # N entries in pair 0, nothing elsewhere
        terms["single", n] = len(lists)
        lists.append(_list(rng, _pair_split(n) + (0, 0, 0)))
    terms["second"] = len(lists)                        # entirely in the second tile of pair 0
    lists.append(_list(rng, (0, 700, 0, 0, 0)))
    terms["late"] = len(lists)                          # pair 1 and tile 4 only
    lists.append(_list(rng, (0, 0, 300, 500, 900)))
    for n in OR8_N:                                     # n per pair (the last pair: what fits)
        terms["or8", n] = len(lists)
        last = min(n, 2500)
        lists.append(_list(rng, _pair_split(n) + _pair_split(n) + (last,)))
    for j in range(16):
        terms["or16", j] = len(lists)
        lists.append(_list(rng, (OR16_PER_TILE,) * 5))
    terms["general"] = len(lists)                       # frequencies up to 200: no table row
    d, f = _list(rng, (700, 650, 600, 550, 500), tf_hi=201)
    f[:: 7] = 200
    lists.append((d, f))
    assert sum(d.size for d, _ in lists) < 200_000
    norms = rng.integers(40, 60, N_DOCS).astype(np.uint8)
    return lists, norms, terms


_SEGMENT = []   # the lists, built once for both tiers


def _batches(terms):
    t = terms
    or8 = [t["or8", n] for n in OR8_N]
    or16 = [t["or16", j] for j in range(16)]
    big, tiny = t["or8", 8193], t["or8", 1]
    plain = [by_term(t["single", n]) for n in SINGLE_N]
    plain += [by_term(t["second"]), by_term(t["late"])]
    # (boosts that fall as the terms get rarer: under TF-IDF with norms the batch only stays on
    # 32-bit accumulators — and so on the joined path — while every query's upper bound is within
    # 1000 x its smallest posting score, and the rare terms' idf already spreads the two)
    plain += [Or([by_term(j) for j in or8]), Or([by_term(j) for j in or16]),
              Or([by_term(j, 2.0 - 0.15 * i) for i, j in enumerate(or8)]),
              Or([by_term(j, 3.0 - 0.125 * i) for i, j in enumerate(or16)]),
              Or([by_term(big), by_term(tiny)]), Or([by_term(tiny), by_term(big)])]
    g = t["general"]
    general = [by_term(g), Or([by_term(g), by_term(t["single", 8193])]),
               Or([by_term(t["single", 4097]), by_term(g, 2.0), by_term(t["late"])]),
               Or([by_term(j) for j in or16[:15]] + [by_term(g)])]
    return plain, general


def _run(sr, seg, filters, scorer, k):
    prep = search.prepare(filters, scorer, [parity.segment_stats(seg)])
    got = {}
    for paired in (True, False):
        b = sr.batch(prep, k).set_path(_lib.PATH_JOINED).set_paired_tiles(2 if paired else 0)
        h, c, t = (x.copy() for x in b.run().results())
        assert b.path() == _lib.PATH_JOINED, (scorer, k, paired)
        assert b.paired_tiles() == paired, (scorer, k, paired)
        parity.check_single_segment(seg, filters, scorer, k, h, c, t)
        h2, c2, t2 = b.run().results()          # replayed
        assert np.array_equal(h, h2) and np.array_equal(c, c2) and np.array_equal(t, t2), (scorer, k, paired)
        got[paired] = (h, c, t)
        b.close()
    for x, y, what in zip(got[True], got[False], ("hits", "counts", "totals")):
        assert np.array_equal(x, y), (what, scorer, k)
    return got[True]


def case_stream_groups(L, layout=synth.LAYOUT_SIMD4):
    if not _SEGMENT:
        _SEGMENT.append(_segment())
    lists, norms, terms = _SEGMENT[0]
    seg, sr = cases.open_lists(L, lists, N_DOCS, layout, norms=norms)
    plain, general = _batches(terms)
    for scorer in (BM25(), TFIDF(True)):
        for k in (3, 1000):
            _, _, totals = _run(sr, seg, plain, scorer, k)
            # the lists are what the table above says
            assert [int(x) for x in totals[:len(SINGLE_N)]] == list(SINGLE_N)
            _run(sr, seg, general, scorer, k)
    sr.close()


def test_stream_groups_emulated(simlib):
    case_stream_groups(simlib)


@pytest.mark.gpu
def test_stream_groups_gpu(gpulib):
    case_stream_groups(gpulib)
