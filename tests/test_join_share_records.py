"""k_join_score<kJKHalf>: what a visit's shares are cut from is one row per (visit, piece), worked
out once per chunk (join.h join_pair_rows, JoinRow, JoinOffH::rows) — a piece's first
slab, its slabs and their running sum over the pair's 32 pieces, for the chunk's visits and the
three empty ones begin() looks at past the last.  No reported figure may move.

Shares.  test_join_score_lean's segment (2 x 16320 + 7000 docs: a lone tile in the last pair, pieces
of 1, 2, 3, 4, 5, 9 slabs +- 1 posting) with more lists: 16 terms of exactly one slab in each tile
of a pair (32 pieces, N = 32: with 16 wavefronts a share is two whole pieces, on 1 / 4 wavefronts
one walks all 32 / eight); 16 terms of which every second is absent from the pair's first tile and
every third from its second (empty pieces leading, between and trailing); terms that live in the
second tile of a pair only (the whole first half empty); one term with fewer slabs than wavefronts
(most shares empty); pieces of 5, 6, 7 and 4 k + 1 .. 3 slabs, k = 2, 3, each queried alone with its
image the first of its allocation.  IRS_HIP_JOIN_SPLIT_LOG2 0 / 2 / 4, IRS_HIP_JOIN_CHUNK 1 / 3, the
default chunking.

The largest chunk.  48 image tiles less 300 docs under IRS_HIP_JOIN_CHUNK=48: one chunk of 24
visits, the row table used to its last row; 47: a second chunk of one lone tile.  Queries of 1, 2, 8
and 16 sparse terms with a posting in the first and the last doc of the first and the last tile.

Epilogue edges.  A thread of the epilogue reads and clears words tid * 4 + [0, 4) of every stretch
of 4 * threads accumulator words: 3 / 7 / 15 whole stretches with 1024 / 512 / 256 threads, then the
1008 / 496 / 240 quads that are left.  Lists of four postings sit exactly on the words where a
pass begins or ends, in the low half (first tile of a pair) and in the high half (second tile):

    words     0 ..     3   thread 0, first pass
          12284 .. 12287   thread 1023, last whole pass at 1024 threads
          12288 .. 12291   thread 0, the partial pass at 1024 threads
          14332 .. 14335 / 14336 .. 14339   the same edge at 512 threads
          15356 .. 15359 / 15360 .. 15363   the same edge at 256 threads
          16316 .. 16319   thread 1007 / 495 / 239: the last words
    and the lone tile's last docs (6996 .. 6999).

Their frequencies (4 .. 7 against 1 .. 3 elsewhere) and their rarity make them the best docs of
every query they are in, so at k = 3 the doc ids of the rare path are what is reported.  Queried
alone, two at a time (low half with high half, the two sides of an edge), and next to a populous
term; the term on every doc of the second tile alone and in a pair, so that every lane of the
partial pass counts.

Every batch: paired against set_paired_tiles(0) bit for bit and against the oracle (hits, scores,
order, counts, totals), replayed.  One body per case, emulator and GPU; sparse lists."""
from __future__ import annotations

import numpy as np
import pytest

import cases
import parity
import test_join_score_lean as lean
from iresearch_amd import search, synth
from iresearch_amd.search import BM25, TFIDF, Or, by_term
from test_join_slab_images import _Budget, _Env, _both, _run, _same

BT = lean.BT
WORDS = (0, 12284, 12288, 14332, 14336, 15356, 15360, 16316)   # first word of a quad, see above
LONE_DOCS = lean.TILE_DOCS[2]
assert BT == 16320 and LONE_DOCS == 7000
# (the passes of the three workgroup sizes, as the kernel cuts them)
for threads, full, rest in ((1024, 3, 1008), (512, 7, 496), (256, 15, 240)):
    assert BT // (4 * threads) == full and BT // 4 - full * threads == rest
    assert 4 * full * threads in WORDS and 4 * full * threads - 4 in WORDS


def _segment():
    lists, norms, terms, sizes = lean._segment()
    lists, terms = list(lists), dict(terms)

    def add(name, docs):
        d = np.asarray(docs, np.uint32)
        terms[name] = len(lists)
        lists.append((d, np.arange(4, 4 + d.size, dtype=np.uint32)))   # 4, 5, 6, 7: a strict order

    for half in (0, 1):
        for w in WORDS:
            add(("word", half, w), [1 + half * BT + w + i for i in range(4)])
    add("lone_last", [1 + 2 * BT + LONE_DOCS - 4 + i for i in range(4)])
    return lists, norms, terms


_SEGMENT = []


def _open(L):
    if not _SEGMENT:
        _SEGMENT.append(_segment())
    lists, norms, terms = _SEGMENT[0]
    seg, sr = cases.open_lists(L, lists, lean.N_DOCS, synth.LAYOUT_SIMD4, norms=norms)
    return seg, sr, terms


def _filters(t):
    word = {(h, w): t["word", h, w] for h in (0, 1) for w in WORDS}
    one = [by_term(word[h, w]) for h in (0, 1) for w in WORDS] + [by_term(t["lone_last"])]
    two = [Or([by_term(word[0, w]), by_term(word[1, w])]) for w in WORDS]          # both halves of a word
    two += [Or([by_term(word[h, a]), by_term(word[1 - h, b])])                     # the sides of an edge
            for h in (0, 1) for a, b in ((12284, 12288), (14332, 14336), (15356, 15360), (0, 16316))]
    two += [Or([by_term(word[h, w]), by_term(t["big"])]) for h, w in ((0, 0), (1, 12284), (0, 12288), (1, 16316))]
    two += [Or([by_term(t["lone_last"]), by_term(t["big"])]), Or([by_term(t["lone_last"]), by_term(t["lone"])])]
    full = [by_term(t["full"]), Or([by_term(t["full"]), by_term(t["edge", 2])]),
            Or([by_term(t["full"]), by_term(word[1, 16316])])]
    return one + two + full, len(one), len(two)


def _best(seg, terms, name):
    """The docs of a four-posting list, best first: frequencies 4 .. 7 in doc order."""
    lists = _SEGMENT[0][0]
    return lists[terms[name]][0][::-1]


def case_edges(L):
    seg, sr, terms = _open(L)
    filters, n_one, n_two = _filters(terms)
    st = [parity.segment_stats(seg)]
    for scorer, ks in ((BM25(1.2, 0.0), (3, 100)), (BM25(), (3,)), (TFIDF(True), (3,))):
        prep = search.prepare(filters, scorer, st)
        for k in ks:
            hits, counts, totals = _both(sr, prep, k, lambda h, c, t: parity.check_single_segment(
                seg, filters, scorer, k, h, c, t), (type(scorer).__name__, k))
            assert [int(x) for x in totals[:n_one]] == [4] * n_one
            edge2 = lean.EDGE_TERMS[2]          # (its piece in the second tile lies inside `full`)
            assert [int(x) for x in totals[n_one + n_two:]] == [BT, BT + edge2[0] + edge2[2], BT]
            if k == 3 and isinstance(scorer, BM25) and float(scorer.b) == 0.0:
                # without norms a higher frequency is a higher score: the three best docs by name
                names = [("word", h, w) for h in (0, 1) for w in WORDS] + ["lone_last"]
                for q, name in enumerate(names):
                    assert int(counts[q]) == 3
                    assert [int(d) for d in hits[q, :3]["doc"]] == [int(d) for d in _best(seg, terms, name)[:3]], name
    sr.close()


def case_threads_and_splits(L):
    """The other trip counts (7 + 496 threads, 15 + 240 threads) and the share and chunk boundaries
    around the same words — against results that were held to the 32-bit tiles and the oracle."""
    seg, sr, terms = _open(L)
    filters, n_one, n_two = _filters(terms)
    st = [parity.segment_stats(seg)]
    for scorer, k in ((BM25(), 3), (TFIDF(True), 100)):
        prep = search.prepare(filters, scorer, st)
        ref = _both(sr, prep, k, lambda h, c, t: parity.check_single_segment(
            seg, filters, scorer, k, h, c, t), ("default", k))
        for env in ({"IRS_HIP_JOIN_THREADS": 512}, {"IRS_HIP_JOIN_THREADS": 256},
                    {"IRS_HIP_JOIN_SPLIT_LOG2": 0}, {"IRS_HIP_JOIN_SPLIT_LOG2": 2},
                    {"IRS_HIP_JOIN_CHUNK": 1}, {"IRS_HIP_JOIN_CHUNK": 3, "IRS_HIP_JOIN_THREADS": 256}):
            with _Env(**env):
                b, out = _run(sr, prep, k)
            _same(ref, out, (env, k))
            _same(ref, b.run().results(), (env, k, "replayed"))
            b.close()
    sr.close()


# ---- shares: where a wavefront's part of a visit begins and what it walks over ---------------------

S = lean.SLAB


def _share_lists():
    """name -> postings per tile of the lean segment's three tiles (pair 0: tiles 0 and 1)."""
    out = {}
    for j in range(16):
        out["one_slab", j] = (S, S, 0)                    # 32 pieces of exactly one slab: N = 32
        # every second term absent from the pair's first tile, every third from its second:
        # empty pieces between non-empty ones, leading (j = 0: no) and trailing
        out["gaps", j] = (0 if j % 2 else S + 6 + j, 0 if j % 3 == 0 else 2 * S + j, 0)
    for j in range(3):
        out["second_only", j] = (0, 3 * S + 5 + 40 * j, 0)  # the whole first half of the pair is empty
    out["few_slabs"] = (4 * S - 7, 0, 0)                   # four slabs for sixteen wavefronts
    for s in BACK_SLABS:
        out["back", s] = (S * s - 3, 0, S * s)              # a full group, then a short one
    return out


BACK_SLABS = (5, 6, 7, 9, 10, 11, 13, 14, 15)              # 4 + 1 .. 3 and 4 k + 1 .. 3 for k = 2, 3


def _share_segment():
    rng = np.random.default_rng(2327)
    lists, norms, terms, sizes = lean._segment()
    lists, terms = list(lists), dict(terms)
    for name, per_tile in _share_lists().items():
        terms[name] = len(lists)
        d = np.concatenate([lean._piece(rng, t, n) for t, n in enumerate(per_tile)]).astype(np.uint32)
        lists.append((d, rng.integers(1, 4, d.size).astype(np.uint32)))
    return lists, norms, terms


_SHARES = []


def _open_shares(L):
    if not _SHARES:
        _SHARES.append(_share_segment())
    lists, norms, terms = _SHARES[0]
    seg, sr = cases.open_lists(L, lists, lean.N_DOCS, synth.LAYOUT_SIMD4, norms=norms)
    return seg, sr, terms


def _share_filters(t):
    return [Or([by_term(t["one_slab", j]) for j in range(16)]),
            Or([by_term(t["gaps", j]) for j in range(16)]),
            Or([by_term(t["gaps", j]) for j in range(1, 16)]),        # (the first piece empty too)
            Or([by_term(t["second_only", j]) for j in range(3)]),
            by_term(t["few_slabs"]),
            Or([by_term(t["few_slabs"]), by_term(t["second_only", 0])]),
            Or([by_term(t["or16", j]) for j in range(16)]),
            Or([by_term(t["edge", i]) for i in range(len(lean.SLABS))])]


def case_shares(L):
    """A share's first piece is any of the 32; shares begin in the first, a middle and the last
    slab of a piece; empty pieces lead, trail and lie between; most shares are empty."""
    seg, sr, terms = _open_shares(L)
    filters = _share_filters(terms)
    st = [parity.segment_stats(seg)]
    for scorer, k in ((BM25(), 100), (TFIDF(True), 3)):
        prep = search.prepare(filters, scorer, st)
        ref = _both(sr, prep, k, lambda h, c, t: parity.check_single_segment(
            seg, filters, scorer, k, h, c, t), ("default", k))
        assert int(ref[2][4]) == 4 * S - 7            # (the unions' totals: the oracle's, in _both)
        for env in ({"IRS_HIP_JOIN_SPLIT_LOG2": 0}, {"IRS_HIP_JOIN_SPLIT_LOG2": 2},
                    {"IRS_HIP_JOIN_SPLIT_LOG2": 4}, {"IRS_HIP_JOIN_CHUNK": 1}, {"IRS_HIP_JOIN_CHUNK": 3},
                    {"IRS_HIP_JOIN_CHUNK": 1, "IRS_HIP_JOIN_SPLIT_LOG2": 2}):
            with _Env(**env):
                b, out = _run(sr, prep, k)
            _same(ref, out, (env, k))
            _same(ref, b.run().results(), (env, k, "replayed"))
            b.close()
    sr.close()


def case_short_groups(L):
    """Pieces of 5, 6, 7 slabs and of 4 k + 1 .. 3 slabs, k = 2, 3: full groups, then a short one
    whose request runs past the piece's end.  Each queried ALONE, its image the first of its
    allocation (the cache off; a cache that holds the streams only), then with the share on 1, 4
    and 16 wavefronts: short groups at share ends with and without a group of the same piece in
    front of them."""
    seg, sr, terms = _open_shares(L)
    st = [parity.segment_stats(seg)]
    scorer = BM25()
    for s in BACK_SLABS:
        filters = [by_term(terms["back", s])]
        prep = search.prepare(filters, scorer, st)
        for budget in (0, 64 << 20):
            with _Budget(L, budget):
                if budget:     # the streams alone, then a budget that holds nothing more
                    b, _ = _run(sr, prep, 3, paired=False)
                    b.close()
                    search.set_stream_cache(search.stream_cache_stats(L)["bytes_held"], L)
                ref = _both(sr, prep, 3, lambda h, c, t: parity.check_single_segment(
                    seg, filters, scorer, 3, h, c, t), (s, budget))
                assert int(ref[2][0]) == 2 * S * s - 3
                if budget:
                    continue
                for v in (0, 2, 4):
                    with _Env(IRS_HIP_JOIN_SPLIT_LOG2=v):
                        b, out = _run(sr, prep, 3)
                    _same(ref, out, (s, v))
                    b.close()
    filters = [by_term(terms["back", s]) for s in BACK_SLABS] + \
        [Or([by_term(terms["back", a]), by_term(terms["back", b])]) for a, b in ((5, 15), (6, 9), (7, 14), (10, 13))]
    prep = search.prepare(filters, scorer, st)
    ref = _both(sr, prep, 100, lambda h, c, t: parity.check_single_segment(
        seg, filters, scorer, 100, h, c, t), "together")
    for v in (0, 2):
        with _Env(IRS_HIP_JOIN_SPLIT_LOG2=v):
            b, out = _run(sr, prep, 100)
        _same(ref, out, ("together", v))
        _same(ref, b.run().results(), ("together", v, "replayed"))
        b.close()
    sr.close()


# ---- the largest chunk: 24 visits, the row table used to its last entry ------------------------------

BIG_TILES = 48                                  # kJoinChunkBound
BIG_DOCS = BIG_TILES * BT - 300                 # the last tile partial
_BIG = []


def _big_segment():
    rng = np.random.default_rng(2329)
    last = BIG_DOCS - (BIG_TILES - 1) * BT      # docs of the last tile
    corners = np.array([1, BT, (BIG_TILES - 1) * BT + 1, BIG_DOCS])   # first / last doc of the first / last tile
    lists = []
    for j in range(16):
        n = 150 + 37 * j                         # sparse: a few postings per tile
        inner = 1 + rng.choice(BIG_DOCS, n, replace=False)
        d = np.unique(np.concatenate([corners, inner])).astype(np.uint32)
        lists.append((d, rng.integers(1, 4, d.size).astype(np.uint32)))
    assert last == BT - 300
    norms = rng.integers(40, 60, BIG_DOCS).astype(np.uint8)
    return lists, norms


def case_largest_chunk(L):
    if not _BIG:
        _BIG.append(_big_segment())
    lists, norms = _BIG[0]
    seg, sr = cases.open_lists(L, lists, BIG_DOCS, synth.LAYOUT_SIMD4, norms=norms)
    filters = [by_term(0), Or([by_term(1), by_term(2)]), Or([by_term(j) for j in range(8)]),
               Or([by_term(j) for j in range(16)])]
    st = [parity.segment_stats(seg)]
    scorer = BM25()
    prep = search.prepare(filters, scorer, st)
    with _Env(IRS_HIP_JOIN_CHUNK=BIG_TILES):     # one chunk of 24 visits
        ref = _both(sr, prep, 100, lambda h, c, t: parity.check_single_segment(
            seg, filters, scorer, 100, h, c, t), "one chunk")
    assert int(ref[2][0]) == lists[0][0].size
    for chunk in (BIG_TILES - 1, 0):             # a second chunk of one lone tile; the default chunking
        with _Env(**({"IRS_HIP_JOIN_CHUNK": chunk} if chunk else {})):
            b, out = _run(sr, prep, 100)
        _same(ref, out, chunk)
        _same(ref, b.run().results(), (chunk, "replayed"))
        b.close()
    sr.close()


CASES = (case_edges, case_threads_and_splits, case_shares, case_short_groups, case_largest_chunk)


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_share_rows_emulated(simlib, case):
    case(simlib)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_share_rows_gpu(gpulib, case):
    case(gpulib)
