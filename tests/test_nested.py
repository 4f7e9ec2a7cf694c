"""irs_hip_batch_nested_sets / _sets_to_device / _topk: ByNestedFilter, the block join
(core/search/nested_filter.{hpp,cpp}), on k_nested_match / k_nested_list / k_nested_merge
(csrc/nested.h).

Expectations come from code that exists, never from the calls under test: the child filter's
(score, matched) for ALL docs of a segment from the oracle, the way test_score_docs.want calls it
(exclusions, a doc mask, the unit's merge, test_nested_boolean.expected for grouped units), then ONE
plain restatement of the semantics in include/irs_hip.h — a loop over the parents with a float64
merge of the oracle's child scores (`blocks_of`, `restate`).  Sets, counts and total_hits are held
bit for bit; the top k as parity.check_single_segment holds it, with a tolerance that is derived:
parity.REL_TOL for MAX / MIN and under kMatchNone, REL_TOL + (c_max - 1) * 2^-24 for SUM, c_max =
the most children merged into one hit of the case (the per-child bound the project holds plus one
float32 rounding per addition of non-negative terms).  c_max <= 65 wherever a SUM is checked (the
issue's 63 / 64 / 65 blocks); the block longer than two kernel tiles is checked by its sets and
counts, and by MAX / MIN scores, whose bound does not grow with the children.
One body per case, on the emulator (CPU tier) and on the GPU."""
from __future__ import annotations

import os
import re
from pathlib import Path

import numpy as np
import pytest

import parity
import test_score_docs as sd
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import (BM25, MERGE_MAX, MERGE_MIN, MERGE_SUM, TFIDF, And, Or, by_doc_set, by_phrase,
                                  by_term, by_terms)

CSRC = Path(__file__).resolve().parents[1] / "iresearch_amd" / "csrc"
X = sd.X


def _const(name: str) -> int:
    """`NAME = <integer>` of nested.h / kernels.h, through one `NAME = OTHER` step."""
    text = (CSRC / "nested.h").read_text() + (CSRC / "kernels.h").read_text()
    m = re.search(r"\b%s\s*=\s*(\w+?)u?\s*[;,]" % name, text)
    assert m, name
    return int(m.group(1)) if m.group(1).isdigit() else _const(m.group(1))


TILE_WORDS = _const("kNestedTile")       # 64-bit words of one k_nested_match / k_nested_list tile
TILE = 64 * TILE_WORDS                   # ... in docs
LONG_RUN = _const("kNestedLongRun")      # children beyond which a wavefront merges a run
SELECT_STAGE = _const("kSelectStage")
MATCHES = [(0, 0), (1, None), (2, None), (0, None), (0, 2), (2, 3), (3, 3), (1, 1)]
MERGES = [MERGE_SUM, MERGE_MAX, MERGE_MIN]


# ------------------------------------------------------------- expectations --

def bits(docs, n_words):
    """A bitset row (bit = doc id) of `docs`."""
    b = np.zeros(64 * n_words, bool)
    b[np.asarray(docs, np.int64)] = True
    return np.packbits(b, bitorder="little").view(np.uint64)


def unbits(row, n1):
    return np.unpackbits(np.ascontiguousarray(row).view(np.uint8), bitorder="little")[:n1].astype(bool)


def blocks_of(parent_row, num_docs, child_matched):
    """[(parent, its children)] in doc order: the parents are the row's bits 1..num_docs, the block
    of p is (prev(p), p), the children are the child filter's matches that are no parent."""
    n1 = num_docs + 1
    par = unbits(parent_row, max(n1, 64 * len(parent_row)))[:n1].copy()
    par[0] = False
    kids = child_matched[:n1] & ~par
    out, prev = [], 0
    for p in np.nonzero(par)[0]:
        out.append((int(p), np.nonzero(kids[prev + 1:p])[0] + prev + 1))
        prev = int(p)
    return out


def restate(blocks, child_score, deleted, match, merge, none_boost, n1):
    """(hit bool[n1], score f64[n1], c_max): the semantics, one parent at a time."""
    lo, hi = match
    hit, score, c_max = np.zeros(n1, bool), np.zeros(n1, np.float64), 0
    for p, kids in blocks:
        c = len(kids)
        if deleted[p] or c < lo or (hi is not None and c > hi):
            continue
        hit[p] = True
        if (lo, hi) == (0, 0):
            score[p] = none_boost
            continue
        if c == 0:
            continue
        vals = child_score[kids].astype(np.float64)
        if (lo, hi) == (0, None):            # the buffer starts from 0 (nested_filter.cpp:477-485)
            vals = np.concatenate([[0.0], vals])
        score[p] = vals.sum() if merge == MERGE_SUM else vals.max() if merge == MERGE_MAX else vals.min()
        c_max = max(c_max, c)
    return hit, score, c_max


def deleted_of(seg):
    d = np.zeros(seg.num_docs + 1, bool)
    m = getattr(seg, "doc_mask", None)
    if m is not None:
        d[np.asarray(m, np.int64)] = True
    return d


def tol_of(match, merge, c_max):
    if match == (0, 0) or merge != MERGE_SUM:
        return parity.REL_TOL
    return parity.REL_TOL + max(c_max - 1, 0) * 2.0 ** -24


def check_sets(tag, sets_row, count, hit, n_words):
    want = bits(np.nonzero(hit)[0], n_words)
    assert np.array_equal(sets_row, want), (tag, "set", np.nonzero(unbits(sets_row, 64 * n_words)[:hit.size] != hit)[0][:8])
    assert int(count) == int(hit.sum()), (tag, "count", int(count), int(hit.sum()))


def check_topk(tag, h, n, total, k, hit, score, tol):
    """parity.check_single_segment's comparison against (hit, score) of all docs."""
    n_hit = int(hit.sum())
    assert int(total) == n_hit, (tag, "total hits", int(total), n_hit)
    n = int(n)
    assert n == min(k, n_hit), (tag, "count", n, k, n_hit)
    if n == 0:
        return
    h = h[:n]
    docs = h["doc"].astype(np.int64)
    assert len(set(docs.tolist())) == n, (tag, "duplicate docs")
    assert (docs < hit.size).all() and hit[docs].all(), (tag, "a doc that is no hit")
    ref = score[docs]
    rel = np.abs(h["score"] - ref) / np.maximum(np.abs(ref), 1e-30)
    rel[(ref == 0) & (h["score"] == 0)] = 0
    print(tag, "max rel", float(rel.max()), "tol", tol)
    assert rel.max() <= tol, (tag, "score", float(rel.max()), tol, int(docs[np.argmax(rel)]))
    s, d = h["score"], h["doc"]
    assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (d[:-1] < d[1:]))).all(), (tag, "order")
    thr = np.sort(score[hit])[::-1][n - 1]
    must = np.nonzero(hit & (score > thr * (1 + 2 * tol)))[0]
    assert np.isin(must, docs).all(), (tag, "missing doc above the k-th score")
    assert (ref >= thr * (1 - 2 * tol)).all(), (tag, "doc below the k-th score")


def family_of(flt):
    return "grouped" if type(flt) is And and any(type(s) is Or for s in flt.subs) else "flat"


def child_of(seg, triple, scorer, all_segs=None, inset=None):
    """(score f64[n1], matched bool[n1]) of one child filter on one segment."""
    sc, m = sd.want(family_of(triple[1]), seg, triple, scorer, all_segs)
    if inset is not None:
        m = m & inset[:m.size]
        sc = np.where(m, sc, 0.0)
    return sc, m


# -------------------------------------------------------------------- cases --

def hand_segment(layout):
    """~70 000 docs; the parents and the children that pin the carries (see case_blocks)."""
    N = 70_000
    assert N > 4 * TILE and N < 5 * TILE
    A = [200, 225, 226, 230,                       # between the parents of word 3
         192, 500,                                  # child hits ON parent docs: ignored
         256,                                       # 1 child, the first bit of word 4
         301, 309,                                  # 2
         319, 320, 399,                             # 3, across the border of word 5
         447, 448, 449, 499]                        # 4, across the border of word 7
    A += list(range(501, 564))                      # 63
    A += list(range(601, 665))                      # 64, across word 10
    A += list(range(701, 766))                      # 65, across word 11
    A += [TILE - 2, TILE, TILE + 1, 2 * TILE - 70,  # around the tile borders
          69_950, 69_951]                           # behind the last parent below num_docs
    # (B inside A's long runs: no union of a unit below holds more than 65 children in one block)
    B = list(range(3, 500, 3)) + list(range(501, 564, 2)) + list(range(601, 665, 4)) + list(range(701, 766, 5))
    B += [TILE - 2, TILE, 2 * TILE - 70, 2 * TILE - 69, 69_950, N - 1]
    Cc = list(range(5, 500, 5)) + list(range(520, 540)) + list(range(610, 700, 9)) + list(range(69_940, 69_960))
    D = [7, 256, 320, 448, 702, 900, TILE + 5, 60_000]
    LONG = list(range(2 * TILE + 1, 69_000))        # fills the block longer than two tiles
    lists = []
    for docs in (A, B, Cc, D, LONG):
        d = np.array(sorted(set(docs)), np.uint32)
        lists.append((d, (1 + d % 3).astype(np.uint32)))
    norms = (np.arange(N, dtype=np.uint32) * 7 % 200 + 20).astype(np.uint8)
    seg = synth.segment_from_lists(lists, N, layout, norms=norms)
    parents = [1, 2,                                 # an empty first block; two adjacent parents
               192, 223, 224, 255,                   # bits 0, 31, 32, 63 of word 3
               300, 310, 400, 500, 600, 700, 800, 1_000,
               TILE - 1,                             # the last bit of tile 0: a block ends on the border ...
               2 * TILE - 100]                       # ... and this one begins on it (child at TILE)
    parents += list(range(2 * TILE - 64, 2 * TILE))  # a word of 64 parents, the last word of tile 1
    parents += [2 * TILE]                            # the first bit of tile 2; then none for > 2 tiles
    parents += [69_000, 69_900]                      # the long block's parent; the last one below num_docs
    return seg, N, np.array(sorted(set(parents)), np.int64)


TA, TB, TC, TD, TLONG = range(5)


def block_filters():
    T = by_term
    return [X(Or([T(TA), T(TB)])), X(And([T(TA), T(TB)])), X(Or([T(TA), T(TB), T(TC)], min_match=2)),
            X(And([Or([T(TA), T(TD)]), Or([T(TB), T(TC, 2.0)])])), X(T(TA, 0.5)),
            X(Or([T(TA), T(TB, 2.0)], merge=MERGE_MAX))]


def case_blocks(L, layout):
    seg, N, parents = hand_segment(layout)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    nw = N // 64 + 1
    n1 = N + 1
    dead = deleted_of(seg)
    rows = {"hand": bits(parents, nw), "with_last": bits(list(parents) + [N], nw),
            "empty": np.zeros(nw, np.uint64), "all": np.full(nw, ~np.uint64(0))}
    triples = block_filters()
    long_triples = [X(by_term(TLONG)), X(Or([by_term(TLONG), by_term(TA)], merge=MERGE_MIN))]
    seen = set()
    for scorer in (BM25(), TFIDF(True)):
        child = [child_of(seg, t, scorer) for t in triples]
        b = sd.batch_of(sr, "flat", triples, scorer, st, k=100)
        for name, row in rows.items():
            if name in ("empty", "all") and not isinstance(scorer, BM25):
                continue
            blocks = [blocks_of(row, N, m) for _, m in child]
            if name == "hand":      # what the segment is built for
                sizes = {len(k) for _, k in blocks[4]}      # (the unit of term A alone)
                assert {0, 1, 2, 3, 4, 63, 64, 65} <= sizes, sizes
                assert child[4][1][500] and child[4][1][192]      # child hits on parent docs
            for match in MATCHES if name in ("hand", "with_last") else [(0, 0), (1, None), (0, 2)]:
                sets, counts = b.nested_sets(row, match)
                exp = [restate(blocks[q], child[q][0], dead, match, MERGE_SUM, 0.0, n1) for q in range(b.nq)]
                for q in range(b.nq):
                    check_sets((name, match, q), sets[q], counts[q], exp[q][0], nw)
                    seen.add((name, match, bool(exp[q][0].any())))
                for merge in MERGES if name == "hand" else [MERGE_SUM]:
                    hits, cnt, tot = b.nested_topk(row, match, merge, none_boost=1.5)
                    for q in range(b.nq):
                        hit, score, c_max = restate(blocks[q], child[q][0], dead, match, merge, 1.5, n1)
                        assert c_max <= 65
                        check_topk((name, match, merge, q), hits[q], cnt[q], tot[q], b.k, hit, score,
                                   tol_of(match, merge, c_max))
                        if match == (0, None) and merge == MERGE_MIN:     # the quirk: MIN from 0
                            assert (hits[q, :int(cnt[q])]["score"] == 0).all()
        b.close()
        # the block longer than two tiles: sets and counts, and scores under MAX / MIN
        lb = sd.batch_of(sr, "flat", long_triples, scorer, st, k=100)
        lchild = [child_of(seg, t, scorer) for t in long_triples]
        lblocks = [blocks_of(rows["hand"], N, m) for _, m in lchild]
        assert max(len(k) for _, k in lblocks[0]) > 2 * TILE
        for match in ((1, None), (0, 0), (2, None), (0, 2)):
            sets, counts = lb.nested_sets(rows["hand"], match)
            for q in range(lb.nq):
                check_sets(("long", match, q), sets[q], counts[q],
                           restate(lblocks[q], lchild[q][0], dead, match, MERGE_SUM, 0.0, n1)[0], nw)
            for merge in (MERGE_MAX, MERGE_MIN):
                hits, cnt, tot = lb.nested_topk(rows["hand"], match, merge)
                for q in range(lb.nq):
                    hit, score, _ = restate(lblocks[q], lchild[q][0], dead, match, merge, 0.0, n1)
                    check_topk(("long", match, merge, q), hits[q], cnt[q], tot[q], lb.k, hit, score, parity.REL_TOL)
        lb.close()
    # what the rows say: an empty row hits nothing, also under {0, 0}; a full row only under {0, *}
    assert ("empty", (0, 0), True) not in seen and ("empty", (1, None), True) not in seen
    assert ("all", (0, 0), True) in seen and ("all", (1, None), True) not in seen
    assert ("hand", (3, 3), True) in seen and ("with_last", (1, 1), True) in seen
    sr.close()


def case_abi(L):
    seg = synth.build_segment(6_000, 48, with_positions=True)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    N = seg.num_docs
    T = lambda *ts: [by_term(t) for t in ts]
    triples = [X(Or(T(0, 1))), X(And(T(0, 2))), X(Or(T(1, 2, 3), min_match=2), [4])]
    b = sd.batch_of(sr, "flat", triples, BM25(), st, k=10)
    nw = b.match_words()
    wide = nw + 3
    parents = np.arange(8, N + 1, 8)
    dbuf = search.DeviceBuffer(L, 0, wide * 8).upload(bits(parents, wide))
    sets, counts = np.zeros((b.nq, wide), np.uint64), np.zeros(b.nq, np.uint64)
    hits, cnt, tot = np.zeros((b.nq, 10), _lib.HIT), np.zeros(b.nq, np.uint32), np.zeros(b.nq, np.uint64)

    def desc(ptr=dbuf.ptr, n_words=wide, lo=1, hi=_lib.NESTED_NO_MAX, merge=0, boost=0.0):
        d = _lib.Nested()
        d.d_parents, d.n_words, d.match_min, d.match_max, d.merge, d.none_boost = ptr, n_words, lo, hi, merge, boost
        return d

    def call_sets(d, s=sets, c=counts, handle=b.handle):
        import ctypes as C
        return L.irs_hip_batch_nested_sets(handle, None if d is None else C.byref(d), None if s is None else s.ctypes.data,
                                           None if c is None else c.ctypes.data)

    def call_topk(d, h=hits, stride=10, c=cnt, t=tot, handle=b.handle):
        import ctypes as C
        return L.irs_hip_batch_nested_topk(handle, None if d is None else C.byref(d), None if h is None else h.ctypes.data,
                                           stride, None if c is None else c.ctypes.data, None if t is None else t.ctypes.data)
    # before any run; every status next to the same call made legally
    for call in (call_sets, call_topk):
        assert call(desc()) == _lib.OK
        assert call(desc(), handle=None) == _lib.EINVAL
        assert call(None) == _lib.EINVAL
        assert call(desc(ptr=None)) == _lib.EINVAL
        assert call(desc(n_words=N // 64)) == _lib.EINVAL and call(desc(n_words=0)) == _lib.EINVAL   # too small
        assert call(desc(n_words=(1 << 26) + 1)) == _lib.EINVAL
        assert call(desc(lo=3, hi=2)) == _lib.EINVAL and call(desc(lo=2, hi=2)) == _lib.OK
        assert call(desc(merge=3)) == _lib.EINVAL and call(desc(merge=2)) == _lib.OK
        for bad in (-1.0, float("nan"), float("inf")):
            assert call(desc(lo=0, hi=0, boost=bad)) == _lib.EINVAL and call(desc(boost=bad)) == _lib.EINVAL
        assert call(desc(lo=0, hi=0, boost=2.0)) == _lib.OK
    assert call_sets(desc(), None, None) == _lib.EINVAL
    assert call_topk(desc(), None, 10, None, None) == _lib.EINVAL
    assert call_topk(desc(), stride=9) == _lib.EINVAL and call_topk(desc(), stride=11, h=np.zeros((b.nq, 11), _lib.HIT)) == _lib.OK
    import ctypes as C
    assert L.irs_hip_batch_nested_sets_to_device(b.handle, C.byref(desc()), None, None, None) == _lib.EINVAL
    # sets alone, counts alone; the words of a row beyond the segment are written as 0
    sets[:] = ~np.uint64(0)
    assert call_sets(desc(), c=None) == _lib.OK
    first = sets.copy()
    assert (first[:, nw:] == 0).all() and first.any()
    counts[:] = 7
    assert call_sets(desc(), s=None) == _lib.OK
    child = [child_of(seg, t, BM25()) for t in triples]
    dead = deleted_of(seg)
    exp = [restate(blocks_of(bits(parents, wide), N, m), sc, dead, (1, None), MERGE_SUM, 0.0, N + 1) for sc, m in child]
    for q in range(b.nq):
        check_sets(("abi", q), first[q], counts[q], exp[q][0], wide)
    # a run, the calls, a second run, the calls again: the hits and re-runs of a batch left alone
    plain = sd.batch_of(sr, "flat", triples, BM25(), st, k=10)
    p1 = tuple(x.copy() for x in plain.run().results())
    p2 = tuple(x.copy() for x in plain.run().results())
    plain_reruns = plain.reruns()
    plain.close()
    g1 = tuple(x.copy() for x in b.run().results())
    n1 = b.nested_topk(dbuf.ptr, n_words=wide)
    s1 = b.nested_sets(dbuf.ptr, n_words=wide)
    g2 = tuple(x.copy() for x in b.run().results())
    n2 = b.nested_topk(dbuf.ptr, n_words=wide)
    s2 = b.nested_sets(dbuf.ptr, n_words=wide)
    assert b.reruns() == plain_reruns
    for x, y in zip(p1 + p2 + n1 + s1, g1 + g2 + n2 + s2):
        assert np.array_equal(x, y), "a run or a call changed by the nested calls"
    assert np.array_equal(s1[0], first)
    for q in range(b.nq):
        check_topk(("abi topk", q), n1[0][q], n1[1][q], n1[2][q], 10, exp[q][0], exp[q][1], tol_of((1, None), MERGE_SUM, exp[q][2]))
    b.close()
    # refused by both calls, and afterwards still running: by_terms, an Or of clauses, a tree
    row = bits(parents, nw)
    for flt, flags in ((by_terms([(0, 1.0), (1, 1.0), (2, 0.5)]), {}),
                       (Or([And(T(0, 1)), by_term(2)]), {"and_clauses": True}),
                       (And([by_term(0), Or([by_term(1), And(T(2, 3))])]), {"boolean_trees": True})):
        rb = sr.batch(search.prepare([flt], BM25(), st, **flags), 10)
        before = tuple(x.copy() for x in rb.run().results())
        for fn in (rb.nested_sets, rb.nested_topk):
            for match in ((1, None), (0, 0)):
                with pytest.raises(_lib.IrsHipError) as e:
                    fn(row, match)
                assert e.value.status == _lib.EUNSUPPORTED, flt
        for x, y in zip(before, tuple(x.copy() for x in rb.run().results())):
            assert np.array_equal(x, y)
        rb.close()
    # a phrase batch: taken by _sets, refused by _topk except under {0, 0}
    for flt, flags in ((by_phrase([0, 1]), {}), (Or([by_phrase([0, 1]), by_term(2)]), {"optional_terms": True})):
        rb = sr.batch(search.prepare([flt], BM25(), st, **flags), 10)
        m = unbits(rb.match_sets(nw)[0][0], N + 1)
        blocks = blocks_of(row, N, m)
        for match in ((1, None), (0, 0), (2, 3)):
            s, c = rb.nested_sets(row, match)
            check_sets(("phrase", match), s[0], c[0], restate(blocks, None, dead, match, MERGE_SUM, 0.0, N + 1)[0] if match == (0, 0)
                       else restate(blocks, np.zeros(N + 1), dead, match, MERGE_SUM, 0.0, N + 1)[0], nw)
        with pytest.raises(_lib.IrsHipError) as e:
            rb.nested_topk(row, (1, None))
        assert e.value.status == _lib.EUNSUPPORTED
        h, c, t = rb.nested_topk(row, (0, 0), none_boost=0.25)
        hit, score, _ = restate(blocks, None, dead, (0, 0), MERGE_SUM, 0.25, N + 1)
        check_topk(("phrase none",), h[0], c[0], t[0], 10, hit, score, parity.REL_TOL)
        rb.close()
    dbuf.close()
    sr.close()


def case_masks(L):
    seg, N, parents = hand_segment(synth.LAYOUT_SIMD4)
    # deleted: some children, some parents, every child of the block of parent 310
    seg.doc_mask = np.array(sorted({520, 601, 300, 600, 2 * TILE - 3, 301, 303, 305, 306, 309, 69_900}), np.uint32)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    nw, n1 = N // 64 + 1, N + 1
    dead = deleted_of(seg)
    row = bits(parents, nw)
    inset = np.zeros(64 * nw, bool)
    inset[np.arange(2, N + 1, 2)] = True
    T = by_term
    inner = [X(Or([T(TA), T(TB)])), X(Or([T(TA), T(TB)]), [TC]), X(And([T(TA), T(TB)]), [TD]), X(Or([T(TA), T(TC)]))]
    filters = [t[0] for t in inner[:3]] + [And([inner[3][0], by_doc_set(0)])]
    b = sr.batch(search.prepare(filters, BM25(), st), 50, doc_sets=bits(np.nonzero(inset)[0], nw).reshape(1, nw))
    child = [child_of(seg, t, BM25(), inset=inset if q == 3 else None) for q, t in enumerate(inner)]
    blocks = [blocks_of(row, N, m) for _, m in child]
    assert all(len(k) == 0 for bl in blocks for p, k in bl if p == 310) and not child[0][1][520]
    for match in MATCHES:
        sets, counts = b.nested_sets(row, match)
        for merge in MERGES:
            hits, cnt, tot = b.nested_topk(row, match, merge, none_boost=3.0)
            for q in range(b.nq):
                hit, score, c_max = restate(blocks[q], child[q][0], dead, match, merge, 3.0, n1)
                assert not hit[[300, 600, 69_900]].any()        # deleted parents delimit, and are no hits
                if merge == MERGE_SUM:
                    check_sets(("masks", match, q), sets[q], counts[q], hit, nw)
                check_topk(("masks", match, merge, q), hits[q], cnt[q], tot[q], 50, hit, score, tol_of(match, merge, c_max))
    b.close()
    sr.close()


def case_topk(L):
    seg = synth.build_segment(40_000, 64)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    N = seg.num_docs
    nw, n1 = N // 64 + 1, N + 1
    dead = deleted_of(seg)
    T = lambda *ts: [by_term(t) for t in ts]
    triples = [X(Or(T(0, 1, 2))), X(And(T(0, 1))), X(by_term(30))]
    many = bits(np.arange(3, N + 1, 3), nw)      # more hit parents than kSelectStage in unit 0
    few = bits(np.arange(50, N + 1, 50), nw)
    child = [child_of(seg, t, BM25()) for t in triples]
    for k, row in ((1, many), (10, many), (_lib.MAX_K, few)):
        b = sd.batch_of(sr, "flat", triples, BM25(), st, k=k)
        blocks = [blocks_of(row, N, m) for _, m in child]
        for match, merge in (((1, None), MERGE_SUM), ((0, None), MERGE_MAX), ((1, 2), MERGE_MIN), ((0, 0), MERGE_SUM)):
            hits, cnt, tot = b.nested_topk(row, match, merge, none_boost=0.5)
            for q in range(b.nq):
                hit, score, c_max = restate(blocks[q], child[q][0], dead, match, merge, 0.5, n1)
                check_topk(("topk", k, match, q), hits[q], cnt[q], tot[q], k, hit, score, tol_of(match, merge, c_max))
                if row is many and q == 0 and match == (1, None):
                    assert hit.sum() > SELECT_STAGE
                if row is few:
                    assert hit.sum() < k
        b.close()
    # zero boosts: every score 0, the order is by doc id; {0, 0} with a boost gives the same order
    zero = [X(Or([by_term(0, 0.0), by_term(1, 0.0)]))]
    b = sd.batch_of(sr, "flat", zero, BM25(), st, k=10)
    h, c, t = b.nested_topk(few, (1, None))
    m = child_of(seg, zero[0], BM25())[1]
    want = [p for p, kids in blocks_of(few, N, m) if len(kids)][:10]
    assert int(c[0]) == 10 and (h[0]["score"] == 0).all() and h[0]["doc"].tolist() == want
    h, c, t = b.nested_topk(few, (0, 0), none_boost=2.0)
    want = [p for p, kids in blocks_of(few, N, m) if not len(kids)][:10]
    assert (h[0, :int(c[0])]["score"] == 2.0).all() and h[0, :int(c[0])]["doc"].tolist() == want
    b.close()
    sr.close()


def case_multi(L):
    sizes, ranks = (9_000, 4_000, 14_000), (96, 40, 80)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    segs = [synth.build_segment(int(n), int(r), first_doc=int(f)) for n, r, f in zip(sizes, ranks, first)]
    segs[1].doc_mask = np.arange(10, 400, dtype=np.uint32)
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    stats = [parity.segment_stats(s) for s in segs]
    T = lambda *ts: [by_term(t) for t in ts]
    triples = [X(Or(T(1, 60))), X(And(T(0, 60))), X(by_term(2))]      # term 60: absent from the middle segment
    b = sd.batch_of(readers, "flat", triples, BM25(), stats, k=20)
    nw = b.match_words()
    steps = (7, 4, 11)
    rows = np.stack([bits(np.arange(s, n + 1, s), nw) for s, n in zip(steps, sizes)])
    for match, merge in (((1, None), MERGE_SUM), ((2, 3), MERGE_MAX), ((0, 0), MERGE_SUM)):
        sets, counts = b.nested_sets(rows, match)
        hits, cnt, tot = b.nested_topk(rows, match, merge, none_boost=1.0)
        for i, s in enumerate(segs):
            for q, t in enumerate(triples):
                u = i * len(triples) + q
                sc, m = child_of(s, t, BM25(), segs)
                hit, score, c_max = restate(blocks_of(rows[i], s.num_docs, m), sc, deleted_of(s), match, merge, 1.0, s.num_docs + 1)
                check_sets(("multi", match, u), sets[u], counts[u], hit, nw)
                check_topk(("multi", match, u), hits[u], cnt[u], tot[u], 20, hit, score, tol_of(match, merge, c_max))
    assert not child_of(segs[1], triples[1], BM25(), segs)[1].any()
    b.close()
    for r in readers:
        r.close()


def case_groups(L):
    seg = synth.build_segment(20_000, 64)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    N = seg.num_docs
    nw = N // 64 + 1
    triples = [X(Or([by_term(t), by_term(t + 1)])) for t in range(12)]
    row = bits(np.arange(5, N + 1, 5), nw)
    b = sd.batch_of(sr, "flat", triples, BM25(), st, k=25)
    assert b.nq == 12
    old = os.environ.pop("IRS_HIP_NESTED_SCRATCH_MB", None)
    try:
        base = b.nested_topk(row, (1, None), MERGE_SUM)
        os.environ["IRS_HIP_NESTED_SCRATCH_MB"] = "0"       # every unit a group of its own: 12 groups
        split = b.nested_topk(row, (1, None), MERGE_SUM)
    finally:
        os.environ.pop("IRS_HIP_NESTED_SCRATCH_MB", None)
        if old is not None:
            os.environ["IRS_HIP_NESTED_SCRATCH_MB"] = old
    for x, y in zip(base, split):
        assert np.array_equal(x, y)
    assert (base[1] == 25).all()
    sc, m = child_of(seg, triples[5], BM25())
    hit, score, c_max = restate(blocks_of(row, N, m), sc, deleted_of(seg), (1, None), MERGE_SUM, 0.0, N + 1)
    check_topk(("groups", 5), base[0][5], base[1][5], base[2][5], 25, hit, score, tol_of((1, None), MERGE_SUM, c_max))
    b.close()
    sr.close()


def case_chain(L):
    """d.x == 1 AND d.children[? ANY ...]: the nested filter's device rows as the doc sets of a
    parent-level batch."""
    seg = synth.build_segment(12_000, 64)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    N = seg.num_docs
    nw, n1 = N // 64 + 1, N + 1
    parents = np.arange(4, N + 1, 4)
    kids = [X(Or([by_term(20), by_term(21)])), X(by_term(9))]
    cb = sd.batch_of(sr, "flat", kids, BM25(), st, k=10)
    d_sets = search.DeviceBuffer(L, 0, cb.nq * nw * 8)
    d_counts = search.DeviceBuffer(L, 0, cb.nq * 8)
    cb.nested_sets_to_device(bits(parents, nw), d_sets.ptr, d_counts.ptr, (1, None))
    want_hit = [restate(blocks_of(bits(parents, nw), N, m), sc, deleted_of(seg), (1, None), MERGE_SUM, 0.0, n1)[0]
                for sc, m in (child_of(seg, t, BM25()) for t in kids)]
    got = d_sets.download(np.uint64, (cb.nq, nw))
    for q in range(cb.nq):
        check_sets(("chain rows", q), got[q], d_counts.download(np.uint64, (cb.nq,))[q], want_hit[q], nw)
    tops = [X(Or([by_term(0), by_term(1)])), X(by_term(2)), X(And([by_term(0), by_term(3)]))]
    pb = sd.batch_of(sr, "flat", tops, BM25(), st, k=30)
    rows_of = [0, 1, 0]
    pb.set_doc_sets(d_sets.ptr, rows_of, n_rows=cb.nq, n_words=nw)
    hits, cnt, tot = pb.run().results()
    for q, t in enumerate(tops):
        sc, m = child_of(seg, t, BM25())
        m = m & want_hit[rows_of[q]]
        check_topk(("chain", q), hits[q], cnt[q], tot[q], 30, m, np.where(m, sc, 0.0), parity.REL_TOL)
        assert 0 < m.sum() < child_of(seg, t, BM25())[1].sum()
    pb.close()
    cb.close()
    d_sets.close()
    d_counts.close()
    sr.close()


# ------------------------------------------------------------------- CPU --

def test_symbols_exist(simlib):
    for name in ("irs_hip_batch_nested_sets", "irs_hip_batch_nested_sets_to_device", "irs_hip_batch_nested_topk"):
        assert hasattr(simlib, name)


def test_constants_read_from_the_source():
    assert TILE_WORDS % 64 == 0 and 1 < LONG_RUN < 63 and SELECT_STAGE == 8192


def test_nested_abi_emulated(simlib):
    case_abi(simlib)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_nested_blocks_emulated(simlib, layout):
    case_blocks(simlib, layout)


def test_nested_masks_emulated(simlib):
    case_masks(simlib)


def test_nested_topk_emulated(simlib):
    case_topk(simlib)


def test_nested_multi_emulated(simlib):
    case_multi(simlib)


def test_nested_groups_emulated(simlib):
    case_groups(simlib)


def test_nested_chain_emulated(simlib):
    case_chain(simlib)


# --------------------------------------------------------------------- GPU --

@pytest.mark.gpu
def test_nested_abi_gpu(gpulib):
    case_abi(gpulib)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_nested_blocks_gpu(gpulib, layout):
    case_blocks(gpulib, layout)


@pytest.mark.gpu
def test_nested_masks_gpu(gpulib):
    case_masks(gpulib)


@pytest.mark.gpu
def test_nested_topk_gpu(gpulib):
    case_topk(gpulib)


@pytest.mark.gpu
def test_nested_multi_gpu(gpulib):
    case_multi(gpulib)


@pytest.mark.gpu
def test_nested_groups_gpu(gpulib):
    case_groups(gpulib)


@pytest.mark.gpu
def test_nested_chain_gpu(gpulib):
    case_chain(gpulib)
