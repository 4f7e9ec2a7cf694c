"""irs::Not in an And (IRS_HIP_EXCLUDE): the included part's matches minus the docs of the
excluded terms — exclusion(incl, disjunction(excluded)), boolean_query.cpp:121-141, exclusion.hpp.

An exclusion is a per-query deletion, so the expected value needs nothing new from the oracle: a
query with excluded terms on segment S equals the same query without them on S opened with
doc_mask = deletions + every doc of the excluded terms (the scorer statistics are the same on both
sides).  One body runs on the emulator (CPU tier) and on the GPU at a larger size."""
from __future__ import annotations

import copy
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import parity
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, TFIDF, And, Not, Or, by_phrase, by_term


def _docs(seg, term):
    if not (0 <= term < len(seg.metas)) or int(seg.metas[term]["docs_count"]) == 0:
        return np.zeros(0, np.int64)
    d, _ = oracle.decode_term(seg.doc_file, seg.metas[term], seg.layout,
                              wand_count=int(getattr(seg, "wand_count", 0)))
    return d.astype(np.int64)


def _gone(seg):
    m = getattr(seg, "doc_mask", None)
    if m is None:
        return np.zeros(0, np.int64)
    m = np.asarray(m, np.int64)
    return np.unique(m[(m >= 1) & (m <= seg.num_docs)])


def _masked(seg, excluded):
    """seg with doc_mask = its deletions + every doc of the excluded terms."""
    out = copy.copy(seg)
    parts = [_gone(seg)] + [_docs(seg, t) for t in excluded]
    out.doc_mask = np.unique(np.concatenate(parts)).astype(np.uint32)
    if out.doc_mask.size == 0:
        out.doc_mask = None
    return out


def _bits(docs, n_words):
    b = np.zeros(n_words, np.uint64)
    docs = np.asarray(docs, np.int64)
    docs = docs[docs < 64 * n_words]
    np.bitwise_or.at(b, docs // 64, np.uint64(1) << (docs % 64).astype(np.uint64))
    return b


def _check(seg, incl, excluded, scorer, k, h, c, t, all_segs=None):
    ms = _masked(seg, excluded)
    if isinstance(incl, by_phrase):
        parity.check_phrase_segment(ms, [incl], scorer, k, h[None], c[None], t[None], all_segs)
    else:
        parity.check_single_segment(ms, [incl], scorer, k, h[None], c[None], t[None], all_segs)


def exclusion_filters(max_rank):
    """(filter, included part, excluded terms) triples: OR, MINMATCH, AND with 1-3 excluded
    terms — an absent one, one equal to an included term, one covering every match, the most
    frequent terms (their docs hold most of the unexcluded top k)."""
    rng = np.random.default_rng(77)
    absent = 10 * max_rank
    rows = synth.make_queries(3, 8, 2, max_rank, synth.SEED + 21)
    out = []
    for i, row in enumerate(rows):
        incl = Or([by_term(int(r) - 1) for r in row])
        ex = [[max_rank - 5], [absent, 6], [0, 1]][i]
        out.append((And([incl] + [Not(by_term(x)) for x in ex]), incl, ex))
    incl = Or([by_term(1), by_term(5), by_term(9)])
    out.append((And([incl, Not(by_term(5))]), incl, [5]))                           # equal to an included term
    out.append((And([by_term(7), Not(by_term(7))]), And([by_term(7)]), [7]))        # covers every match
    incl = Or([by_term(3), by_term(max_rank // 4)], merge=search.MERGE_MAX)
    out.append((And([incl, Not(Or([by_term(0), by_term(2)]))]), incl, [0, 2]))      # the top k moves
    mm = [by_term(2), by_term(max_rank // 16), by_term(max_rank // 4), by_term(5), by_term(9)]
    incl = Or(mm, min_match=2)
    out.append((And([incl, Not(by_term(3)), Not(by_term(12))]), incl, [3, 12]))
    out.append((And([Or(mm, min_match=3), Not(by_term(absent))]), Or(mm, min_match=3), [absent]))
    out.append((And([by_term(0), by_term(1), Not(by_term(2))]), And([by_term(0), by_term(1)]), [2]))
    out.append((And([by_term(0), by_term(3), by_term(8), Not(by_term(max_rank // 2)), Not(by_term(40)),
                     Not(Not(Not(by_term(11))))]),
                And([by_term(0), by_term(3), by_term(8)]), [max_rank // 2, 40, 11]))
    incl = And([by_term(max_rank - 1), by_term(4)])
    x = int(rng.integers(20, 60))
    out.append((And([incl, Not(by_term(x))]), incl, [x]))
    return out


def exclusion_phrases():
    return [(And([by_phrase([0, 1]), Not(by_term(2))]), by_phrase([0, 1]), [2]),
            (And([by_phrase([1, 4, 0]), Not(by_term(100_000))]), by_phrase([1, 4, 0]), [100_000]),
            (And([by_phrase([2, 0]), Not(by_term(0))]), by_phrase([2, 0]), [0]),          # empty
            (And([by_phrase([0, 3], [0, 3]), Not(by_term(7)), Not(by_term(1))]), by_phrase([0, 3], [0, 3]), [7, 1])]


def _run(sr, filters, scorer, k, path=None, **kw):
    b = sr.batch(search.prepare(filters, scorer, kw.pop("stats")), k)
    if path is not None:
        b.set_path(path)
    h, c, t = (x.copy() for x in b.run().results())
    return b, h, c, t


def case_exclusion(L, num_docs, max_rank, layout, scorers, ks, bit_identity=True):
    """Parity with the oracle's masked run (both a plain segment and one with deletions), bit
    identity with the plain query on the union-masked segment, k_excl_mask against
    dead | bit_union(excluded), wand, min scores, a re-run, the joined path on a mixed batch."""
    seg0 = synth.build_segment(num_docs, max_rank, layout=layout, with_positions=True)
    rng = np.random.default_rng(2027)
    seg1 = copy.copy(seg0)
    seg1.doc_mask = np.concatenate([rng.choice(num_docs, num_docs // 20, replace=False).astype(np.uint32) + 1,
                                    np.arange(100, 700, dtype=np.uint32)])
    st = [parity.segment_stats(seg0)]
    trip = exclusion_filters(max_rank)
    phr = exclusion_phrases()
    filters = [f for f, _, _ in trip]
    n_words = (num_docs + 64) // 64
    for seg in (seg0, seg1):
        sr = search.SegmentReader.from_synth(seg, L=L)
        masked_readers = {}
        for scorer in scorers:
            for k in ks:
                for path in (_lib.PATH_AUTO, _lib.PATH_ITEMS):
                    b, h, c, t = _run(sr, filters, scorer, k, path, stats=st)
                    for q, (_, incl, ex) in enumerate(trip):
                        _check(seg, incl, ex, scorer, k, h[q], c[q], t[q])
                    b.close()
                assert int(t[4]) == 0 and int(c[4]) == 0          # the excluded term covers every match
                b, h, c, t = _run(sr, [f for f, _, _ in phr], scorer, k, stats=st)
                for q, (_, incl, ex) in enumerate(phr):
                    _check(seg, incl, ex, scorer, k, h[q], c[q], t[q])
                assert int(t[2]) == 0
                b.close()
        # the k-th boundary moved: the plain query's top k holds docs of the excluded terms
        b, h, c, _ = _run(sr, [trip[5][1]], BM25(), min(ks), stats=st)
        top = h[0, :int(c[0])]["doc"].astype(np.int64)
        assert np.isin(top, np.concatenate([_docs(seg, 0), _docs(seg, 2)])).mean() > 0.5
        b.close()
        # bit identity with the plain query on the union-masked segment, one query a batch
        if bit_identity:
            for flt, incl, ex in trip + phr:
                key = tuple(sorted(set(x for x in ex if 0 <= x < max_rank)))
                if key not in masked_readers:
                    masked_readers[key] = search.SegmentReader.from_synth(_masked(seg, key), L=L)
                for k in ks:
                    b, h, c, t = _run(sr, [flt], scorers[0], k, _lib.PATH_ITEMS, stats=st)
                    b.close()
                    b, h2, c2, t2 = _run(masked_readers[key], [incl], scorers[0], k, _lib.PATH_ITEMS, stats=st)
                    b.close()
                    assert np.array_equal(h, h2) and np.array_equal(c, c2) and np.array_equal(t, t2), (flt, k)
        # every unit's mask: dead | bit_union(excluded terms), bit for bit — one workgroup per
        # mask and a small slice (many slice boundaries)
        dead = _bits(_gone(seg), n_words)
        for slice_words in (None, "64"):
            if slice_words:
                os.environ["IRS_HIP_EXCL_SLICE"] = slice_words
            try:
                b, h, c, t = _run(sr, filters, BM25(), 25, stats=st)
            finally:
                os.environ.pop("IRS_HIP_EXCL_SLICE", None)
            for q, (_, _, ex) in enumerate(trip):
                got = b.unit_mask(q, n_words)
                present = [x for x in ex if 0 <= x < max_rank]
                want = dead | (sr.bit_union(present, n_words)[0] if present else 0)
                assert np.array_equal(got, want), q
            b.close()
        # wand (ExecutionContext::wand): the exhaustive top k
        k = max(ks)
        b, h0, c0, _ = _run(sr, filters, BM25(), k, stats=st)
        b.close()
        b = sr.batch(search.prepare(filters, BM25(), st), k).set_wand(True)
        hw, cw, _ = b.run().results()
        assert np.array_equal(hw, h0) and np.array_equal(cw, c0)
        b.close()
        # irs::score::Min pushed down, and a re-run of the same batch
        b = sr.batch(search.prepare(filters, BM25(), st), k)
        h1, c1, t1 = (x.copy() for x in b.run().results())
        h2, c2, t2 = (x.copy() for x in b.run().results())
        assert np.array_equal(h1, h2) and np.array_equal(c1, c2) and np.array_equal(t1, t2)
        kth = np.array([h1[q, c1[q] - 1]["score"] if c1[q] else 0.0 for q in range(len(filters))], np.float32)
        h3, c3, t3 = b.set_min_scores(kth).run().results()
        assert np.array_equal(h1, h3) and np.array_equal(c1, c3) and np.array_equal(t1, t3)
        b.close()
        # the joined path asked for on a mixed batch: the units with exclusions run as work items /
        # block driven (and pass parity), the others are bit for bit what they are without them
        plain = standard_plain(max_rank)
        for scorer in scorers:
            b = sr.batch(search.prepare(plain, scorer, st), k).set_path(_lib.PATH_JOINED)
            hp, cp, tp = (x.copy() for x in b.run().results())
            pp = b.paired_tiles()
            b.close()
            b = sr.batch(search.prepare(plain + filters, scorer, st), k).set_path(_lib.PATH_JOINED)
            hm, cm, tm = b.run().results()
            assert b.paired_tiles() == pp
            n = len(plain)
            assert np.array_equal(hm[:n], hp) and np.array_equal(cm[:n], cp) and np.array_equal(tm[:n], tp)
            for q, (_, incl, ex) in enumerate(trip):
                _check(seg, incl, ex, scorer, k, hm[n + q], cm[n + q], tm[n + q])
            b.close()
            # (a unit whose excluded terms are all absent has no mask: it may join)
            masked = [f for f, _, ex in trip if any(0 <= x < max_rank for x in ex)]
            b = sr.batch(search.prepare(masked, scorer, st), k).set_path(_lib.PATH_JOINED)
            b.run().results()
            assert b.path() == _lib.PATH_ITEMS
            b.close()
        for r in masked_readers.values():
            r.close()
        sr.close()


def standard_plain(max_rank):
    """Queries without exclusions, among them every included part above."""
    ranks = synth.make_queries(4, 8, 2, max_rank, synth.SEED + 5)
    fl = [Or([by_term(int(r) - 1) for r in row]) for row in ranks]
    fl += [incl for _, incl, _ in exclusion_filters(max_rank)]
    return fl


def case_exclusion_lists(L, layout):
    """k_excl_mask on hand-made lists: a single-doc term, a tail-only term, a term of exact
    blocks, a dense one crossing every slice, docs on slice boundaries; every slice size."""
    num_docs = 9_000
    rng = np.random.default_rng(5)
    lists = []
    def add(docs):
        docs = np.unique(np.asarray(docs, np.uint32))
        lists.append((docs, np.ones(docs.size, np.uint32) + (docs % 3).astype(np.uint32)))
    add([num_docs])                                       # single doc, the last one
    add([1])                                              # single doc, the first one
    add(rng.choice(num_docs, 90, replace=False) + 1)      # tail only
    add(np.arange(1, 257))                                # exactly two blocks
    add(np.arange(1, num_docs + 1, 2))                    # dense: blocks in every slice
    add(np.concatenate([np.arange(2040, 2060), np.arange(4090, 4100), [2048, 2049, 4096, 4097, 8192]]))
    add(rng.choice(num_docs, 3000, replace=False) + 1)
    seg = synth.segment_from_lists(lists, num_docs, layout)
    gone = np.array([3, 2049, 2050, 8191, num_docs], np.uint32)
    seg.doc_mask = gone
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    n_words = (num_docs + 64) // 64
    sets = [[0], [1], [2], [3], [4], [5], [6], [0, 1, 2, 3, 4, 5], [2, 6], [1, 3]]
    filters = [And([by_term(6 if 6 not in s else 4), *[Not(by_term(x)) for x in s]]) for s in sets]
    filters.append(And([by_term(6), Not(by_term(4))]))      # the same mask as set [4]: shared
    dead = _bits(gone, n_words)
    for slice_words in (None, "64", "128", "8192"):
        if slice_words:
            os.environ["IRS_HIP_EXCL_SLICE"] = slice_words
        try:
            b = sr.batch(search.prepare(filters, BM25(), st), 10)
        finally:
            os.environ.pop("IRS_HIP_EXCL_SLICE", None)
        h, c, t = b.run().results()
        for q, s in enumerate(sets):
            want = dead | sr.bit_union(s, n_words)[0]
            assert np.array_equal(b.unit_mask(q, n_words), want), (slice_words, s)
            incl = by_term(6 if 6 not in s else 4)
            _check(seg, And([incl]), s, BM25(), 10, h[q], c[q], t[q])
        b.close()
    sr.close()


def case_exclusion_multi(L, sizes, max_rank=256, k=100):
    """create_multi with a shared threshold, each segment its own ordinals (an excluded term
    missing from one segment), merged on the host and with irs_hip_merge_topk."""
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    segs = [synth.build_segment(int(n), max_rank, first_doc=int(f)) for n, f in zip(sizes, first)]
    segs[1].metas[max_rank - 5]["docs_count"] = 0
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    trip = exclusion_filters(max_rank)
    filters = [f for f, _, _ in trip]
    stats = [parity.segment_stats(s) for s in segs]
    prep = search.prepare(filters, BM25(), stats)
    plain = search.QueryBatch(readers, prep, k)
    ph, pc, pt = plain.run().results()
    for i, s in enumerate(segs):
        for q, (_, incl, ex) in enumerate(trip):
            _check(s, incl, ex, BM25(), k, ph[i, q], pc[i, q], pt[i, q], segs)
    shared = search.QueryBatch(readers, prep, k).set_shared_threshold(True)
    sh, sc, st_ = shared.run().results()
    assert np.array_equal(pt, st_)
    mp = search.merge_topk_host([(ph[i], pc[i]) for i in range(len(segs))], k)
    ms = search.merge_topk_host([(sh[i], sc[i]) for i in range(len(segs))], k)
    assert mp == ms
    # the merged top k is the oracle's heap over the masked segments
    for q, (_, incl, ex) in enumerate(trip):
        ref = parity.oracle_topk([_masked(s, ex) for s in segs], [incl], BM25(), k)[0][0]
        a = np.array([r[0] for r in ms[q]], np.float32)
        assert a.size == ref.size and np.allclose(a, np.sort(ref["score"])[::-1], rtol=parity.REL_TOL, atol=0), q
    # irs_hip_merge_topk over per-segment batches
    import torch
    from iresearch_amd import distributed
    arch = C.create_string_buffer(64)
    L.irs_hip_device_arch(0, arch, 64)
    dev = "cpu" if arch.value.endswith(b"-sim") else "cuda"
    lists, batches = [], []
    for i, r in enumerate(readers):
        b = r.batch(prep, k)
        b.run()
        h = torch.zeros((len(filters), k), dtype=torch.int64, device=dev)
        c = torch.zeros((len(filters),), dtype=torch.int32, device=dev)
        b.results_to_device(h.data_ptr(), c.data_ptr())
        if dev == "cuda":
            torch.cuda.synchronize()
        lists.append((i, h, c))
        batches.append(b)
    oh, os_, oc = distributed.gather_merge(L, 0, lists, len(segs), 0, 1, len(filters), k, dev)
    if dev == "cuda":
        torch.cuda.synchronize()
    gh = distributed.hits_from_int64(oh)
    gs, gc = os_.cpu().numpy(), oc.cpu().numpy()
    for q, rows in enumerate(mp):
        assert gc[q] == len(rows)
        got = [(float(gh[q, i]["score"]), int(gs[q, i]), int(gh[q, i]["doc"])) for i in range(len(rows))]
        assert got == [(float(np.float32(a)), s, d) for a, s, d in rows], q
    for b in batches + [plain, shared]:
        b.close()
    for r in readers:
        r.close()


def case_exclusion_abi(L):
    """irs_hip_batch_create refuses malformed exclusions with EINVAL."""
    seg = synth.build_segment(5_000, 64)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]

    def create(prep, edit=None):
        arr = search.QueryArrays.from_prepared([sr], prep, 10)
        if edit:
            edit(arr)
        h = C.c_void_p()
        rc = L.irs_hip_batch_create(sr.handle, arr.queries.ctypes.data, len(arr.queries),
                                    arr.terms.ctypes.data, arr.terms.shape[1], C.byref(h))
        if rc == 0:
            L.irs_hip_batch_destroy(h)
        return rc

    good = search.prepare([And([by_term(1), by_term(2), Not(by_term(3))])], BM25(), st)
    assert create(good) == _lib.OK
    # excluded before included: swap the last two entries
    def swap(arr):
        arr.terms[0, [1, 2]] = arr.terms[0, [2, 1]]
    assert create(good, swap) == _lib.EINVAL
    # only excluded
    def only(arr):
        arr.terms[0, :]["kind"] = _lib.EXCLUDE
    assert create(good, only) == _lib.EINVAL
    # too many excluded (IRS_HIP_MAX_EXCLUDED) — and exactly as many is fine
    many = search.prepare([And([by_term(1)] + [Not(by_term(t)) for t in range(2, 2 + _lib.MAX_EXCLUDED + 1)])], BM25(), st)
    assert create(many) == _lib.EINVAL
    most = search.prepare([And([by_term(1)] + [Not(by_term(t)) for t in range(2, 2 + _lib.MAX_EXCLUDED)])], BM25(), st)
    assert create(most) == _lib.OK
    # the included entries keep their own limit; the excluded ones do not count against it
    full = search.prepare([And([by_term(t) for t in range(_lib.MAX_TERMS)] + [Not(by_term(40))])], BM25(), st)
    assert create(full) == _lib.OK
    # an unknown kind among the excluded entries, an ordinal beyond the term table
    def unknown(arr):
        arr.terms[0, 2]["kind"] = _lib.EXCLUDE + 1
    assert create(good, unknown) == _lib.EINVAL
    def beyond(arr):
        arr.terms[0, 2]["term"] = 1_000_000
    assert create(good, beyond) == _lib.EINVAL
    sr.close()


# ---------------------------------------------------------------- emulator --

def test_exclusion_emulated(simlib):
    case_exclusion(simlib, 20_000, 96, synth.LAYOUT_SIMD4, (BM25(), TFIDF(True)), (25,))


def test_exclusion_emulated_scalar(simlib):
    case_exclusion(simlib, 12_000, 64, synth.LAYOUT_SCALAR, (TFIDF(False),), (25,), bit_identity=False)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_exclusion_lists_emulated(simlib, layout):
    case_exclusion_lists(simlib, layout)


def test_exclusion_multi_emulated(simlib):
    case_exclusion_multi(simlib, (9_000, 4_000, 14_000), max_rank=96, k=50)


def test_exclusion_abi_emulated(simlib):
    case_exclusion_abi(simlib)


def test_prepare_exclusions():
    st = [search.SegmentStats(1000, 100_000, np.full(64, 50, np.int64))]
    p = search.prepare([And([by_term(1), by_term(2), Not(by_term(3)), Not(Or([by_term(4), by_term(5)]))])], BM25(), st)[0]
    assert p.op == _lib.OP_AND and p.terms == [1, 2] and p.excluded == [3, 4, 5]
    # a single included child keeps its op, min_match and merge
    p = search.prepare([And([Or([by_term(1), by_term(2), by_term(3)], min_match=2, merge=search.MERGE_MAX),
                             Not(by_term(9))])], BM25(), st)[0]
    assert (p.op, p.min_match, p.merge, p.terms, p.excluded) == (_lib.OP_MINMATCH, 2, search.MERGE_MAX, [1, 2, 3], [9])
    p = search.prepare([And([by_phrase([1, 2]), Not(by_term(3))])], BM25(), st)[0]
    assert p.op == _lib.OP_PHRASE and p.terms == [1, 2] and p.offsets == [0, 1] and p.excluded == [3]
    # Not(Not(f)) is f; the scorers are those of the query without its exclusions
    a = search.prepare([Not(Not(Or([by_term(1), by_term(2)])))], BM25(), st)[0]
    b = search.prepare([Or([by_term(1), by_term(2)])], BM25(), st)[0]
    assert a == b and a.excluded == []
    c = search.prepare([And([Or([by_term(1), by_term(2)]), Not(by_term(3))])], BM25(), st)[0]
    assert c.scorers == b.scorers and c.excluded == [3]
    arr = search.QueryArrays.from_prepared([type("S", (), {"metas": np.zeros(64)})()], [c], 10)
    assert arr.queries[0]["n_terms"] == 3
    assert list(arr.terms[0, :3]["kind"]) == [_lib.SCORE_BM25, _lib.SCORE_BM25, _lib.EXCLUDE]
    for bad, why in [(Or([by_term(1), Not(by_term(2))]), "Or with a Not"),
                     (Not(by_term(1)), "only Not"),
                     (And([Not(by_term(1)), Not(by_term(2))]), "only Not"),
                     (And([by_term(1), Not(by_phrase([1, 2]))]), "Not of by_phrase"),
                     (And([by_term(1), Not(And([by_term(2), by_term(3)]))]), "Not of And"),
                     (And([by_term(1), Or([by_term(2), by_term(3)]), Not(by_term(4))]), "ONE Or")]:
        with pytest.raises(ValueError, match=why):
            search.prepare([bad], BM25(), st)
    with pytest.raises(ValueError, match="Not"):
        search.prepare_filters([And([by_term(1), Not(by_term(2))])], BM25(), st, [], 10)


def _cpp(L, tmp_path, extra=()):
    """tests/cpp/test_exclusion.cpp: the C++ layer's Exclusion through prepare() and QueryBatch."""
    import subprocess
    from pathlib import Path
    from iresearch_amd import _build
    root = Path(__file__).resolve().parents[1]
    synth_lib = _build.build_synth()
    exe = tmp_path / "test_exclusion"
    lib = Path(L._name)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall",
           "-I", str(root / "include"), "-I", str(root / "iresearch_amd" / "cpp"),
           "-I", str(root / "iresearch_amd" / "index"),
           str(root / "tests" / "cpp" / "test_exclusion.cpp"), "-o", str(exe), str(lib), str(synth_lib),
           "-pthread", "-Wl,-rpath," + str(lib.parent), "-Wl,-rpath," + str(Path(synth_lib).parent), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "test_exclusion OK" in run.stdout, (run.stdout + run.stderr)[-3000:]


def test_cpp_exclusion_emulated(simlib, tmp_path):
    _cpp(simlib, tmp_path)


# --------------------------------------------------------------------- GPU --

@pytest.mark.gpu
def test_cpp_exclusion_gpu(gpulib, tmp_path):
    rocm = "/opt/rocm/lib"
    _cpp(gpulib, tmp_path, ["-Wl,-rpath," + rocm, "-Wl,-rpath-link," + rocm, "-Wl,--allow-shlib-undefined"])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_exclusion_gpu(gpulib, layout):
    case_exclusion(gpulib, 300_000, 512, layout, (BM25(), TFIDF(True), TFIDF(False)), (25, 1000))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_exclusion_lists_gpu(gpulib, layout):
    case_exclusion_lists(gpulib, layout)


@pytest.mark.gpu
def test_exclusion_multi_gpu(gpulib):
    case_exclusion_multi(gpulib, (70_000, 30_000, 140_000))


@pytest.mark.gpu
def test_exclusion_abi_gpu(gpulib):
    case_exclusion_abi(gpulib)
