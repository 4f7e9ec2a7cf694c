"""And filters whose children are Ors of by_term (IRS_HIP_GROUP_ALT, k_conj_any): And::prepare ->
make_conjunction over the children, an Or child being its own make_disjunction
(boolean_filter.cpp:150-210, boolean_query.cpp:60-145).

Expected values come from the oracle, composed without changing it: per group the oracle's Or over
its present members (score and match arrays), the match the AND of the groups', the score the And's
merge over the group scores.  One body runs on the emulator (CPU tier) and on the GPU at a larger
size."""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import pytest

import oracle
import parity
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, TFIDF, And, Not, Or, by_phrase, by_term


# ------------------------------------------------------------- expectations --

def _docs(seg, term):
    if not (0 <= term < len(seg.metas)) or int(seg.metas[term]["docs_count"]) == 0:
        return np.zeros(0, np.int64)
    d, _ = oracle.decode_term(seg.doc_file, seg.metas[term], seg.layout,
                              wand_count=int(getattr(seg, "wand_count", 0)))
    return d.astype(np.int64)


def _masked(seg, excluded):
    """seg with doc_mask = its deletions + every doc of the excluded terms."""
    if not excluded:
        return seg
    out = copy.copy(seg)
    m = getattr(seg, "doc_mask", None)
    parts = [np.zeros(0, np.int64) if m is None else np.asarray(m, np.int64)] + [_docs(seg, t) for t in excluded]
    out.doc_mask = np.unique(np.concatenate(parts)).astype(np.uint32)
    return out


def _groups(flt, mult=np.float32(1)):
    """The groups of an And tree, (term, boost product) per member — written out here, apart from
    search.and_groups (the code under test): an Or's by_term and SUM-Or members join its group, an
    And child's groups join the parent's; boosts multiply from the top in float32."""
    mult = np.float32(mult * np.float32(flt.boost))

    def members(o, m):
        out = []
        for s in o.subs:
            if type(s) is by_term:
                out.append((s.term, np.float32(m * np.float32(s.boost))))
            else:
                assert type(s) is Or
                out += members(s, np.float32(m * np.float32(s.boost)))
        return out

    out = []
    for s in flt.subs:
        if type(s) is by_term:
            out.append([(s.term, np.float32(mult * np.float32(s.boost)))])
        elif type(s) is Or:
            out.append(members(s, np.float32(mult * np.float32(s.boost))))
        else:
            assert type(s) is And
            out += _groups(s, mult)
    return out


def expected(seg, flt, scorer, all_segs=None, excluded=()):
    """(score f64[num_docs + 1], matched bool[num_docs + 1]) of a grouped And on one segment."""
    all_segs = all_segs or [seg]
    view = parity.oracle_view(_masked(seg, excluded))
    osc = parity.oracle_scorer(scorer)
    dwf = sum(s.docs_with_field for s in all_segs)
    ttf = sum(s.total_term_freq for s in all_segs)
    groups = _groups(flt)
    per = []
    match = None
    for g in groups:
        terms = [t for t, _ in g]
        boosts = [b for _, b in g]
        dwt = [sum(int(s.metas[t]["docs_count"]) if 0 <= t < len(s.metas) else 0 for s in all_segs)
               for t in terms]
        sc, m = oracle.score_all(view, parity.metas_for(seg, terms), oracle.OP_OR, osc, dwf, dwt, ttf, boosts)
        cost = sum(int(seg.metas[t]["docs_count"]) for t in terms if 0 <= t < len(seg.metas))
        per.append((cost, sc.astype(np.float64)))
        match = m.astype(bool) if match is None else match & m.astype(bool)
    per.sort(key=lambda x: x[0])   # (stable: Conjunction's cost order)
    score = per[0][1].copy()
    for _, sc in per[1:]:
        if flt.merge == search.MERGE_MAX:
            score = np.maximum(score, sc)
        elif flt.merge == search.MERGE_MIN:
            score = np.minimum(score, sc)
        else:
            score = score + sc
    return score, match


def check(seg, flt, scorer, k, h, c, t, all_segs=None, excluded=()):
    scores, matched = expected(seg, flt, scorer, all_segs, excluded)
    n_match = int(matched.sum())
    assert int(t) == n_match, ("total hits", flt, int(t), n_match)
    n = int(c)
    assert n == min(k, n_match), ("count", flt, n, k, n_match)
    if n == 0:
        return
    docs = h[:n]["doc"].astype(np.int64)
    assert len(set(docs.tolist())) == n, ("duplicate docs", flt)
    assert matched[docs].all(), ("unmatched doc returned", flt)
    ref = scores[docs]
    rel = np.abs(h[:n]["score"] - ref) / np.maximum(np.abs(ref), 1e-30)
    assert rel.max() <= parity.REL_TOL, ("score", flt, float(rel.max()))
    s, d = h[:n]["score"], h[:n]["doc"]
    assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (d[:-1] < d[1:]))).all(), ("order", flt)
    ms = np.sort(scores[matched])[::-1]
    thr = ms[n - 1]
    must = np.nonzero(matched & (scores > thr * (1 + 2 * parity.REL_TOL)))[0]
    assert np.isin(must, docs).all(), ("missing doc above the k-th score", flt)
    assert (ref >= thr * (1 - 2 * parity.REL_TOL)).all(), ("doc below the k-th score", flt)


# ------------------------------------------------------------------ shapes --

def _rare(seg, lo, hi):
    """A term with lo <= docs_count < hi (tail-only lists, single docs), or None."""
    dc = np.asarray(seg.metas["docs_count"])
    idx = np.nonzero((dc >= lo) & (dc < hi))[0]
    return int(idx[0]) if idx.size else None


def shape_filters(seg, max_rank, merge=search.MERGE_SUM):
    R, A = max_rank, 10 * max_rank
    fl = [
        And([by_term(R // 8), Or([by_term(1), by_term(2)])]),                        # lead group of one
        And([Or([by_term(3), by_term(R // 4)]), Or([by_term(0), by_term(5)])]),       # lead of two
        And([Or([by_term(R // 2 + i) for i in range(4)]), by_term(0)]),               # lead of four
        And([Or([by_term(0), by_term(1), by_term(2)]), Or([by_term(3), by_term(4)])]),  # heavy overlap
        And([Or([by_term(1), by_term(R // 3)]), Or([by_term(R // 3), by_term(9)])]),  # a term in two groups
        And([by_term(7), Or([by_term(3), by_term(3)])]),                              # a term twice in a group
        And([Or([by_term(2), by_term(A)]), Or([by_term(4), by_term(6)])]),            # an absent member
        And([by_term(1), Or([by_term(A), by_term(A + 1)])]),                          # a group without one
        And([Or([by_term(R - 1), by_term(R - 2)]), Or([by_term(0), by_term(1)])]),    # rare lead members
        And([Or([by_term(0), by_term(1)], boost=1.5), by_term(6, boost=0.5),
             Or([by_term(11), by_term(13), by_term(R // 5)])], boost=2.0),            # three groups, boosts
        And([Or([by_term(2), Or([by_term(8), by_term(12)])]), And([by_term(0), Or([by_term(5), by_term(6)])])]),
    ]
    tail = _rare(seg, 2, 128)
    one = _rare(seg, 1, 2)
    if tail is not None:
        fl.append(And([Or([by_term(tail), by_term(R - 3)]), Or([by_term(0), by_term(2), by_term(4)])]))
    if one is not None:
        fl.append(And([Or([by_term(one), by_term(tail if tail is not None else 3)]), by_term(0)]))
    for f in fl:
        f.merge = merge
        for s in f.subs:
            if isinstance(s, And):
                s.merge = merge
    return fl


def _run(sr, filters, scorer, k, stats, **kw):
    b = sr.batch(search.prepare(filters, scorer, stats), k)
    if kw.get("wand"):
        b.set_wand(True)
    h, c, t = (x.copy() for x in b.run().results())
    return b, h, c, t


def case_shapes(L, num_docs, max_rank, layout, scorers, ks, merges=(0, 1, 2)):
    seg = synth.build_segment(num_docs, max_rank, layout=layout)
    st = [parity.segment_stats(seg)]
    sr = search.SegmentReader.from_synth(seg, L=L)
    for merge in merges:
        fl = shape_filters(seg, max_rank, merge)
        assert all(any(search.prepare([f], BM25(), st)[0].alts or [False]) for f in fl)
        for scorer in scorers:
            for k in ks:
                b, h, c, t = _run(sr, fl, scorer, k, st)
                b.close()
                for q, f in enumerate(fl):
                    check(seg, f, scorer, k, h[q], c[q], t[q])
                assert int(t[7]) == 0
    sr.close()


def case_cross(L, num_docs, max_rank, layout):
    """Against today's kernels: a one-member group is the flat And bit for bit; +a +(b c) matches
    the union of +a +b and +a +c; flat units of a mixed batch are what they are alone."""
    seg = synth.build_segment(num_docs, max_rank, layout=layout)
    st = [parity.segment_stats(seg)]
    sr = search.SegmentReader.from_synth(seg, L=L)
    k = 1000
    pairs = [(3, 1, 2), (max_rank // 8, 0, 5), (max_rank - 2, 1, 3), (4, 4, 9)]
    for a, b_, c_ in pairs:
        bb, h1, c1, t1 = _run(sr, [And([by_term(a), Or([by_term(b_)])])], BM25(), k, st)
        bb.close()
        bb, h2, c2, t2 = _run(sr, [And([by_term(a), by_term(b_)])], BM25(), k, st)
        bb.close()
        assert np.array_equal(h1, h2) and np.array_equal(c1, c2) and np.array_equal(t1, t2)
        big = int(seg.num_docs)
        bb, hg, cg, tg = _run(sr, [And([by_term(a), Or([by_term(b_), by_term(c_)])])], BM25(), big if big <= _lib.MAX_K else _lib.MAX_K, st)
        bb.close()
        bb, hf, cf, tf = _run(sr, [And([by_term(a), by_term(b_)]), And([by_term(a), by_term(c_)])], BM25(), _lib.MAX_K, st)
        bb.close()
        union = set(hf[0, :int(cf[0])]["doc"].tolist()) | set(hf[1, :int(cf[1])]["doc"].tolist())
        want = set(_docs(seg, a).tolist()) & (set(_docs(seg, b_).tolist()) | set(_docs(seg, c_).tolist()))
        assert int(tg[0]) == len(want)
        if int(tf[0]) <= _lib.MAX_K and int(tf[1]) <= _lib.MAX_K:
            assert union == want == set(hg[0, :int(cg[0])]["doc"].tolist())
    # mixed batch: flat units bit-identical to the same units alone, on every path
    ranks = synth.make_queries(6, 8, 3, max_rank, synth.SEED + 3)
    flat = [Or([by_term(int(r) - 1) for r in row]) for row in ranks]
    flat += [And([by_term(0), by_term(3)]), And([by_term(max_rank // 4), by_term(1), by_term(2)]),
             Or([by_term(1), by_term(5), by_term(9)], min_match=2), by_term(17)]
    grouped = shape_filters(seg, max_rank)
    for path in (_lib.PATH_AUTO, _lib.PATH_ITEMS, _lib.PATH_JOINED):
        for scorer in (BM25(), TFIDF(True)):
            b = sr.batch(search.prepare(flat, scorer, st), 100).set_path(path)
            hp, cp, tp = (x.copy() for x in b.run().results())
            pth, pp = b.path(), b.paired_tiles()
            b.close()
            b = sr.batch(search.prepare(flat + grouped, scorer, st), 100).set_path(path)
            hm, cm, tm = b.run().results()
            assert (b.path(), b.paired_tiles()) == (pth, pp)
            n = len(flat)
            assert np.array_equal(hm[:n], hp) and np.array_equal(cm[:n], cp) and np.array_equal(tm[:n], tp)
            for q, f in enumerate(grouped):
                check(seg, f, scorer, 100, hm[n + q], cm[n + q], tm[n + q])
            b.close()
    sr.close()


def case_deletions(L, num_docs, max_rank, layout):
    """A segment with deleted docs, Not exclusions (And([And([groups]), Not(...)])), unit masks,
    wand on / off, min scores, a plan ahead, a forced re-run."""
    seg = synth.build_segment(num_docs, max_rank, layout=layout)
    rng = np.random.default_rng(31)
    seg.doc_mask = np.concatenate([rng.choice(num_docs, num_docs // 20, replace=False).astype(np.uint32) + 1,
                                   np.arange(100, 700, dtype=np.uint32)])
    st = [parity.segment_stats(seg)]
    sr = search.SegmentReader.from_synth(seg, L=L)
    grouped = shape_filters(seg, max_rank)
    excl = [[], [max_rank // 2], [0, 10 * max_rank], [6, 7]]
    filters, incl = [], []
    for i, f in enumerate(grouped):
        ex = excl[i % len(excl)]
        filters.append(And([f] + [Not(by_term(x)) for x in ex]) if ex else f)
        incl.append((f, ex))
    n_words = (num_docs + 64) // 64
    for k in (10, 1000):
        for scorer in (BM25(), TFIDF(False)):
            b, h, c, t = _run(sr, filters, scorer, k, st)
            for q, (f, ex) in enumerate(incl):
                check(seg, f, scorer, k, h[q], c[q], t[q], excluded=[x for x in ex if x < max_rank])
            for q, (f, ex) in enumerate(incl):
                present = [x for x in ex if 0 <= x < max_rank]
                dead = np.zeros(n_words, np.uint64)
                docs = np.unique(np.asarray(seg.doc_mask, np.int64))
                np.bitwise_or.at(dead, docs // 64, np.uint64(1) << (docs % 64).astype(np.uint64))
                want = dead | (sr.bit_union(present, n_words)[0] if present else 0)
                if int(t[q]):   # (a unit without rows has no mask of its own)
                    assert np.array_equal(b.unit_mask(q, n_words), want), q
            b.close()
            # wand: grouped units run exhaustively — the same top k and totals
            bw, hw, cw, tw = _run(sr, filters, scorer, k, st, wand=True)
            bw.close()
            assert np.array_equal(hw, h) and np.array_equal(cw, c) and np.array_equal(tw, t)
    # min scores, a plan queued ahead, a re-run of the same batch
    k = 100
    b = sr.batch(search.prepare(filters, BM25(), st), k)
    h1, c1, t1 = (x.copy() for x in b.run().results())
    b.plan()
    h2, c2, t2 = (x.copy() for x in b.run().results())
    assert np.array_equal(h1, h2) and np.array_equal(c1, c2) and np.array_equal(t1, t2)
    kth = np.array([h1[q, c1[q] - 1]["score"] if c1[q] else 0.0 for q in range(len(filters))], np.float32)
    h3, c3, _ = (x.copy() for x in b.set_min_scores(kth).run().results())
    assert np.array_equal(h1, h3) and np.array_equal(c1, c3)
    half = np.array([h1[q, c1[q] // 2]["score"] if c1[q] else 0.0 for q in range(len(filters))], np.float32)
    h4, c4, _ = b.set_min_scores(half).run().results()
    for q in range(len(filters)):
        n = int(c1[q])
        keep = h1[q, :n][h1[q, :n]["score"] >= half[q]] if n else h1[q, :0]
        assert int(c4[q]) == keep.size and np.array_equal(h4[q, :keep.size], keep), q
    b.close()
    # a forced re-run: a candidate buffer far too small
    b = sr.batch(search.prepare(filters, BM25(), st), 100)
    b.configure(cand_cap=100)
    h5, c5, t5 = (x.copy() for x in b.run().results())
    assert b.reruns() > 0
    for q, (f, ex) in enumerate(incl):
        check(seg, f, BM25(), 100, h5[q], c5[q], t5[q], excluded=[x for x in ex if x < max_rank])
    b.close()
    sr.close()


def case_multi(L, sizes, ranks, k=100):
    """create_multi over segments with different term tables (a member present in some only),
    per-segment parity with global statistics, merged on the host and with irs_hip_merge_topk."""
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    segs = [synth.build_segment(int(n), int(r), first_doc=int(f)) for n, r, f in zip(sizes, ranks, first)]
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    lo = min(ranks)
    filters = [And([Or([by_term(1), by_term(max(ranks) - 1)]), Or([by_term(0), by_term(lo + 2)])]),
               And([by_term(2), Or([by_term(3), by_term(lo - 1), by_term(max(ranks) - 2)])], merge=search.MERGE_MAX),
               And([Or([by_term(max(ranks) - 1), by_term(max(ranks) - 3)]), by_term(0)]),
               And([Or([by_term(4), by_term(5)]), Or([by_term(6), by_term(7)])], merge=search.MERGE_MIN)]
    stats = [parity.segment_stats(s) for s in segs]
    prep = search.prepare(filters, BM25(), stats)
    qb = search.QueryBatch(readers, prep, k)
    h, c, t = qb.run().results()
    for i, s in enumerate(segs):
        for q, f in enumerate(filters):
            check(s, f, BM25(), k, h[i, q], c[i, q], t[i, q], segs)
    shared = search.QueryBatch(readers, prep, k).set_shared_threshold(True)
    sh, sc, stt = shared.run().results()
    assert np.array_equal(t, stt)
    mp = search.merge_topk_host([(h[i], c[i]) for i in range(len(segs))], k)
    assert mp == search.merge_topk_host([(sh[i], sc[i]) for i in range(len(segs))], k)
    # the merged top k against the composed oracle over all segments
    for q, f in enumerate(filters):
        allsc = []
        for s in segs:
            sc_, m = expected(s, f, BM25(), segs)
            allsc += sc_[m].tolist()
        allsc = np.sort(np.asarray(allsc))[::-1][:k]
        got = np.array([r[0] for r in mp[q]])
        assert got.size == allsc.size and np.allclose(got, allsc, rtol=parity.REL_TOL, atol=0), q
    import torch
    from iresearch_amd import distributed
    arch = C.create_string_buffer(64)
    L.irs_hip_device_arch(0, arch, 64)
    dev = "cpu" if arch.value.endswith(b"-sim") else "cuda"
    lists, batches = [], []
    for i, r in enumerate(readers):
        b = r.batch(prep, k)
        b.run()
        hh = torch.zeros((len(filters), k), dtype=torch.int64, device=dev)
        cc = torch.zeros((len(filters),), dtype=torch.int32, device=dev)
        b.results_to_device(hh.data_ptr(), cc.data_ptr())
        if dev == "cuda":
            torch.cuda.synchronize()
        lists.append((i, hh, cc))
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
    for b in batches + [qb, shared]:
        b.close()
    for r in readers:
        r.close()


def case_abi(L):
    """IRS_HIP_GROUP_ALT where it does not belong: EINVAL; more than 16 included entries as for
    flat queries."""
    seg = synth.build_segment(5_000, 64)
    sr = search.SegmentReader.from_synth(seg, L=L)

    def create(op, kinds, terms=None):
        n = len(kinds)
        q = np.zeros(1, _lib.QUERY)
        q[0] = (op, n, 0, 10, 2 if op == _lib.OP_MINMATCH else 0, 0)
        t = np.zeros(max(n, 1), _lib.TERM_SCORER)
        for i, kd in enumerate(kinds):
            t[i] = ((terms[i] if terms else i + 1), kd, 1.0, 0.3, 0.01, 0)
        h = C.c_void_p()
        rc = L.irs_hip_batch_create(sr.handle, q.ctypes.data, 1, t.ctypes.data, n, C.byref(h))
        if rc == 0:
            L.irs_hip_batch_destroy(h)
        return rc

    G, B, X = _lib.GROUP_ALT, _lib.SCORE_BM25, _lib.EXCLUDE
    assert create(_lib.OP_AND, [B, B | G, B]) == 0
    assert create(_lib.OP_AND, [B, B | G, B, X]) == 0
    assert create(_lib.OP_AND, [B, B | G, B, B | G], [1, 1, 2, 2]) == 0   # repeats
    assert create(_lib.OP_AND, [B | G, B]) == _lib.EINVAL                  # on the first entry
    assert create(_lib.OP_AND, [B, B | G, X | G]) == _lib.EINVAL          # on an exclude entry
    assert create(_lib.OP_AND, [B, B | G, X, X | G]) == _lib.EINVAL
    assert create(_lib.OP_OR, [B, B | G]) == _lib.EINVAL
    assert create(_lib.OP_MINMATCH, [B, B | G, B]) == _lib.EINVAL
    many = [B] + [B | G] * 16
    assert create(_lib.OP_AND, many) == create(_lib.OP_AND, [B] * 17) == _lib.EINVAL
    assert create(_lib.OP_AND, [B] + [B | G] * 15) == 0
    sr.close()


# --------------------------------------------------------------- host layer --

def test_prepare_groups():
    st = [search.SegmentStats(1000, 100_000, np.arange(64, dtype=np.int64) + 10)]
    sc = BM25()
    # a one-term Or is a by_term; a tree without a group of two goes out as today's flat And
    flat = search.prepare([And([by_term(1), by_term(2), by_term(3)])], sc, st)[0]
    for f in (And([by_term(1), Or([by_term(2)]), by_term(3)]),
              And([And([by_term(1), Or([by_term(2)])]), by_term(3)]),
              And([Or([Or([by_term(1)])]), by_term(2), And([by_term(3)])])):
        p = search.prepare([f], sc, st)[0]
        assert p == flat and p.alts is None
        a = search.QueryArrays.from_prepared([type("S", (), {"metas": np.zeros(64)})()], [p], 10)
        b = search.QueryArrays.from_prepared([type("S", (), {"metas": np.zeros(64)})()], [flat], 10)
        assert a.queries.tobytes() == b.queries.tobytes() and a.terms.tobytes() == b.terms.tobytes()
    # flattening: same-merge And children, SUM Ors inside a group
    f = And([by_term(1), And([Or([by_term(2), by_term(3)]), by_term(4)]),
             Or([by_term(5), Or([by_term(6), by_term(7)])])])
    assert [[t for t, _ in g] for g in search.and_groups(f)] == [[1], [2, 3], [4], [5, 6, 7]]
    p = search.prepare([f], sc, st)[0]
    assert p.op == _lib.OP_AND and p.terms == [1, 2, 3, 4, 5, 6, 7]
    assert p.alts == [False, False, True, False, False, True, True]
    arr = search.QueryArrays.from_prepared([type("S", (), {"metas": np.zeros(64)})()], [p], 10)
    assert [int(x) & _lib.GROUP_ALT for x in arr.terms[0, :7]["kind"]] == [0, 0, _lib.GROUP_ALT, 0, 0,
                                                                           _lib.GROUP_ALT, _lib.GROUP_ALT]
    # boosts multiply down the tree (boolean_query_boost.hierarchy): leaf x Or x And
    f = And([Or([by_term(1, boost=3.0), by_term(2)], boost=2.0), by_term(4, boost=0.5)], boost=1.5)
    p = search.prepare([f], sc, st)[0]
    for (t, leaf, mults), got in zip([(1, 3.0, (1.5, 2.0)), (2, 1.0, (1.5, 2.0)), (4, 0.5, (1.5,))], p.scorers):
        boost = np.float32(1.0)
        for m in mults:
            boost = np.float32(boost * np.float32(m))
        boost = np.float32(boost * np.float32(leaf))
        want = sc.term_scorer(sc.collect(1000, int(st[0].docs_count[t]), 100_000), boost)
        assert got[1] == want[1], (t, got, want)
    # a flat Or / And boost multiplies too
    p = search.prepare([Or([by_term(1), by_term(2, boost=2.0)], boost=3.0)], sc, st)[0]
    q = search.prepare([Or([by_term(1, boost=3.0), by_term(2, boost=6.0)])], sc, st)[0]
    assert p.scorers == q.scorers
    # exclusions compose by nesting: groups plus IRS_HIP_EXCLUDE entries
    p = search.prepare([And([And([Or([by_term(2), by_term(3)]), by_term(1)]), Not(by_term(9))])], sc, st)[0]
    assert p.terms == [2, 3, 1] and p.alts == [False, True, False] and p.excluded == [9]
    # refused
    for bad, why in [(Or([by_term(1), And([by_term(2), by_term(3)])]), "only flat"),
                     (And([by_term(1), Or([by_term(2), And([by_term(3), by_term(4)])])]), "And children"),
                     (And([by_term(1), Or([by_term(2), by_term(3)], min_match=2)]), "min_match"),
                     (And([by_term(1), Or([by_term(2), by_term(3)], merge=search.MERGE_MAX)]), "SUM"),
                     (And([by_term(1), by_phrase([2, 3])]), "phrase"),
                     (And([by_term(1), And([by_term(2), Or([by_term(3), by_term(4)])], merge=search.MERGE_MAX)]),
                      "merge"),
                     (And([by_term(1), Or([by_term(i) for i in range(16)])]), "16"),
                     (And([by_term(1), Or([by_term(2), by_term(3)]), Not(by_term(4))]), "ONE Or")]:
        with pytest.raises(ValueError, match=why):
            search.prepare([bad], sc, st)


def _cpp(L, tmp_path, extra=()):
    """tests/cpp/test_nested_boolean.cpp: the C++ layer's And::groups through prepare() and QueryBatch."""
    import subprocess
    from pathlib import Path
    from iresearch_amd import _build
    root = Path(__file__).resolve().parents[1]
    synth_lib = _build.build_synth()
    exe = tmp_path / "test_nested_boolean"
    lib = Path(L._name)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall",
           "-I", str(root / "include"), "-I", str(root / "iresearch_amd" / "cpp"),
           "-I", str(root / "iresearch_amd" / "index"),
           str(root / "tests" / "cpp" / "test_nested_boolean.cpp"), "-o", str(exe), str(lib), str(synth_lib),
           "-pthread", "-Wl,-rpath," + str(lib.parent), "-Wl,-rpath," + str(Path(synth_lib).parent), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "test_nested_boolean OK" in run.stdout, (run.stdout + run.stderr)[-3000:]


# ------------------------------------------------------------------- CPU --

def test_cpp_nested_boolean_emulated(simlib, tmp_path):
    _cpp(simlib, tmp_path)


def test_nested_abi_emulated(simlib):
    case_abi(simlib)


def test_nested_shapes_emulated(simlib):
    case_shapes(simlib, 20_000, 96, synth.LAYOUT_SIMD4, (BM25(), TFIDF(True)), (1, 10, 1000))


def test_nested_shapes_emulated_scalar(simlib):
    case_shapes(simlib, 12_000, 64, synth.LAYOUT_SCALAR, (BM25(b=0.0), TFIDF(False)), (100,), merges=(0, 2))


def test_nested_cross_emulated(simlib):
    case_cross(simlib, 15_000, 64, synth.LAYOUT_SIMD4)


def test_nested_deletions_emulated(simlib):
    case_deletions(simlib, 15_000, 64, synth.LAYOUT_SIMD4)


def test_nested_multi_emulated(simlib):
    case_multi(simlib, (9_000, 4_000, 14_000), (96, 64, 80), k=50)


# --------------------------------------------------------------------- GPU --

@pytest.mark.gpu
def test_cpp_nested_boolean_gpu(gpulib, tmp_path):
    rocm = "/opt/rocm/lib"
    _cpp(gpulib, tmp_path, ["-Wl,-rpath," + rocm, "-Wl,-rpath-link," + rocm, "-Wl,--allow-shlib-undefined"])


@pytest.mark.gpu
def test_nested_abi_gpu(gpulib):
    case_abi(gpulib)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_nested_shapes_gpu(gpulib, layout):
    case_shapes(gpulib, 2_000_000, 2048, layout, (BM25(), BM25(b=0.0), TFIDF(True), TFIDF(False)),
                (1, 10, 100, 1000))


@pytest.mark.gpu
def test_nested_cross_gpu(gpulib):
    case_cross(gpulib, 2_000_000, 1024, synth.LAYOUT_SIMD4)


@pytest.mark.gpu
def test_nested_deletions_gpu(gpulib):
    case_deletions(gpulib, 2_000_000, 1024, synth.LAYOUT_SIMD4)


@pytest.mark.gpu
def test_nested_multi_gpu(gpulib):
    case_multi(gpulib, (700_000, 300_000, 1_000_000), (512, 256, 384), k=1000)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_nested_at_size_gpu(gpulib, layout):
    """1000 grouped queries (two groups of two, the shape of sweep.py --op and --terms 2 --alts 2)
    at 10 M docs, k = 1000, checked against the oracle on 32 of them."""
    num_docs, max_rank = 10_000_000, 4096
    seg = synth.build_segment(num_docs, max_rank, layout=layout)
    st = [parity.segment_stats(seg)]
    sr = search.SegmentReader.from_synth(seg, L=gpulib)
    rng = np.random.default_rng(99)
    filters = []
    for _ in range(1000):
        a, b_ = (int(x) for x in rng.integers(0, max_rank // 4, 2))
        filters.append(And([Or([by_term(a), by_term(min(a + 1 + int(rng.integers(0, 8)), max_rank - 1))]),
                            Or([by_term(b_), by_term(min(b_ + 1 + int(rng.integers(0, 8)), max_rank - 1))])]))
    b, h, c, t = _run(sr, filters, BM25(), 1000, st)
    b.close()
    for q in range(0, 1000, 31):
        check(seg, filters[q], BM25(), 1000, h[q], c[q], t[q])
    sr.close()
