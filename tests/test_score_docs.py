"""irs_hip_batch_score_docs / _to_device: doc_iterator::seek(target) + score for docs the caller
names (formats_10.cpp:2304-2365, conjunction.hpp:207-223), on k_score_docs (csrc/score_docs.h).

Expectations come from the oracle as it stands, for ALL docs of a segment: flat units from
oracle.score_all (the way test_match_sets.want_set calls it, with the unit's merge in
parity.oracle_op), grouped units from test_nested_boolean.expected, clause units from
test_or_clauses.expected, trees from test_boolean_trees.expected, exclusions as extra mask docs
(test_nested_boolean._masked).  A call's `matched` must equal the oracle's bit for bit, every matched
score lie within 1e-5 relative of the oracle's (parity.REL_TOL, the project's bound), every
unmatched score be exactly 0.  One body per case, on the emulator (CPU tier) and on the GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle
import parity
import test_boolean_trees as bt
import test_nested_boolean as nb
import test_or_clauses as oc
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, TFIDF, And, Not, Or, by_doc_set, by_phrase, by_term, by_terms

MAX_K = _lib.MAX_K
CHUNK = 128          # kScoreDocsChunk: docs one wavefront takes
FLAGS = {"flat": {}, "grouped": {}, "clause": {"and_clauses": True}, "tree": {"boolean_trees": True}}


# ------------------------------------------------------------- expectations --

def X(inner, ex=()):
    """(filter with Not(by_term(x)) for x in ex, inner filter, ex)."""
    return (And([inner] + [Not(by_term(x)) for x in ex]) if ex else inner, inner, list(ex))


def want_flat(seg, inner, ex, scorer, all_segs=None):
    """(score f64[n1], matched bool[n1]) of a flat Or / And / min-match minus the excluded terms."""
    all_segs = all_segs or [seg]
    present = [x for x in ex if 0 <= x < len(seg.metas)]
    view = parity.oracle_view(nb._masked(seg, present))
    op, subs = search._terms_of(inner)
    terms = [s.term for s in subs]
    dwf = sum(s.docs_with_field for s in all_segs)
    ttf = sum(s.total_term_freq for s in all_segs)
    dwt = [sum(int(s.metas[t]["docs_count"]) if 0 <= t < len(s.metas) else 0 for s in all_segs) for t in terms]
    sc, m = oracle.score_all(view, parity.metas_for(seg, terms), parity.oracle_op(inner, op),
                             parity.oracle_scorer(scorer), dwf, dwt, ttf, [s.boost for s in subs])
    n1 = seg.num_docs + 1
    m = m[:n1].astype(bool)
    return np.where(m, sc[:n1], 0).astype(np.float64), m


def want(family, seg, triple, scorer, all_segs=None):
    flt, inner, ex = triple
    n1 = seg.num_docs + 1
    if family == "flat":
        return want_flat(seg, inner, ex, scorer, all_segs)
    if family == "grouped":
        present = [x for x in ex if 0 <= x < len(seg.metas)]
        sc, m = nb.expected(seg, inner, scorer, all_segs, excluded=present)
        m = m[:n1].astype(bool)
        return np.where(m, sc[:n1], 0.0), m
    assert not ex
    sc, m = (oc.expected if family == "clause" else bt.expected)(seg, flt, scorer, all_segs)
    return np.asarray(sc, np.float64)[:n1], np.asarray(m, bool)[:n1]


def check_list(tag, docs, scores, matched, exp, tol=parity.REL_TOL):
    """One unit's answers for `docs` against (score, matched) of all docs."""
    docs = np.asarray(docs, np.int64)
    assert scores.shape == matched.shape == docs.shape, tag
    wm, ws = exp[1][docs], exp[0][docs]
    assert np.array_equal(matched, wm), (tag, "matched", docs[matched != wm][:8])
    assert (scores[~wm] == 0).all(), (tag, "an unmatched score is not 0")
    if wm.any():
        rel = np.abs(scores[wm] - ws[wm]) / np.maximum(np.abs(ws[wm]), 1e-30)
        assert rel.max() <= tol, (tag, "score", float(rel.max()), docs[wm][np.argmax(rel)])


def batch_of(sr, family, triples, scorer, stats, k=100, doc_sets=None):
    prep = search.prepare([t[0] for t in triples], scorer, stats, **FLAGS[family])
    if isinstance(sr, list):
        return search.QueryBatch(sr, prep, k)
    return sr.batch(prep, k, doc_sets=doc_sets)


def score_all_units(b, docs):
    """The same list for every unit of the batch."""
    return b.score_docs([docs] * b.nq)


def device_of(L):
    arch = C.create_string_buffer(64)
    L.irs_hip_device_arch(0, arch, 64)
    return "cpu" if arch.value.endswith(b"-sim") else "cuda"


# -------------------------------------------------------------------- cases --

def case_abi(L):
    seg = synth.build_segment(6_000, 48, with_positions=True)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    T = lambda *ts: [by_term(t) for t in ts]
    triples = [X(Or(T(0, 1))), X(And(T(0, 2))), X(Or(T(1, 2, 3), min_match=2), [4])]
    b = batch_of(sr, "flat", triples, BM25(), st)
    nq, N = b.nq, seg.num_docs
    u32, u64 = (lambda *v: np.array(v, np.uint32)), (lambda *v: np.array(v, np.uint64))
    sc, mt = np.zeros(8, np.float32), np.zeros(8, np.uint8)

    def call(docs, offs, scores=sc, matched=mt, handle=b.handle):
        return L.irs_hip_batch_score_docs(handle, None if docs is None else docs.ctypes.data,
                                          None if offs is None else offs.ctypes.data,
                                          None if scores is None else scores.ctypes.data,
                                          None if matched is None else matched.ctypes.data)
    good_d, good_o = u32(1, 5, 9, 2, 3), u64(0, 3, 3, 5)
    # a call before any run; matched == NULL; an empty list in the middle
    assert call(good_d, good_o) == _lib.OK
    first = (sc[:5].copy(), mt[:5].copy())
    sc[:] = -1
    assert call(good_d, good_o, matched=None) == _lib.OK and np.array_equal(sc[:5], first[0])
    assert call(u32(0), u64(0, 0, 0, 0)) == _lib.OK             # every list empty
    # IRS_HIP_EINVAL: null batch, docs, offsets, scores; offsets[0] != 0; decreasing offsets
    assert call(good_d, good_o, handle=None) == _lib.EINVAL
    assert call(None, good_o) == _lib.EINVAL
    assert call(good_d, None) == _lib.EINVAL
    assert call(good_d, good_o, scores=None) == _lib.EINVAL
    assert call(good_d, u64(1, 3, 3, 5)) == _lib.EINVAL
    assert call(good_d, u64(0, 3, 2, 5)) == _lib.EINVAL
    # host variant only: a doc of 0, a doc above num_docs, a list not strictly ascending
    assert call(u32(0, 5, 9, 2, 3), good_o) == _lib.EINVAL
    assert call(u32(1, 5, N + 1, 2, 3), good_o) == _lib.EINVAL
    assert call(u32(1, 5, N, 2, 3), good_o) == _lib.OK
    assert call(u32(1, 5, 5, 2, 3), good_o) == _lib.EINVAL
    assert call(u32(1, 9, 5, 2, 3), good_o) == _lib.EINVAL
    assert call(u32(1, 5, 9, 3, 2), good_o) == _lib.EINVAL
    # more than 2^31 docs in all (no doc is read)
    assert call(good_d, u64(0, 3, 3, (1 << 31) + 1)) == _lib.EUNSUPPORTED
    assert L.irs_hip_batch_score_docs_to_device(b.handle, good_d.ctypes.data, good_o.ctypes.data, (1 << 31) + 1,
                                                sc.ctypes.data, None, None) == _lib.EUNSUPPORTED
    for args in ((None, good_o.ctypes.data, 5, sc.ctypes.data), (good_d.ctypes.data, None, 5, sc.ctypes.data),
                 (good_d.ctypes.data, good_o.ctypes.data, 5, None)):
        assert L.irs_hip_batch_score_docs_to_device(b.handle, args[0], args[1], args[2], args[3], None, None) == _lib.EINVAL
    assert L.irs_hip_batch_score_docs_to_device(None, good_d.ctypes.data, good_o.ctypes.data, 5, sc.ctypes.data,
                                                None, None) == _lib.EINVAL
    # a run, then score_docs, then a second run: the hits and the re-runs of a batch left alone
    plain = batch_of(sr, "flat", triples, BM25(), st)
    p1 = tuple(x.copy() for x in plain.run().results())
    p2 = tuple(x.copy() for x in plain.run().results())
    plain_reruns = plain.reruns()
    plain.close()
    g1 = tuple(x.copy() for x in b.run().results())
    lists = [np.arange(1, N + 1, 7, dtype=np.uint32)] * nq
    s1, m1 = b.score_docs(lists)
    g2 = tuple(x.copy() for x in b.run().results())
    s2, m2 = b.score_docs(lists)
    assert b.reruns() == plain_reruns
    for x, y in zip(p1 + p2, g1 + g2):
        assert np.array_equal(x, y), "scored results changed by score_docs"
    for q in range(nq):
        assert np.array_equal(s1[q], s2[q]) and np.array_equal(m1[q], m2[q])
        check_list(("abi", q), lists[q], s1[q], m1[q], want("flat", seg, triples[q], BM25()))
    assert np.array_equal(first[1][:3].astype(bool), want("flat", seg, triples[0], BM25())[1][[1, 5, 9]])
    b.close()
    # refused, and afterwards still running: a phrase batch, a phrase with optional terms, by_terms
    for flt, flags in ((by_phrase([0, 1]), {}), (Or([by_phrase([0, 1]), by_term(2)]), {"optional_terms": True}),
                       (by_terms([(0, 1.0), (1, 1.0), (2, 0.5)]), {})):
        rb = sr.batch(search.prepare([flt], BM25(), st, **flags), 10)
        before = tuple(x.copy() for x in rb.run().results())
        with pytest.raises(_lib.IrsHipError) as e:
            rb.score_docs([np.array([1, 2, 3], np.uint32)])
        assert e.value.status == _lib.EUNSUPPORTED, flt
        after = tuple(x.copy() for x in rb.run().results())
        for x, y in zip(before, after):
            assert np.array_equal(x, y)
        rb.close()
    sr.close()


def doc_lists(N, lists):
    """name -> docs: the smallest shapes at which the walk can go wrong."""
    rng = np.random.default_rng(11)
    pick = lambda n: np.sort(rng.choice(N, n, replace=False).astype(np.uint32) + 1)
    out = {"n%d" % n: pick(n) for n in (1, 127, 128, 129, 257)}
    out["consecutive"] = np.arange(1, 301, dtype=np.uint32)           # bucket shift 0, three chunks
    out["spread"] = np.arange(3, N + 1, 97, dtype=np.uint32)          # shift > 0: several lead docs per bucket
    out["dense_far"] = np.unique(np.concatenate([np.arange(1, 60, dtype=np.uint32), np.arange(N - 60, N + 1, dtype=np.uint32)]))
    out["border"] = np.array(sorted(set(oc.BORDER) | {oc.ALL, 1, N}), np.uint32)
    # in front of a term's first posting and behind its last (T128: 100 .. 24040; TTAIL: 7 .. 19207)
    out["outside"] = np.array([1, 2, 6, 99, 24041, 24042, N - 1, N], np.uint32)
    # the short lists' own docs (the 128th posting ends a block, the 129th is a vint tail of one,
    # TTAIL is tail only, TONE a single doc) and their neighbours
    edge = np.concatenate([lists[t][0].astype(np.int64) for t in (oc.T128, oc.T129, oc.TTAIL, oc.TONE)])
    edge = np.unique(np.concatenate([edge - 1, edge, edge + 1]))
    out["short_lists"] = edge[(edge >= 1) & (edge <= N)].astype(np.uint32)
    # block borders of a long list: postings 127 / 128 / 129, 255 / 256 / 257 of term 0
    d0 = lists[0][0]
    out["block_borders"] = np.unique(np.concatenate([d0[120:136], d0[250:262], d0[-130:]])).astype(np.uint32)
    return out


def flat_shapes():
    T, A, E = oc.T, oc.ABSENT, oc.TEMPTY
    S = search
    return [
        X(T(3)), X(Or([T(0), T(1, 2.0)])), X(Or([T(t) for t in range(16)])), X(And([T(0), T(2)])),
        X(And([T(1), T(3), T(5, 0.5), T(7)])), X(And([T(t) for t in range(0, 10, 2)])),
        X(Or([T(0), T(1), T(2)], min_match=2)), X(Or([T(t) for t in range(8)], min_match=7)),
        X(Or([T(oc.T128), T(oc.T129), T(oc.TTAIL), T(oc.TONE)])), X(And([T(oc.T129), T(1)])),
        X(And([T(oc.TTAIL), T(2)])), X(And([T(oc.TONE), T(0)])), X(Or([T(oc.T128), T(0)], min_match=2)),
        X(Or([T(oc.TBIG), T(4)])),
        # absent members under And, Or, Not; min-match above the present children
        X(And([T(0), T(A)])), X(And([T(0), T(E)])), X(Or([T(1), T(A), T(E)])), X(T(A)),
        X(And([T(0), T(2)]), [A, E]), X(Or([T(0), T(A), T(E)], min_match=2)), X(Or([T(0), T(1), T(A)], min_match=2)),
        # Not terms on every op
        X(T(1), [2]), X(Or([T(4), T(5), T(6)]), [0, oc.T129]), X(And([T(0), T(1)]), [2, A]),
        X(Or([T(0), T(1), T(2), T(3)], min_match=2), [4]), X(And([T(0), T(2)]), [0]),
        # zero boosts
        X(Or([T(0, 0.0), T(1, 0.0)])), X(And([T(0, 0.0), T(2)])), X(Or([T(0, 0.0), T(1), T(2, 0.0)], min_match=2)),
        # MAX and MIN on an Or of two and of three and on an And
        X(Or([T(0), T(2, 2.0)], merge=S.MERGE_MAX)), X(Or([T(0), T(2, 2.0)], merge=S.MERGE_MIN)),
        X(Or([T(0), T(1), T(2, 0.5)], merge=S.MERGE_MAX)), X(Or([T(0), T(1), T(2)], merge=S.MERGE_MIN)),
        X(And([T(0), T(2, 2.0), T(4)], merge=S.MERGE_MAX)), X(And([T(0), T(2, 0.5), T(4)], merge=S.MERGE_MIN)),
        X(Or([T(0), T(1), T(2)], min_match=2, merge=S.MERGE_MAX)), X(Or([T(0), T(A)], merge=S.MERGE_MIN)),
        # a term twice
        X(Or([T(5), T(5)])), X(And([T(5), T(5), T(6)])),
    ]


def grouped_shapes():
    T, A, E = oc.T, oc.ABSENT, oc.TEMPTY
    S = search
    return [
        X(And([T(6), Or([T(1), T(2)])])), X(And([Or([T(3), T(7)]), Or([T(0), T(5)])])),
        X(And([Or([T(oc.T128), T(oc.TTAIL), T(oc.TONE)]), Or([T(0), T(1), T(2)])])),
        X(And([Or([T(0), T(1)], boost=1.5), T(6, 0.5), Or([T(11), T(oc.T129), T(4)])], boost=2.0)),
        X(And([Or([T(2), T(A)]), Or([T(4), T(6)])])), X(And([T(1), Or([T(A), T(E)])])),
        X(And([T(0), Or([T(2), T(4)])]), [6, A]), X(And([Or([T(1), T(3)]), Or([T(0), T(2)])]), [oc.T129]),
        X(And([Or([T(0), T(2, 2.0)]), Or([T(1), T(3)])], merge=S.MERGE_MAX)),
        X(And([Or([T(0), T(2)]), Or([T(1), T(3, 0.5)]), T(4)], merge=S.MERGE_MIN)),
        X(And([Or([T(0, 0.0), T(2, 0.0)]), T(1, 0.0)])),
    ]


def case_lists(L, layout):
    lists = oc.hand_lists()
    N = oc.N_HAND
    norms = (np.arange(N, dtype=np.uint32) * 7 % 200 + 20).astype(np.uint8)
    ask = doc_lists(N, lists)
    assert [len(ask["n%d" % n]) for n in (1, 127, 128, 129, 257)] == [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
    gone = np.array(sorted({7, oc.TILE, oc.ALL, N, 100, 50, int(ask["n129"][128])}), np.uint32)
    families = {"flat": flat_shapes(), "grouped": grouped_shapes(),
                "clause": [X(f) for f in oc.hand_queries().values()],
                "tree": [X(f) for f in bt.hand_queries().values()]}
    for deleted in (False, True):
        seg = synth.segment_from_lists(lists, N, layout, norms=norms)
        seg.metas[oc.TEMPTY]["docs_count"] = 0       # an ordinal whose range is empty here
        if deleted:
            seg.doc_mask = gone
        sr = search.SegmentReader.from_synth(seg, L=L)
        st = [parity.segment_stats(seg)]
        for scorer in ((BM25(), TFIDF(True)) if not deleted else (BM25(),)):
            for family, triples in families.items():
                exp = [want(family, seg, t, scorer) for t in triples]
                if deleted:
                    assert not any(m[gone.astype(np.int64)].any() for _, m in exp)
                b = batch_of(sr, family, triples, scorer, st)
                for name, docs in ask.items():
                    if deleted and name not in ("border", "spread", "n129", "short_lists"):
                        continue
                    sc, mt = score_all_units(b, docs)
                    for q, t in enumerate(triples):
                        check_list((family, name, q, t[0]), docs, sc[q], mt[q], exp[q])
                # a different list per unit in one call, empty ones among them
                names = list(ask)
                per = [ask[names[q % len(names)]] if q % 5 else np.zeros(0, np.uint32) for q in range(len(triples))]
                sc, mt = b.score_docs(per)
                for q, t in enumerate(triples):
                    check_list((family, "mixed", q), per[q], sc[q], mt[q], exp[q])
                b.close()
            # what the lists say: the hits are hits, the zero boosts score 0
            if not deleted:
                e = want("flat", seg, X(Or([oc.T(0, 0.0), oc.T(1, 0.0)])), scorer)
                assert e[1].sum() > 100 and (e[0] == 0).all()
                e = want("flat", seg, X(Or([oc.T(0), oc.T(1), oc.T(oc.ABSENT)], min_match=2)), scorer)
                assert e[1][oc.ALL] and 0 < e[1].sum() < N
                e = want("flat", seg, X(Or([oc.T(0), oc.T(oc.ABSENT), oc.T(oc.TEMPTY)], min_match=2)), scorer)
                assert not e[1].any()
                e = want("flat", seg, X(Or([oc.T(0), oc.T(1), oc.T(2)], merge=search.MERGE_MIN)), scorer)
                assert e[1].sum() > 100 and (e[0] == 0).all()
        # a unit restricted by by_doc_set: the same answers inside the set, nothing outside
        if not deleted:
            words = N // 64 + 1
            inset = np.zeros(64 * words, bool)
            inset[np.arange(2, N + 1, 3)] = True
            inset[list(oc.BORDER)] = True
            sets = np.packbits(inset, bitorder="little").view(np.uint64).reshape(1, words)
            inner = [Or([oc.T(0), oc.T(1)]), And([oc.T(0), oc.T(2)]), Or([oc.T(0), oc.T(1), oc.T(2)], min_match=2),
                     And([Or([oc.T(1), oc.T(3)]), Or([oc.T(0), oc.T(2)])])]
            filters = [And([f, by_doc_set(0)]) for f in inner]
            b = sr.batch(search.prepare(filters, BM25(), st), 100, doc_sets=sets)
            for name in ("spread", "border", "consecutive", "n257"):
                sc, mt = score_all_units(b, ask[name])
                for q, f in enumerate(inner):
                    s0, m0 = want("grouped" if q == 3 else "flat", seg, X(f), BM25())
                    m1 = m0 & inset[:N + 1]
                    check_list(("doc set", name, q), ask[name], sc[q], mt[q], (np.where(m1, s0, 0.0), m1))
            b.close()
        sr.close()


def random_flat(n, seed, frequent=12):
    rng = np.random.default_rng(seed)
    pick = [0.25, 0.5, 1.0, 1.0, 2.0, 4.0]
    out = []
    for i in range(n):
        m = int(rng.integers(2, 9))
        terms = [by_term(int(t), float(rng.choice(pick))) for t in rng.choice(frequent if i % 4 else 60, m, replace=False)]
        merge = int(rng.choice([0, 0, 1, 2]))
        kind = i % 3
        if kind == 0:
            flt = Or(terms, merge=merge)
        elif kind == 1:
            flt = And(terms[:int(rng.integers(2, 4))], merge=merge)
        else:
            flt = Or(terms, min_match=int(rng.integers(2, m)) if m > 2 else 2, merge=merge if merge != 2 else 0)
        out.append(X(flt, [int(rng.integers(20, 50))] if i % 5 == 0 else []))
    return out


def random_grouped(n, seed, frequent=12):
    rng = np.random.default_rng(seed)
    pick = [0.25, 0.5, 1.0, 1.0, 2.0, 4.0]
    out = []
    for i in range(n):
        groups = []
        for _ in range(int(rng.integers(2, 4))):
            g = [by_term(int(t), float(rng.choice(pick))) for t in rng.choice(frequent if rng.random() < 0.7 else 60, int(rng.integers(1, 4)), replace=False)]
            groups.append(g[0] if len(g) == 1 else Or(g, boost=float(rng.choice(pick))))
        if all(type(g) is by_term for g in groups):
            groups[0] = Or([groups[0], by_term(int(rng.integers(frequent)))])
        out.append(X(And(groups, merge=int(rng.choice([0, 0, 1, 2]))), [int(rng.integers(20, 50))] if i % 4 == 0 else []))
    return out


def case_parity(L, num_docs, max_rank, layout, n_queries=24, seed=5):
    seg = synth.build_segment(num_docs, max_rank, layout=layout)
    seg.doc_mask = np.arange(9, num_docs, 101, dtype=np.uint32)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    rng = np.random.default_rng(seed)
    families = {"flat": random_flat(n_queries, seed), "grouped": random_grouped(n_queries, seed),
                "clause": [X(f) for f in oc.random_filters(n_queries, seed)],
                "tree": [X(f) for f in bt.random_trees(n_queries, seed)]}
    small = 0
    for family, triples in families.items():
        scorer = BM25() if family != "clause" else TFIDF(True)
        exp = [want(family, seg, t, scorer) for t in triples]
        b = batch_of(sr, family, triples, scorer, st, k=MAX_K)
        h, c, t = (x.copy() for x in b.run().results())
        # a random list per unit
        per = [np.sort(rng.choice(num_docs, int(rng.integers(1, 700)), replace=False).astype(np.uint32) + 1)
               for _ in triples]
        sc, mt = b.score_docs(per)
        for q in range(len(triples)):
            check_list((family, "random", q, triples[q][0]), per[q], sc[q], mt[q], exp[q])
        # the run's own hits, sorted by doc: all matched, the run's scores
        own = []
        for q in range(len(triples)):
            order = np.argsort(h[q, :int(c[q])]["doc"], kind="stable")
            own.append(h[q, :int(c[q])][order])
        sc, mt = b.score_docs([o["doc"].astype(np.uint32) for o in own])
        for q, o in enumerate(own):
            assert mt[q].all(), (family, "a hit of the run does not match", q)
            rel = np.abs(sc[q] - o["score"]) / np.maximum(np.abs(o["score"]), 1e-30)
            assert o.size == 0 or rel.max() <= 2 * parity.REL_TOL, (family, "run", q, float(rel.max()))
            check_list((family, "own", q), o["doc"], sc[q], mt[q], exp[q])
        # where the run returned every hit: a sample of the complement matches nothing
        comp = []
        for q, o in enumerate(own):
            rest = np.setdiff1d(np.arange(1, num_docs + 1, dtype=np.uint32), o["doc"].astype(np.uint32))
            comp.append(rest[::max(1, rest.size // 500)] if int(t[q]) <= MAX_K else np.zeros(0, np.uint32))
            small += int(t[q]) <= MAX_K
        sc, mt = b.score_docs(comp)
        for q in range(len(triples)):
            assert not mt[q].any() and (sc[q] == 0).all(), (family, "complement", q)
        b.close()
    assert small > 0, "no unit returned every hit: the complement check never ran"
    sr.close()


def case_multi(L, sizes, ranks):
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    segs = [synth.build_segment(int(n), int(r), first_doc=int(f)) for n, r, f in zip(sizes, ranks, first)]
    segs[1].doc_mask = np.arange(10, 400, dtype=np.uint32)
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    stats = [parity.segment_stats(s) for s in segs]
    lo, hi = min(ranks), max(ranks)
    T = lambda *ts: [by_term(t) for t in ts]
    families = {
        "flat": [X(by_term(hi - 1)), X(Or(T(1, hi - 1))), X(And(T(0, lo + 2))), X(And(T(0, 1)), [lo + 1]),
                 X(Or(T(0, lo - 1, hi - 2), min_match=2)), X(Or(T(2, 3, 4), merge=search.MERGE_MAX), [hi - 3])],
        "grouped": [X(And([Or(T(1, hi - 1)), Or(T(0, lo + 2))])), X(And([by_term(0), Or(T(lo + 1, hi - 1))]))],
        "clause": [X(Or([And(T(0, 1)), by_term(hi - 1), And(T(2, lo + 2))]))],
        "tree": [X(And([by_term(0), Or([by_term(lo + 1), And(T(1, 2))])])), X(Or([And([by_term(0), Not(by_term(hi - 2))]), by_term(3)]))],
    }
    rng = np.random.default_rng(3)
    for family, triples in families.items():
        b = batch_of(readers, family, triples, BM25(), stats)
        nq = len(triples)
        assert b.nq == nq * len(segs)
        per = [np.sort(rng.choice(int(sizes[u // nq]), 150 + 37 * (u % 3), replace=False).astype(np.uint32) + 1)
               for u in range(b.nq)]
        per[nq + 1] = np.arange(1, int(sizes[1]) + 1, 9, dtype=np.uint32)    # through the deleted run, to the last doc
        sc, mt = b.score_docs(per)
        for i, s in enumerate(segs):
            for q, t in enumerate(triples):
                u = i * nq + q
                check_list((family, "multi", i, q), per[u], sc[u], mt[u], want(family, s, t, BM25(), segs))
        b.close()
    # a term absent from the smallest rank table: an And with it matches nothing there
    e = want("flat", segs[int(np.argmin(ranks))], X(And(T(0, lo + 2))), BM25(), segs)
    assert not e[1].any()
    for r in readers:
        r.close()


def case_device(L, num_docs, max_rank):
    import torch
    dev = device_of(L)
    seg = synth.build_segment(num_docs, max_rank)
    seg.doc_mask = np.arange(50, 90, dtype=np.uint32)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    T = lambda *ts: [by_term(t) for t in ts]
    triples = [X(Or(T(0, 1, 2))), X(And(T(0, 2))), X(Or(T(0, 1, 2, 3), min_match=2), [4]), X(by_term(max_rank * 10)),
               X(Or(T(0, 1), merge=search.MERGE_MIN)), X(And(T(1, 3), merge=search.MERGE_MAX))]
    b = batch_of(sr, "flat", triples, BM25(), st)
    rng = np.random.default_rng(9)
    per = [np.sort(rng.choice(num_docs, n, replace=False).astype(np.uint32) + 1) for n in (300, 1, 129, 500, 0, 128)]
    flat = np.concatenate(per)
    offs = np.concatenate([[0], np.cumsum([p.size for p in per])]).astype(np.uint64)
    hs, hm = b.score_docs(flat, offs)
    for q in range(b.nq):
        lo, hi = int(offs[q]), int(offs[q + 1])
        check_list(("device", q), per[q], hs[lo:hi], hm[lo:hi], want("flat", seg, triples[q], BM25()))

    def dev_call(docs, stream=None):
        d_docs = torch.from_numpy(docs.view(np.int32)).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_sc = torch.full((docs.size,), -1.0, dtype=torch.float32, device=dev)
        d_mt = torch.full((docs.size,), 7, dtype=torch.uint8, device=dev)
        if dev == "cuda":
            torch.cuda.synchronize()
        b.score_docs_to_device(d_docs.data_ptr(), d_offs.data_ptr(), docs.size, d_sc.data_ptr(), d_mt.data_ptr(), stream)
        if dev == "cuda":
            torch.cuda.synchronize()
        return d_sc.cpu().numpy(), d_mt.cpu().numpy()
    if dev == "cuda":     # on a caller's stream
        s = torch.cuda.Stream()
        ds, dm = dev_call(flat, s.cuda_stream)
    else:
        ds, dm = dev_call(flat)
    assert np.array_equal(ds, hs) and np.array_equal(dm.astype(bool), hm)
    b.run()     # (a run queued behind a device-form call, and a call behind the run)
    ds, dm = dev_call(flat)
    assert np.array_equal(ds, hs) and np.array_equal(dm.astype(bool), hm)
    # what the host form refuses comes back unmatched: a doc of 0 and docs above num_docs (their chunk's
    # other docs keep their answers), a chunk out of order (all of it; its neighbours keep theirs)
    bad = flat.copy()
    bad[0] = 0                                    # unit 0, chunk 0, still ascending
    bad[298:300] = [num_docs + 1, 0xFFFFFFF0]     # the last docs of unit 0's last chunk, still ascending
    ds, dm = dev_call(bad)
    exp = hs.copy(), hm.copy()
    for e in exp:
        e[0] = 0
        e[298:300] = 0
    assert np.array_equal(ds, exp[0]) and np.array_equal(dm.astype(bool), exp[1])
    assert hm[1:CHUNK].any() and hm[2 * CHUNK:298].any()     # (the chunks' other docs have hits to keep)
    # unit 0's second chunk out of order
    bad = flat.copy()
    bad[[CHUNK + 3, CHUNK + 4]] = bad[[CHUNK + 4, CHUNK + 3]]
    ds, dm = dev_call(bad)
    exp = hs.copy(), hm.copy()
    for e in exp:
        e[CHUNK:2 * CHUNK] = 0
    assert hm[CHUNK:2 * CHUNK].any()
    assert np.array_equal(ds, exp[0]) and np.array_equal(dm.astype(bool), exp[1])
    b.close()
    sr.close()


def case_forms(L):
    """The Python layer's two input forms."""
    seg = synth.build_segment(5_000, 48)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]
    filters = [Or([by_term(0), by_term(1)]), And([by_term(0), by_term(2)]), by_term(5)]
    b = sr.batch(search.prepare(filters, BM25(), st), 10)
    per = [np.arange(1, 400, 3), [5, 9, 4000], np.zeros(0, np.int64)]
    sc, mt = b.score_docs(per)
    assert [s.size for s in sc] == [133, 3, 0] and [m.dtype for m in mt] == [bool] * 3
    flat = np.concatenate([np.asarray(p, np.uint32) for p in per])
    fs, fm = b.score_docs(flat, [0, 133, 136, 136])
    assert fs.dtype == np.float32 and np.array_equal(fs, np.concatenate(sc)) and np.array_equal(fm, np.concatenate(mt))
    only, none = b.score_docs(per, matched=False)
    assert none is None and all(np.array_equal(x, y) for x, y in zip(only, sc))
    for q, f in enumerate(filters):
        check_list(("forms", q), per[q], sc[q], mt[q], want("flat", seg, X(f), BM25()))
    with pytest.raises(ValueError):
        b.score_docs(per[:2])
    with pytest.raises(ValueError):
        b.score_docs(flat, [0, 133, 136])
    with pytest.raises(ValueError):
        b.score_docs(flat, [0, 133, 136, 135])
    with pytest.raises(_lib.IrsHipError) as e:
        b.score_docs([[3, 2], [], []])
    assert e.value.status == _lib.EINVAL
    b.close()
    sr.close()


# ------------------------------------------------------------------- CPU --

def test_symbols_exist(simlib):
    assert hasattr(simlib, "irs_hip_batch_score_docs") and hasattr(simlib, "irs_hip_batch_score_docs_to_device")


def test_score_docs_forms(simlib):
    case_forms(simlib)


def test_score_docs_abi_emulated(simlib):
    case_abi(simlib)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_score_docs_lists_emulated(simlib, layout):
    case_lists(simlib, layout)


def test_score_docs_parity_emulated(simlib):
    case_parity(simlib, 50_000, 128, synth.LAYOUT_SIMD4)


def test_score_docs_multi_emulated(simlib):
    case_multi(simlib, (9_000, 4_000, 14_000), (96, 64, 80))


def test_score_docs_device_emulated(simlib):
    case_device(simlib, 10_000, 64)


# --------------------------------------------------------------------- GPU --

@pytest.mark.gpu
def test_score_docs_abi_gpu(gpulib):
    case_abi(gpulib)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_score_docs_lists_gpu(gpulib, layout):
    case_lists(gpulib, layout)


@pytest.mark.gpu
def test_score_docs_parity_gpu(gpulib):
    case_parity(gpulib, 50_000, 128, synth.LAYOUT_SIMD4)


@pytest.mark.gpu
def test_score_docs_multi_gpu(gpulib):
    case_multi(gpulib, (9_000, 4_000, 14_000), (96, 64, 80))


@pytest.mark.gpu
def test_score_docs_device_gpu(gpulib):
    case_device(gpulib, 10_000, 64)
