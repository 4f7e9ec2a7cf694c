"""Unscored execution (irs_hip_batch_match_sets / _to_device): filter::prepared::execute with
Scorers::kUnordered (filter.hpp:52-78) — the full match set of every unit as a bitset, and its count.

Expected sets come from the oracle, unchanged: score_all(...)[1] for Or / And / min-match on
parity.oracle_view of the masked segment, grouped Ands composed as test_nested_boolean.expected
composes them, exclusions expressed as extra mask docs, score_all_phrase(...)[1] > 0 for plain
phrases, and for variadic phrases a restatement over oracle.decode_positions written below.  Every
unit of every case is compared bit for bit with its oracle set, and `counts` with its population.
Every case also runs the batch scored (k = MAX_K): counts == total_hits, and where total_hits <= MAX_K
the returned docs are the set.  One body per case, on the emulator (CPU tier) and on the GPU at a
larger size.

Segments without frequencies: irs_hip_batch_create refuses them (IRS_HIP_EUNSUPPORTED, scorers need
IndexFeatures::FREQ), so there is no batch to take match sets of — case_device pins that refusal."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

import oracle
import parity
import test_nested_boolean as nb
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, And, Not, Or, by_phrase, by_term

MAX_K = _lib.MAX_K


# ------------------------------------------------------------- expectations --

def bits_of(row, num_docs):
    """bool[num_docs + 1] of one u64 row; every bit behind num_docs must be clear."""
    b = np.unpackbits(np.ascontiguousarray(row).view(np.uint8), bitorder="little").astype(bool)
    assert not b[num_docs + 1:].any(), "bits behind the segment's last doc"
    assert not b[0], "doc 0 does not exist"
    return b[:num_docs + 1]


def X(inner, ex):
    """(filter with Not(by_term(x)) for x in ex, inner filter, ex)."""
    return (And([inner] + [Not(by_term(x)) for x in ex]) if ex else inner, inner, list(ex))


def phrase_freq_variadic(seg, parts, offsets):
    """{doc: freq} of a variadic phrase, restated over the oracle's position decoder:
    freq(d) = sum over t in P_0 of #{p in pos(t, d): every later part has a member with p + off_i}."""
    def pos_of(t):
        out = {}
        if 0 <= t < len(seg.metas) and int(seg.metas[t]["docs_count"]):
            d, f = oracle.decode_term(seg.doc_file, seg.metas[t], seg.layout)
            p = oracle.decode_positions(seg.doc_file, seg.pos_file, seg.metas[t], seg.layout)
            at = np.concatenate([[0], np.cumsum(f.astype(np.int64))])
            for i, doc in enumerate(d.tolist()):
                out[int(doc)] = p[at[i]:at[i + 1]].astype(np.int64)
        return out
    lists = [[pos_of(t) for t in part] for part in parts]
    cand = None
    for part in lists:
        docs = set().union(*[set(m) for m in part]) if part else set()
        cand = docs if cand is None else cand & docs
    out = {}
    for d in sorted(cand or ()):
        f = 0
        for lead in lists[0]:
            ok = np.ones(len(lead.get(d, ())), bool)
            for part, off in zip(lists[1:], offsets[1:]):
                hit = np.zeros(ok.size, bool)
                for m in part:
                    if d in m and ok.size:
                        hit |= np.isin(lead[d] + off, m[d])
                ok &= hit
            f += int(ok.sum())
        if f:
            out[d] = f
    return out


def want_set(seg, inner, ex, all_segs=None):
    """bool[num_docs + 1]: the docs `inner` minus the excluded terms matches on seg, by the oracle."""
    present = [x for x in ex if 0 <= x < len(seg.metas)]
    masked = nb._masked(seg, present)
    view = parity.oracle_view(masked)
    osc = parity.oracle_scorer(BM25())
    n1 = seg.num_docs + 1
    if isinstance(inner, by_phrase):
        if inner.variadic:
            out = np.zeros(n1, bool)
            docs = np.array(sorted(phrase_freq_variadic(seg, inner.parts(), inner.offsets)), np.int64)
            out[docs] = True
            gone = getattr(masked, "doc_mask", None)
            if gone is not None:
                g = np.asarray(gone, np.int64)
                out[g[(g >= 1) & (g < n1)]] = False
            return out
        if any(not (0 <= t < len(seg.metas)) or int(seg.metas[t]["docs_count"]) == 0 for t in inner.terms):
            return np.zeros(n1, bool)   # no phrase state without one of its terms (phrase_filter.cpp:254-258)
        dwt = [int(seg.metas[t]["docs_count"]) for t in inner.terms]
        _, pf = oracle.score_all_phrase(view, parity.metas_for(seg, inner.terms), inner.offsets, osc,
                                        seg.docs_with_field, dwt, seg.total_term_freq)
        return pf[:n1] > 0
    if isinstance(inner, And) and any(not isinstance(s, by_term) for s in inner.subs):
        return nb.expected(seg, inner, BM25(), all_segs, excluded=present)[1][:n1]
    op, subs = search._terms_of(inner)
    terms = [s.term for s in subs]
    dwt = [int(seg.metas[t]["docs_count"]) if 0 <= t < len(seg.metas) else 0 for t in terms]
    _, m = oracle.score_all(view, parity.metas_for(seg, terms), parity.oracle_op(inner, op), osc,
                            seg.docs_with_field, dwt, seg.total_term_freq, [1.0] * len(terms))
    return m[:n1].astype(bool)


def check_units(seg, triples, sets, counts, scored=None, all_segs=None):
    """Every unit's row against the oracle, its count against the population; no deleted doc; and
    against a scored k = MAX_K run (h, c, t) of the same batch.  Returns (#units with total_hits <=
    MAX_K, #units above)."""
    gone = getattr(seg, "doc_mask", None)
    small = big = 0
    for q, (_, inner, ex) in enumerate(triples):
        got = bits_of(sets[q], seg.num_docs)
        want = want_set(seg, inner, ex, all_segs)
        assert np.array_equal(got, want), ("set", q, inner, ex, int(got.sum()), int(want.sum()),
                                           np.nonzero(got != want)[0][:8])
        assert int(counts[q]) == int(want.sum()), ("count", q, inner)
        if gone is not None:
            assert not got[np.asarray(gone, np.int64)].any(), ("a deleted doc in the set", q)
        if scored is not None:
            h, c, t = scored
            assert int(counts[q]) == int(t[q]), ("count vs total_hits", q, int(counts[q]), int(t[q]))
            if int(t[q]) <= MAX_K:
                small += 1
                assert np.array_equal(np.sort(h[q, :int(c[q])]["doc"].astype(np.int64)), np.nonzero(got)[0]), q
            else:
                big += 1
    return small, big


def run_case(sr, seg, triples, st=None, k=MAX_K, all_segs=None):
    st = st or [parity.segment_stats(seg)]
    b = sr.batch(search.prepare([t[0] for t in triples], BM25(), st), k)
    sets, counts = b.match_sets()
    scored = tuple(x.copy() for x in b.run().results())
    sets2, counts2 = b.match_sets()
    assert np.array_equal(sets, sets2) and np.array_equal(counts, counts2), "sets differ after run()"
    only, c3 = b.match_sets(sets=False)
    assert only is None and np.array_equal(c3, counts)
    b.close()
    return check_units(seg, triples, sets, counts, scored, all_segs)


class knob:
    """An environment knob for the batches created inside (read at create)."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = str(self.value)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


# -------------------------------------------------------------------- cases --

def boolean_shapes(seg, R):
    """The boolean shapes of the issue: (filter, inner, excluded) each."""
    A = 10 * R   # an absent term
    T = lambda *ts: [by_term(t) for t in ts]
    tail, one = nb._rare(seg, 2, 128), nb._rare(seg, 1, 2)
    fl = [
        X(by_term(3), []),
        X(Or(T(1, R // 2)), []), X(Or(T(*range(2, 10))), []), X(Or(T(*range(16))), []),
        X(And(T(0, 2)), []), X(And(T(R // 3, 2, 1)), []), X(And(T(0, 1, 2, 3)), []),
        X(Or(T(0, 1, 2), min_match=2), []), X(Or(T(0, 1, 2, 3), min_match=3), []),
        X(Or(T(*range(8)), min_match=7), []), X(Or(T(*range(16)), min_match=16), []),
        X(Or(T(*range(R // 2, R // 2 + 16)), min_match=5), []),
        # Not on each op
        X(by_term(1), [2]), X(Or(T(4, 5, 6)), [0, R // 2]), X(And(T(0, 1)), [2, A]),
        X(Or(T(0, 1, 2, 3), min_match=2), [4]), X(And(T(0, 1)), [0]),
        # absent terms, an empty group
        X(Or(T(1, A)), []), X(And(T(1, A)), []), X(Or(T(1, 2, A), min_match=2), []),
        X(Or(T(1, A, A + 1), min_match=2), []), X(by_term(A), []),
        X(And([by_term(1), Or(T(A, A + 1))]), []),
        # a term twice in one query
        X(Or(T(5, 5)), []), X(And(T(5, 5, 6)), []), X(Or(T(5, 5, 6), min_match=2), []),
        # rare leads: most slices are left early
        X(And(T(R - 1, 0)), []), X(And(T(R - 2, R - 1)), []),
    ]
    if tail is not None:
        fl += [X(by_term(tail), []), X(Or(T(tail, R - 1)), []), X(And(T(tail, 0)), []),
               X(Or(T(tail, 0, 1), min_match=2), [])]
    if one is not None:
        fl += [X(by_term(one), []), X(And(T(one, 0)), []), X(Or(T(one, 0, 1), min_match=2), []),
               X(And(T(0, 1)), [one])]
    fl += [X(f, []) for f in nb.shape_filters(seg, R)]
    fl += [X(f, ex) for f, ex in zip(nb.shape_filters(seg, R), ([1], [R // 2, A], [6, 7]) * 5)]
    return fl


def case_shapes(L, num_docs, max_rank, layout, deletions=False):
    seg = synth.build_segment(num_docs, max_rank, layout=layout)
    if deletions:   # 5 % random deletions plus a contiguous run
        rng = np.random.default_rng(31)
        seg.doc_mask = np.concatenate([rng.choice(num_docs, num_docs // 20, replace=False).astype(np.uint32) + 1,
                                       np.arange(100, 700, dtype=np.uint32),
                                       np.array([1, num_docs], np.uint32)])
    sr = search.SegmentReader.from_synth(seg, L=L)
    small, big = run_case(sr, seg, boolean_shapes(seg, max_rank))
    assert small > 0 and big > 0, (small, big)   # both comparisons against the scored run were made
    sr.close()


def border_lists(num_docs, slice_docs):
    """Posting lists with docs at every border: doc 1, num_docs, multiples of the slice size +- 1,
    of 64 and of 128-doc blocks."""
    edge = {1, 2, 63, 64, 65, num_docs - 1, num_docs}
    for s in range(slice_docs, num_docs, slice_docs):
        edge |= {s - 1, s, s + 1}
    edge = np.array(sorted(d for d in edge if 1 <= d <= num_docs), np.uint32)
    rng = np.random.default_rng(5)
    dense = np.unique(np.concatenate([edge, rng.choice(num_docs, num_docs // 3, replace=False).astype(np.uint32) + 1]))
    half = np.unique(np.concatenate([edge[::2], rng.choice(num_docs, num_docs // 7, replace=False).astype(np.uint32) + 1]))
    every = np.arange(1, num_docs + 1, dtype=np.uint32)
    ones = lambda d: (d, np.ones(d.size, np.uint32))
    return [ones(edge), ones(dense), ones(half), ones(every), ones(edge[-1:]), ones(edge[:1])]


def case_borders(L, layout):
    num_docs, slice_docs = 9000, 64 * 32
    seg = synth.segment_from_lists(border_lists(num_docs, slice_docs), num_docs, layout)
    seg.doc_mask = np.array([64, slice_docs + 1, num_docs - 1], np.uint32)
    sr = search.SegmentReader.from_synth(seg, L=L)
    T = lambda *ts: [by_term(t) for t in ts]
    fl = [X(by_term(t), []) for t in range(6)]
    fl += [X(Or(T(0, 2)), []), X(And(T(0, 1)), []), X(And(T(0, 1, 2, 3)), []), X(And(T(3, 3)), []),
           X(Or(T(0, 1, 2, 3), min_match=3), []), X(Or(T(0, 1, 2), min_match=2), [4]),
           X(And(T(3, 0)), [5]), X(And([Or(T(4, 5)), Or(T(0, 3))]), []), X(Or(T(4, 5)), []),
           X(And(T(4, 3)), []), X(by_term(3), [0])]
    for v in (64, None):   # 2048-doc slices, and the default (one slice)
        with knob("IRS_HIP_MATCH_SLICE", v):
            small, big = run_case(sr, seg, fl)
            assert small > 0 and big > 0, (small, big)
    sr.close()


def case_cross(L, num_docs, max_rank):
    """Against the scored path: at least a third of the units below MAX_K matches (their docs are
    compared), at least a third above (their totals are)."""
    seg = synth.build_segment(num_docs, max_rank)
    sr = search.SegmentReader.from_synth(seg, L=L)
    dc = np.asarray(seg.metas["docs_count"]).astype(np.int64)
    rare = [int(t) for t in np.nonzero((dc > 0) & (dc < MAX_K // 4))[0]][-24:]
    freq = [int(t) for t in np.nonzero(dc > 3 * MAX_K)[0]][:16]
    assert len(rare) >= 12 and len(freq) >= 8, (len(rare), len(freq))
    T = lambda *ts: [by_term(t) for t in ts]
    fl = []
    for i in range(0, 12, 3):
        a, b_, c_ = rare[i:i + 3]
        fl += [X(by_term(a), []), X(Or(T(a, b_, c_)), []), X(And(T(a, freq[0])), []),
               X(Or(T(a, b_, freq[1]), min_match=2), []), X(And([Or(T(a, b_)), Or(T(freq[0], freq[1]))]), [c_])]
    for i in range(0, 8, 2):
        a, b_ = freq[i:i + 2]
        fl += [X(by_term(a), []), X(Or(T(a, b_)), []), X(Or(T(*freq[:8])), [rare[0]]),
               X(Or(T(*freq[:4]), min_match=2), []), X(And(T(freq[0], freq[1])), [])]
    small, big = run_case(sr, seg, fl)
    assert 3 * small >= len(fl) and 3 * big >= len(fl), (small, big, len(fl))
    sr.close()


def case_independence(L, num_docs, max_rank):
    """The slice knob, runs before / after, every setter, a forced re-run: the sets stay what they
    are; and the scored results are byte-identical with and without match_sets calls in between."""
    seg = synth.build_segment(num_docs, max_rank)
    rng = np.random.default_rng(7)
    seg.doc_mask = rng.choice(num_docs, num_docs // 20, replace=False).astype(np.uint32) + 1
    st = [parity.segment_stats(seg)]
    sr = search.SegmentReader.from_synth(seg, L=L)
    triples = boolean_shapes(seg, max_rank)
    prep = search.prepare([t[0] for t in triples], BM25(), st)
    ref = None
    for v in (64, 256, 2048, 8192, None):
        with knob("IRS_HIP_MATCH_SLICE", v):
            b = sr.batch(prep, 100)
            sets, counts = b.match_sets()
            b.close()
        if ref is None:
            ref = (sets, counts)
            check_units(seg, triples, sets, counts)
        assert np.array_equal(sets, ref[0]) and np.array_equal(counts, ref[1]), ("slice knob", v)
    # plain scored results, nothing in between
    b = sr.batch(prep, 100)
    plain = tuple(x.copy() for x in b.run().results())
    plain2 = tuple(x.copy() for x in b.run().results())
    plain_reruns = b.reruns()
    b.close()
    b = sr.batch(prep, 100)
    s0, c0 = b.match_sets()
    b.run()
    s1, c1 = b.match_sets()
    got = tuple(x.copy() for x in b.results())
    s2, c2 = b.match_sets()
    got2 = tuple(x.copy() for x in b.run().results())
    assert b.reruns() == plain_reruns
    b.close()
    for s, c in ((s0, c0), (s1, c1), (s2, c2)):
        assert np.array_equal(s, ref[0]) and np.array_equal(c, ref[1])
    for x, y in zip(plain + plain2, got + got2):
        assert x.tobytes() == y.tobytes(), "scored results changed by match_sets"
    # setters and a forced re-run
    half = np.array([plain[0][q, plain[1][q] // 2]["score"] if plain[1][q] else 0.0
                     for q in range(len(triples))], np.float32)
    for name, setup in (("wand", lambda b: b.set_wand(True)),
                        ("min scores", lambda b: b.set_min_scores(half)),
                        ("items", lambda b: b.set_path(_lib.PATH_ITEMS)),
                        ("joined", lambda b: b.set_path(_lib.PATH_JOINED)),
                        ("cand_cap", lambda b: b.configure(cand_cap=100))):
        b = sr.batch(prep, 100)
        setup(b)
        sa, ca = b.match_sets()
        b.run().results()
        if name == "cand_cap":
            assert b.reruns() > 0
        sb, cb = b.match_sets()
        b.close()
        assert np.array_equal(sa, ref[0]) and np.array_equal(ca, ref[1]), name
        assert np.array_equal(sb, ref[0]) and np.array_equal(cb, ref[1]), name
    sr.close()


def case_multi(L, sizes, ranks):
    """create_multi over segments with different term tables and sizes: unit order, per-segment
    rows (bits behind a smaller segment's last doc stay clear), members present in some only."""
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    segs = [synth.build_segment(int(n), int(r), first_doc=int(f)) for n, r, f in zip(sizes, ranks, first)]
    segs[1].doc_mask = np.arange(10, 400, dtype=np.uint32)
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    lo, hi = min(ranks), max(ranks)
    T = lambda *ts: [by_term(t) for t in ts]
    triples = [X(by_term(hi - 1), []), X(Or(T(1, hi - 1)), []), X(And(T(0, lo + 2)), []),
               X(And(T(0, 1)), [lo + 1]), X(Or(T(0, lo - 1, hi - 2), min_match=2), []),
               X(And([Or(T(1, hi - 1)), Or(T(0, lo + 2))]), []), X(Or(T(2, 3, 4)), [hi - 3])]
    stats = [parity.segment_stats(s) for s in segs]
    qb = search.QueryBatch(readers, search.prepare([t[0] for t in triples], BM25(), stats), MAX_K)
    n_words = qb.match_words()
    assert n_words == max(sizes) // 64 + 1
    sets, counts = qb.match_sets()
    h, c, t = qb.run().results()
    assert sets.shape == (len(segs) * len(triples), n_words)
    nq = len(triples)
    for i, s in enumerate(segs):
        check_units(s, triples, sets[i * nq:(i + 1) * nq], counts[i * nq:(i + 1) * nq],
                    (h[i], c[i], t[i]), segs)
    wide, cw = qb.match_sets(n_words + 5)
    assert np.array_equal(wide[:, :n_words], sets) and not wide[:, n_words:].any() and np.array_equal(cw, counts)
    qb.close()
    for r in readers:
        r.close()


def case_device(L, num_docs, max_rank):
    """match_sets_to_device into torch buffers equals the host form; counts-only and sets-only
    calls; IRS_HIP_EINVAL for both outputs NULL and for n_words too small."""
    import torch
    arch = C.create_string_buffer(64)
    L.irs_hip_device_arch(0, arch, 64)
    dev = "cpu" if arch.value.endswith(b"-sim") else "cuda"
    seg = synth.build_segment(num_docs, max_rank)
    seg.doc_mask = np.arange(50, 90, dtype=np.uint32)
    sr = search.SegmentReader.from_synth(seg, L=L)
    triples = boolean_shapes(seg, max_rank)[:24]
    b = sr.batch(search.prepare([t[0] for t in triples], BM25(), [parity.segment_stats(seg)]), 100)
    n_words, nq = b.match_words(), len(triples)
    sets, counts = b.match_sets()

    def sync():
        if dev == "cuda":
            torch.cuda.synchronize()

    def fresh():   # (old content must be overwritten, not OR-ed into)
        return (torch.full((nq, n_words), -1, dtype=torch.int64, device=dev),
                torch.full((nq,), -1, dtype=torch.int64, device=dev))
    ds, dc = fresh()
    b.match_sets_to_device(ds.data_ptr(), n_words, dc.data_ptr())
    sync()
    assert np.array_equal(ds.cpu().numpy().view(np.uint64), sets)
    assert np.array_equal(dc.cpu().numpy().view(np.uint64), counts)
    b.run()   # (a run queued behind a device-form call)
    ds, dc = fresh()
    b.match_sets_to_device(None, n_words, dc.data_ptr())
    b.match_sets_to_device(ds.data_ptr(), n_words, None)
    sync()
    assert np.array_equal(ds.cpu().numpy().view(np.uint64), sets)
    assert np.array_equal(dc.cpu().numpy().view(np.uint64), counts)
    h, c, t = b.results()
    assert np.array_equal(t, counts)
    for call in (lambda: b.match_sets_to_device(None, n_words, None),
                 lambda: b.match_sets_to_device(ds.data_ptr(), num_docs // 64, dc.data_ptr()),
                 lambda: b.match_sets(num_docs // 64),
                 lambda: b.match_sets(0)):
        with pytest.raises(_lib.IrsHipError) as e:
            call()
        assert e.value.status == _lib.EINVAL
    assert L.irs_hip_batch_match_sets(b.handle, None, n_words, None) == _lib.EINVAL
    assert L.irs_hip_batch_match_sets(None, None, n_words, None) == _lib.EINVAL
    b.close()
    sr.close()
    # a segment without frequencies opens, but no batch can be made of it: nothing to take sets of
    docs = np.arange(1, 400, 3, dtype=np.uint32)
    nseg = synth.segment_from_lists([(docs, None), (docs[::2], None)], 2000, norms=False)
    nsr = search.SegmentReader.from_synth(nseg, L=L, has_freq=False)
    with pytest.raises(_lib.IrsHipError) as e:
        nsr.batch(search.prepare([Or([by_term(0), by_term(1)])], BM25(), [parity.segment_stats(nseg)]), 10)
    assert e.value.status == _lib.EUNSUPPORTED
    nsr.close()


def phrase_shapes(seg, R, variadic):
    A = 10 * R
    tail = nb._rare(seg, 2, 128)
    fl = [X(by_phrase([3, 4]), []), X(by_phrase([0, 1]), []), X(by_phrase([1, 0], [0, 2]), []),
          X(by_phrase([0, 1, 2], [0, 1, 3]), []), X(by_phrase([2, 0, 1]), []),
          X(by_phrase([0, 1, 2, 3]), []), X(by_phrase([5, 2, 0, 1], [0, 1, 3, 4]), []),
          X(by_phrase([R // 2, 1]), []), X(by_phrase([0, 0]), []),
          X(by_phrase([0, 1]), [2]), X(by_phrase([0, 1, 2], [0, 1, 3]), [R // 2, A]),
          X(by_phrase([1, A]), []), X(by_phrase([A, 1, 2]), [])]
    if tail is not None:
        fl += [X(by_phrase([tail, 0]), []), X(by_phrase([0, tail], [0, 2]), [])]
    if variadic:
        fl += [X(by_phrase([[0, 1], [2, 3]]), []), X(by_phrase([0, [1, 2, 3]]), []),
               X(by_phrase([[3, 4, 5], 0, [1, 2]], [0, 1, 3]), []),
               X(by_phrase([[0, 1], [2, 3]]), [4]), X(by_phrase([[0, A], [1, 2]]), []),
               X(by_phrase([[A, A + 1], [1, 2]]), []),   # an empty part: no phrase state
               X(by_phrase([[R // 2, R // 2 + 1], [0, 1], 2]), [])]
    return fl


def case_phrases(L, num_docs, max_rank, layout, variadic):
    seg = synth.build_segment(num_docs, max_rank, layout=layout, with_positions=True)
    rng = np.random.default_rng(3)
    seg.doc_mask = np.concatenate([rng.choice(num_docs, num_docs // 20, replace=False).astype(np.uint32) + 1,
                                   np.arange(200, 500, dtype=np.uint32)])
    sr = search.SegmentReader.from_synth(seg, L=L)
    triples = phrase_shapes(seg, max_rank, variadic)
    run_case(sr, seg, triples)
    # the device form, and a forced re-run in between
    import torch
    arch = C.create_string_buffer(64)
    L.irs_hip_device_arch(0, arch, 64)
    dev = "cpu" if arch.value.endswith(b"-sim") else "cuda"
    b = sr.batch(search.prepare([t[0] for t in triples], BM25(), [parity.segment_stats(seg)]), 10)
    b.configure(cand_cap=16)
    sets, counts = b.match_sets()
    h, c, t = b.run().results()
    nq, n_words = len(triples), b.match_words()
    ds = torch.full((nq, n_words), -1, dtype=torch.int64, device=dev)
    dc = torch.full((nq,), -1, dtype=torch.int64, device=dev)
    b.match_sets_to_device(ds.data_ptr(), n_words, dc.data_ptr())
    if dev == "cuda":
        torch.cuda.synchronize()
    assert np.array_equal(ds.cpu().numpy().view(np.uint64), sets)
    assert np.array_equal(dc.cpu().numpy().view(np.uint64), counts) and np.array_equal(t, counts)
    check_units(seg, triples, sets, counts)
    b.close()
    sr.close()


def _cpp(L, tmp_path, extra=()):
    """tests/cpp/test_match_sets.cpp: execute_unscored and QueryBatch::match_sets of the C++ layer,
    checked by the program itself against the oracle's C API."""
    import subprocess
    from pathlib import Path
    from iresearch_amd import _build
    root = Path(__file__).resolve().parents[1]
    synth_lib, orc = _build.build_synth(), oracle.build()
    exe = tmp_path / "test_match_sets"
    lib = Path(L._name)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall",
           "-I", str(root / "include"), "-I", str(root / "iresearch_amd" / "cpp"),
           "-I", str(root / "iresearch_amd" / "index"), "-I", str(root / "oracle"),
           str(root / "tests" / "cpp" / "test_match_sets.cpp"), "-o", str(exe), str(lib), str(synth_lib),
           str(orc), "-pthread", "-Wl,-rpath," + str(lib.parent), "-Wl,-rpath," + str(Path(synth_lib).parent),
           "-Wl,-rpath," + str(Path(orc).parent), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "test_match_sets OK" in run.stdout, (run.stdout + run.stderr)[-3000:]


# ------------------------------------------------------------------- CPU --

def test_cpp_match_sets_emulated(simlib, tmp_path):
    _cpp(simlib, tmp_path)


def test_symbols_exist(simlib):
    assert hasattr(simlib, "irs_hip_batch_match_sets") and hasattr(simlib, "irs_hip_batch_match_sets_to_device")


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_match_shapes_emulated(simlib, layout):
    case_shapes(simlib, 20_000, 96, layout)


def test_match_deletions_emulated(simlib):
    case_shapes(simlib, 15_000, 64, synth.LAYOUT_SIMD4, deletions=True)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_match_borders_emulated(simlib, layout):
    case_borders(simlib, layout)


def test_match_cross_emulated(simlib):
    case_cross(simlib, 60_000, 512)


def test_match_independence_emulated(simlib):
    case_independence(simlib, 12_000, 64)


def test_match_multi_emulated(simlib):
    case_multi(simlib, (9_000, 4_000, 14_000), (96, 64, 80))


def test_match_device_emulated(simlib):
    case_device(simlib, 10_000, 64)


@pytest.mark.parametrize("variadic", [False, True])
def test_match_phrases_emulated(simlib, variadic):
    case_phrases(simlib, 6_000, 48, synth.LAYOUT_SIMD4, variadic)


def test_match_phrases_emulated_scalar(simlib):
    case_phrases(simlib, 4_000, 32, synth.LAYOUT_SCALAR, True)


# --------------------------------------------------------------------- GPU --

@pytest.mark.gpu
def test_cpp_match_sets_gpu(gpulib, tmp_path):
    rocm = "/opt/rocm/lib"
    _cpp(gpulib, tmp_path, ["-Wl,-rpath," + rocm, "-Wl,-rpath-link," + rocm, "-Wl,--allow-shlib-undefined"])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_match_shapes_gpu(gpulib, layout):
    case_shapes(gpulib, 1_000_000, 1024, layout)


@pytest.mark.gpu
def test_match_deletions_gpu(gpulib):
    case_shapes(gpulib, 1_000_000, 1024, synth.LAYOUT_SIMD4, deletions=True)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_match_borders_gpu(gpulib, layout):
    case_borders(gpulib, layout)


@pytest.mark.gpu
def test_match_cross_gpu(gpulib):
    case_cross(gpulib, 250_000, 4096)   # (rank 4096 stays below MAX_K / 4 docs at this size)


@pytest.mark.gpu
def test_match_independence_gpu(gpulib):
    case_independence(gpulib, 600_000, 512)


@pytest.mark.gpu
def test_match_multi_gpu(gpulib):
    case_multi(gpulib, (700_000, 300_000, 1_000_000), (512, 256, 384))


@pytest.mark.gpu
def test_match_device_gpu(gpulib):
    case_device(gpulib, 500_000, 512)


@pytest.mark.gpu
@pytest.mark.parametrize("variadic", [False, True])
def test_match_phrases_gpu(gpulib, variadic):
    case_phrases(gpulib, 300_000, 512, synth.LAYOUT_SIMD4, variadic)


@pytest.mark.gpu
def test_match_phrases_gpu_scalar(gpulib):
    case_phrases(gpulib, 200_000, 256, synth.LAYOUT_SCALAR, True)


def _at_size(L, seg, filters, inner_of, sample=32):
    """1000 queries: counts of all units against the scored totals, the sets of `sample` units
    against the oracle — into device memory, only those rows copied back."""
    import time

    import torch
    st = [parity.segment_stats(seg)]
    sr = search.SegmentReader.from_synth(seg, L=L)
    b = sr.batch(search.prepare(filters, BM25(), st), 100)
    nq, n_words = len(filters), b.match_words()
    ds = torch.empty((nq, n_words), dtype=torch.int64, device="cuda")
    dc = torch.empty((nq,), dtype=torch.int64, device="cuda")
    b.match_sets_to_device(ds.data_ptr(), n_words, dc.data_ptr())   # (first call: tables go out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b.match_sets_to_device(ds.data_ptr(), n_words, dc.data_ptr())
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    counts = dc.cpu().numpy().view(np.uint64)
    _, only = b.match_sets(sets=False)
    assert np.array_equal(only, counts)
    h, c, t = b.run().results()
    assert np.array_equal(counts, t), np.nonzero(counts != t)[0][:8]
    for q in range(0, nq, nq // sample):
        row = ds[q].cpu().numpy().view(np.uint64)
        got = bits_of(row, seg.num_docs)
        want = want_set(seg, inner_of(filters[q]), [])
        assert np.array_equal(got, want), (q, filters[q])
        assert int(counts[q]) == int(want.sum())
    print("match sets at size: %d units x %d docs in %.2f ms" % (nq, seg.num_docs, ms))
    b.close()
    sr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["and", "minmatch"])
def test_match_at_size_gpu(gpulib, shape):
    """10 M docs, 1000 queries: And-2 / And-3, and MinMatch 3 of 4."""
    seg = synth.build_segment(10_000_000, 4096)
    if shape == "and":
        r2, r3 = synth.make_queries(500, 2, 2, 4096, synth.SEED + 7), synth.make_queries(500, 3, 2, 4096, synth.SEED + 8)
        filters = [And([by_term(int(x) - 1) for x in row]) for row in r2] + \
                  [And([by_term(int(x) - 1) for x in row]) for row in r3]
    else:
        rows = synth.make_queries(1000, 4, 2, 4096, synth.SEED + 9)
        filters = [Or([by_term(int(x) - 1) for x in row], min_match=3) for row in rows]
    _at_size(gpulib, seg, filters, lambda f: f)


@pytest.mark.gpu
def test_match_at_size_phrases_gpu(gpulib):
    """1000 two-word phrases on a positions segment of the size the phrase GPU tests use."""
    seg = synth.build_segment(2_000_000, 4096, with_positions=True)
    rows = synth.make_queries(1000, 2, 2, 4096, synth.SEED + 5)
    filters = [by_phrase([int(r[0]) - 1, int(r[1]) - 1]) for r in rows]
    _at_size(gpulib, seg, filters, lambda f: f)
