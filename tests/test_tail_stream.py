"""The tail stream (pool.h): a batch whose whole score stage is the one paired launch
ends its run — k_join_rescore, k_select, the status copy, `done` — on a stream of the library, beside
the pilot of the next batch on the caller's stream.  Stream order on the caller's stream no longer
covers the end of a run, so everything here is about ORDER: batches in flight together, replays,
destroy, host copies, a second caller stream, a recovery re-run while another batch's tail is
pending — and about which batches keep the path they had.

Every sequence runs twice, with the knob on and with IRS_HIP_TAIL_STREAM=0: the results must agree
bit for bit and with the oracle, and irs_hip_batch_tail_stream_used must say what was taken.  One
body per case, emulator (synchronous: the code paths) and GPU (the ordering).  The segment is
test_join_score_lean's: 2 x 16320 + 7000 docs, under 300 k postings; pairing forced."""
from __future__ import annotations

import math

import numpy as np
import pytest

import cases
import parity
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, And, Or, by_phrase, by_term
from test_join_score_lean import _open
from test_join_slab_images import BT, _Env, _same

KS = (3, 100)
TIES_DOCS = 3 * BT + 7000


def _batch_filters(terms, seed):
    """About 40 plain disjunctions of 1, 2, 8 and 16 terms, boosts within half a decade."""
    rng = np.random.default_rng(seed)
    names = [n for n in terms if n != "full"]   # (on every doc of a tile: alone and in pairs only)
    out = [by_term(terms[n]) for n in ("full", "lone", "last", "big")]
    for n_terms, count in ((1, 8), (2, 10), (8, 10), (16, 8)):
        for _ in range(count):
            pick = [names[i] for i in rng.choice(len(names), n_terms, replace=False)]
            boosts = 10.0 ** rng.uniform(-0.25, 0.25, n_terms)
            subs = [by_term(terms[n], float(w)) for n, w in zip(pick, boosts)]
            out.append(subs[0] if n_terms == 1 else Or(subs))
    out.append(Or([by_term(terms["full"]), by_term(terms["edge", 2])]))
    return out


class _Lean:
    """The segment, three batches' queries (A, B, C) prepared for BM25, and their oracle check."""

    def __init__(self, L):
        self.L = L
        self.seg, self.sr, self.terms, _ = _open(L)
        self.stats = [parity.segment_stats(self.seg)]
        self.filters = [_batch_filters(self.terms, 4100 + i) for i in range(3)]
        self.preps = [search.prepare(f, BM25(), self.stats) for f in self.filters]

    def batch(self, i, k, paired=2):
        return self.sr.batch(self.preps[i], k).set_path(_lib.PATH_JOINED).set_paired_tiles(paired)

    def check(self, i, k, out):
        parity.check_single_segment(self.seg, self.filters[i], BM25(), k, *out)

    def close(self):
        self.sr.close()


def _copy(res):
    return [np.array(x, copy=True) for x in res]


def _listed(res):
    """Host results are the device's rows as they are: only the first counts[q] hits of a row are
    results (results() hands out zeros behind them)."""
    hits, counts, totals = _copy(res)
    for q, n in enumerate(counts.reshape(-1)):
        hits.reshape(counts.size, -1)[q, int(n):] = 0
    return [hits, counts, totals]


def _on_off(sequence, what):
    """`sequence(tail)` -> list of results, with the knob on and off: the same bit for bit; the
    first list (oracle-checked by the sequence itself) is returned."""
    got = {}
    for tail in (True, False):
        with _Env(IRS_HIP_TAIL_STREAM=int(tail)):
            got[tail] = sequence(tail)
    assert len(got[True]) == len(got[False])
    for i, (a, b) in enumerate(zip(got[True], got[False])):
        _same(a, b, (what, i, "knob on / off"))
    return got[True]


def case_three_in_flight(L, streams=None):
    """A, B, C — never seen before — run before any result is taken; results in order.  `streams`:
    the caller's stream of each (GPU tier: A and C on one, B on another)."""
    w = _Lean(L)
    streams = streams or (None, None, None)
    for k in KS:
        def sequence(tail):
            bs = [w.batch(i, k) for i in range(3)]
            for b, st in zip(bs, streams):
                b.run(st)
            out = []
            for i, b in enumerate(bs):
                out.append(_copy(b.results()))
                assert b.tail_stream_used() == tail and b.paired_tiles() and b.reruns() == 0, (i, k, tail)
            for b in bs:
                b.close()
            if tail:
                for i in range(3):
                    w.check(i, k, out[i])
            return out
        _on_off(sequence, ("three in flight", k))
    w.close()


def case_rerun(L):
    """One batch run twice back to back with no result call between, and run -> results -> run:
    the second run rewrites what the first one's tail reads."""
    w = _Lean(L)
    for k in KS:
        def sequence(tail):
            b = w.batch(0, k)
            first = _copy(b.run().run().results())
            assert b.tail_stream_used() == tail
            second = _copy(b.run().results())
            third = _copy(b.run().run().run().results())
            assert b.tail_stream_used() == tail and b.reruns() == 0
            b.close()
            _same(first, second, ("replayed", k, tail))
            _same(first, third, ("replayed thrice", k, tail))
            if tail:
                w.check(0, k, first)
            return [first]
        _on_off(sequence, ("re-run", k))
    w.close()


def case_destroy(L):
    """A destroyed right after B's run is queued: destroy waits for A's own end (on the tail
    stream), not for the caller's stream, and B's results are still right."""
    w = _Lean(L)
    for k in KS:
        def sequence(tail):
            a, b = w.batch(0, k), w.batch(1, k)
            a.run()
            b.run()
            a.close()
            out = _copy(b.results())
            assert b.tail_stream_used() == tail
            c = w.batch(2, k).run()   # (and a batch that takes over A's pooled buffers)
            out_c = _copy(c.results())
            b.close()
            c.close()
            if tail:
                w.check(1, k, out)
                w.check(2, k, out_c)
            return [out, out_c]
        _on_off(sequence, ("destroy", k))
    w.close()


def case_host_results(L):
    """results_to_host() / host_results() of A, taken after B's run is queued: the copy on the
    download stream gets behind A's tail."""
    w = _Lean(L)
    for k in KS:
        def sequence(tail):
            a, b = w.batch(0, k), w.batch(1, k)
            a.run()
            b.run()
            host = _listed(a.results_to_host().host_results())
            assert a.tail_stream_used() == tail
            plain = _copy(a.results())
            out_b = _listed(b.results_to_host().host_results())
            a.close()
            b.close()
            _same(host, plain, ("host results against results", k, tail))
            if tail:
                w.check(0, k, host)
                w.check(1, k, out_b)
            return [host, out_b]
        _on_off(sequence, ("host results", k))
    w.close()


def _ties(L):
    """The ties batch of test_join_slab_images (case_ties): thousands of docs with one sum at the
    k-th score."""
    rng = np.random.default_rng(53)

    def term(n, tf):
        d = np.sort(rng.choice(TIES_DOCS, n, replace=False)).astype(np.uint32) + 1
        return d, np.full(n, tf, np.uint32)
    lists = [term(5000, 3), term(3000, 3), term(2000, 2), term(2000, 2)]
    lists += [term(1500, 1) for _ in range(8)]
    seg, sr = cases.open_lists(L, lists, TIES_DOCS, synth.LAYOUT_SIMD4, norms=np.full(TIES_DOCS, 9, np.uint8))
    filters = [by_term(0), by_term(1), Or([by_term(2), by_term(3)]), Or([by_term(j) for j in range(4, 12)])]
    return seg, sr, filters


def case_recovery(L, k=1000):
    """The ties batch with a candidate buffer of k slots (configure(cand_cap = k)): its first run
    overflows.  B is queued behind it before A's results are taken, so A's re-run — on A's stream,
    from the host — meets B's pending tail."""
    w = _Lean(L)
    seg, sr, filters = _ties(L)
    scorer = BM25()
    prep = search.prepare(filters, scorer, [parity.segment_stats(seg)])

    def sequence(tail):
        a = sr.batch(prep, k).configure(0, 0, k).set_path(_lib.PATH_JOINED).set_paired_tiles(2)
        b = w.batch(1, 100)
        a.run()
        b.run()
        out_a = _copy(a.results())
        assert a.reruns() >= 1 and a.paired_tiles() and a.tail_stream_used() == tail
        out_b = _copy(b.results())
        assert b.reruns() == 0 and b.tail_stream_used() == tail
        n = a.reruns()
        _same(out_a, a.run().results(), ("ties, replayed", tail))   # (the grown buffer stays)
        assert a.reruns() == n
        a.close()
        b.close()
        if tail:
            parity.check_single_segment(seg, filters, scorer, k, *out_a)
            cases._exact_ties(seg, filters, scorer, k, out_a[0], out_a[1])
            w.check(1, 100, out_b)
        return [out_a, out_b]
    _on_off(sequence, "recovery")
    sr.close()
    w.close()


def case_not_taken(L, k=100):
    """Batches whose score stage is more than the one paired launch keep today's path: an Or + And
    mix, two segments under a shared threshold, a by_phrase batch, a batch on 32-bit tiles."""
    w = _Lean(L)
    t = w.terms
    # an Or + And mix
    mix = w.filters[0][:12] + [And([by_term(t["big"]), by_term(t["or16", j])]) for j in range(4)]
    prep = search.prepare(mix, BM25(), w.stats)

    def mixed(tail):
        b = w.sr.batch(prep, k).set_paired_tiles(2)
        out = _copy(b.run().results())
        assert not b.tail_stream_used()
        b.close()
        if tail:
            parity.check_single_segment(w.seg, mix, BM25(), k, *out)
        return [out]
    _on_off(mixed, "Or + And")

    # 32-bit tiles
    def unpaired(tail):
        b = w.batch(0, k, paired=0)
        out = _copy(b.run().results())
        assert not b.tail_stream_used() and not b.paired_tiles()
        b.close()
        if tail:
            w.check(0, k, out)
        return [out]
    plain = _on_off(unpaired, "32-bit tiles")

    def paired(tail):   # (... and the same batch paired: on the tail, the same bits)
        b = w.batch(0, k)
        out = _copy(b.run().results())
        assert b.tail_stream_used() == tail
        b.close()
        return [out]
    _same(plain[0], _on_off(paired, "paired")[0], "paired against 32-bit tiles")
    w.close()

    # two segments, one threshold per query
    sizes = (40_000, 12_000)
    segs = [synth.build_segment(n, 256, first_doc=f) for n, f in zip(sizes, (0, sizes[0]))]
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    ranks = synth.make_queries(8, 8, 4, 256, synth.SEED + 23)
    filters = [Or([by_term(int(r) - 1) for r in row]) for row in ranks] + [by_term(3)]
    prep2 = search.prepare(filters, BM25(), [parity.segment_stats(s) for s in segs])
    ref = parity.oracle_topk(segs, filters, BM25(), k)

    def shared(tail):
        arrays = search.QueryArrays.from_prepared(readers, prep2, k)
        b = search.QueryBatch(readers, arrays).set_path(_lib.PATH_JOINED).set_paired_tiles(2)
        b.set_shared_threshold(True)
        h, c, tot = _copy(b.run().results())
        assert b.paired_tiles() and not b.tail_stream_used()
        b.close()
        if tail:
            merged = search.merge_topk_host([(h[i], c[i]) for i in range(len(segs))], k)
            for q, (rows, (ohits, total)) in enumerate(zip(merged, ref)):
                assert len(rows) == len(ohits) and int(tot[:, q].sum()) == total, q
                a = np.array([r[0] for r in rows], np.float32)
                assert np.allclose(a, np.sort(ohits["score"])[::-1], rtol=parity.REL_TOL, atol=0), q
        return [[h, c, tot]]
    _on_off(shared, "shared threshold")
    for r in readers:
        r.close()

    # by_phrase
    pseg = synth.build_segment(20_000, 128, with_positions=True)
    psr = search.SegmentReader.from_synth(pseg, L=L)
    phrases = [by_phrase([0, 1]), by_phrase([2, 0]), by_phrase([1, 4, 0]), by_phrase([5])]
    pprep = search.prepare(phrases, BM25(), [parity.segment_stats(pseg)])

    def phrase(tail):
        b = psr.batch(pprep, k)
        out = _copy(b.run().results())
        assert not b.tail_stream_used()
        b.close()
        if tail:
            parity.check_phrase_segment(pseg, phrases, BM25(), k, *out)
        return [out]
    _on_off(phrase, "by_phrase")
    psr.close()


def case_profile(L):
    """profile(True): the four stage times of a tail run — K_SCORE ends and K_SELECT lies on the
    tail stream — are finite and not negative."""
    w = _Lean(L)
    for k in KS:
        a = w.batch(0, k).profile(True)
        b = w.batch(1, k).profile(True)
        a.run()
        b.run()
        for i, x in enumerate((a, b)):
            out = _copy(x.results())
            assert x.tail_stream_used()
            ms = x.timings()
            assert len(ms) == _lib.K_COUNT == 4
            assert all(math.isfinite(v) and v >= 0.0 for v in ms), (k, ms)
            w.check(i, k, out)
            x.close()
    w.close()


CASES = (case_three_in_flight, case_rerun, case_destroy, case_host_results, case_recovery,
         case_not_taken, case_profile)


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_tail_stream_emulated(simlib, case):
    case(simlib)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_tail_stream_gpu(gpulib, case):
    case(gpulib)


@pytest.mark.gpu
def test_two_caller_streams_gpu(gpulib):
    """A on the current stream, B on a second stream, C on the first again: B's score launch waits
    for A's tail, C's for B's — whichever caller stream they were queued on."""
    import torch
    other = torch.cuda.Stream()
    cur = torch.cuda.current_stream().cuda_stream or None
    case_three_in_flight(gpulib, streams=(cur, other.cuda_stream, cur))
    torch.cuda.synchronize()
