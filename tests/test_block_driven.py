"""Block-driven conjunctions and phrases (conj.h k_conj; phrase.h k_phrase2 / k_phrase<MT>;
vphrase.h k_vphrase) on the paths that only run when something goes wrong, and config 5's shape.

  * the pilot pass samples lead items {phase, phase + P, ...} of every unit (ensure_pilot_list;
    phase = (unit * 7) % P, unit = segment * queries + query) and k_conj_threshold picks the bin
    that holds margin * k * sampled / total of them.  When every high-scoring match sits in the
    sampled items the estimate is too high: k_select must raise kStatusUnderflow and recover_now
    re-run the batch with the sound threshold.  Under block-max WAND the skipped lead blocks are
    never evaluated and do not count in `hits`: `pruned[unit]` is then the only sign;
  * more candidates than slots (a configured cap, and the default cap's 16384 floor): the buffer
    grows (recover_overflow), and later batches on the same segments start with the size the
    failed one needed (cand_cap_hint);
  * config 5 in miniature: 8 consecutive segments with positions and MaxFreq wand data, AND-of-2..4
    under WAND and 2-word phrases, one QueryBatch per class.

Every case compares with the oracle (docs, counts, totals exactly; scores within 1e-5) and asserts
the path and the re-runs it was built to cause.  Runs under WAND compare with the exhaustive run
bit for bit in docs, scores and counts; their totals only count evaluated docs, so they may only be
smaller — except where the construction fixes them.  One body runs on the emulator (CPU tier) and
on the GPU."""
from __future__ import annotations

import os

import numpy as np
import pytest

import oracle
import parity
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import TFIDF, And, by_phrase, by_term

STRIDE = 16          # the pilot stride the misled cases configure
LEAD_BLOCKS = 64     # full 128-posting blocks of a lead term, no tail
HOT_TF = 50          # frequency (or phrase frequency) of every match in a hot lead block
MISLED_K = 1000      # > the 512 hot matches of a unit, < 3 * k * 4 / 64 = 188 of them needed


def pilot_phase(unit, stride=STRIDE):
    """The first lead item the pilot pass samples for `unit` (ensure_pilot_list)."""
    return (unit * 7) % stride


def _stack(x, multi):
    return x if multi else x[None]


def _batch(readers, prep, k, stride=0, cap=0, wand=False):
    b = search.QueryBatch(readers if len(readers) > 1 else readers[0], prep, k)
    b.configure(0, stride, cap).set_path(_lib.PATH_ITEMS)
    if wand:
        b.set_wand(True)
    return b


def _results(b, n_segs):
    return tuple(_stack(x.copy(), n_segs > 1) for x in b.results())


def _same(a, b, totals=True, what=""):
    assert np.array_equal(a[0], b[0]), ("hits", what)
    assert np.array_equal(a[1], b[1]), ("counts", what)
    if totals:
        assert np.array_equal(a[2], b[2]), ("totals", what)
    else:
        assert (a[2] <= b[2]).all(), ("pruned totals above the exhaustive ones", what)


def _trace_status(capfd):
    """The `[irs_hip] re-run:` lines IRS_HIP_TRACE printed since the last read."""
    return [ln for ln in capfd.readouterr().err.splitlines() if "[irs_hip] re-run:" in ln]


def _check_merged(merged, ref, what=""):
    """merge_topk_host rows (score, segment, doc) against the oracle's harness run."""
    for q, (rows, (ohits, _)) in enumerate(zip(merged, ref)):
        assert len(rows) == len(ohits), ("merged count", what, q)
        if not rows:
            continue
        got = np.array([r[0] for r in rows], np.float32)
        want = np.sort(ohits["score"])[::-1]
        assert np.allclose(got, want, rtol=parity.REL_TOL, atol=0), ("merged scores", what, q)
        kth = float(want[-1])
        above = lambda pairs: {p for p in pairs if p[0] > kth * (1 + 2 * parity.REL_TOL)}
        g = above((float(sc), int(s), int(d)) for sc, s, d in rows)
        o = above((float(h["score"]), int(h["segment"]), int(h["doc"])) for h in ohits)
        assert {(s, d) for _, s, d in g} == {(s, d) for _, s, d in o}, ("merged docs", what, q)


def _phrase_topk(segs, phrases, scorer, k):
    """The merged top k of fixed phrases by the oracle's exhaustive phrase scores, in the shape of
    parity.oracle_topk (segment = index in `segs`, doc = the segment's own id)."""
    osc = parity.oracle_scorer(scorer)
    dwf = sum(s.docs_with_field for s in segs)
    ttf = sum(s.total_term_freq for s in segs)
    out = []
    for ph in phrases:
        dwt = [sum(int(s.metas[t]["docs_count"]) if 0 <= t < len(s.metas) else 0 for s in segs)
               for t in ph.terms]
        rows = []
        for si, seg in enumerate(segs):
            sc, pf = oracle.score_all_phrase(parity.oracle_view(seg), parity.metas_for(seg, ph.terms),
                                             ph.offsets, osc, dwf, dwt, ttf, ph.boost)
            docs = np.nonzero(pf > 0)[0]
            rows += [(-float(sc[d]), si, int(d)) for d in docs]
        rows.sort()
        hits = np.zeros(min(k, len(rows)), oracle.HIT)
        for i, (sc, si, d) in enumerate(rows[:k]):
            hits[i] = (-sc, d, si)
        out.append((hits, len(rows)))
    return out


# ------------------------------------------------------- misled pilot (And) --

def _lead(phase):
    """A lead term of LEAD_BLOCKS full blocks (docs 2, 4, ...): tf HOT_TF in the blocks the pilot
    samples at `phase`, tf 1 elsewhere (phase None: no hot block)."""
    docs = 2 * np.arange(1, LEAD_BLOCKS * 128 + 1, dtype=np.uint32)
    blk = np.arange(docs.size) // 128
    hot = (blk % STRIDE == phase) if phase is not None else np.zeros(docs.size, bool)
    return docs, np.where(hot, HOT_TF, 1).astype(np.uint32)


def _misled_conj_segments(L, layout, n_segs, nq, shift):
    """Per segment: one lead per query (term q), hot at its unit's phase + shift, then two terms
    that hold every doc with tf 1 (terms nq, nq + 1)."""
    n_docs = 2 * LEAD_BLOCKS * 128 + 100
    dense = np.arange(1, n_docs + 1, dtype=np.uint32)
    segs, readers = [], []
    for s in range(n_segs):
        lists = [_lead((pilot_phase(s * nq + q) + shift) % STRIDE) for q in range(nq)]
        lists += [(dense, np.ones(n_docs, np.uint32))] * 2
        seg = synth.segment_from_lists(lists, n_docs, layout, norms=False)
        segs.append(seg)
        readers.append(search.SegmentReader.from_synth(seg, L=L))
    return segs, readers


def _conj_filters(nq):
    return [And([by_term(0), by_term(nq)]), And([by_term(1), by_term(nq), by_term(nq + 1)])][:nq]


def _check_conj(segs, filters, scorer, k, res):
    h, c, t = res
    for s, seg in enumerate(segs):
        parity.check_single_segment(seg, filters, scorer, k, h[s], c[s], t[s], all_segs=segs)
    if len(segs) > 1:
        merged = search.merge_topk_host([(h[s], c[s]) for s in range(len(segs))], k)
        _check_merged(merged, parity.oracle_topk(segs, filters, scorer, k))


def case_conj_pilot_misled(L, layout=synth.LAYOUT_SIMD4, n_segs=1, capfd=None):
    """k_conj without WAND, And of two and of three terms: every high-scoring match lies in the
    lead blocks the pilot samples for its unit, so the estimated threshold bin holds only those
    512 docs while k = 1000: k_select sees fewer than k candidates and more hits — one re-run,
    exact results, still one after a second run(), bit for bit the stride-1 batch.  The control
    (hot blocks half a stride off the sampled phase) does not re-run."""
    nq, k, scorer = 2, MISLED_K, TFIDF(False)
    filters = _conj_filters(nq)
    for shift, reruns in ((0, 1), (STRIDE // 2, 0)):
        segs, readers = _misled_conj_segments(L, layout, n_segs, nq, shift)
        prep = search.prepare(filters, scorer, [parity.segment_stats(s) for s in segs])
        ref_b = _batch(readers, prep, k, stride=1)
        ref = _results(ref_b.run(), n_segs)
        assert ref_b.reruns() == 0
        ref_b.close()
        _check_conj(segs, filters, scorer, k, ref)
        os.environ["IRS_HIP_TRACE"] = "1"
        try:
            if capfd is not None:
                capfd.readouterr()
            b = _batch(readers, prep, k, stride=STRIDE)
            assert b.reruns() == 0
            got = _results(b.run(), n_segs)
            assert b.reruns() == reruns and b.path() == _lib.PATH_ITEMS, (shift, b.reruns())
            if capfd is not None:
                lines = _trace_status(capfd)
                assert len(lines) == reruns, lines
                if reruns:   # underflow only; every unit short of k with more hits than listed
                    assert "status 4, %d units short of k" % (nq * n_segs) in lines[0], lines
        finally:
            os.environ.pop("IRS_HIP_TRACE", None)
        _same(got, ref, what=("first run", shift))
        again = _results(b.run(), n_segs)
        assert b.reruns() == reruns, "a re-run batch keeps its sound threshold"
        _same(again, ref, what=("second run", shift))
        b.close()
        for r in readers:
            r.close()


def case_conj_pruned_only(L, layout=synth.LAYOUT_SIMD4, capfd=None):
    """The same data under WAND.  The pilot's bin is the hot one; every unsampled lead block holds
    tf-1 docs whose block-max bound (lead tf 1 + the dense terms' tf 1) lies below it, so step 0
    skips it: the failed run evaluates exactly the 512 hot docs and lists them all (hits == n).
    Only `pruned[unit]` tells k_select that the threshold was too high.  One re-run; the result
    is the exhaustive batch's bit for bit — totals included, since the sound re-run's threshold
    bin is 0 and prunes nothing — and the oracle's."""
    nq, k, scorer = 2, MISLED_K, TFIDF(False)
    filters = _conj_filters(nq)
    segs, readers = _misled_conj_segments(L, layout, 1, nq, 0)
    prep = search.prepare(filters, scorer, [parity.segment_stats(segs[0])])
    ex = _batch(readers, prep, k, stride=1)
    ref = _results(ex.run(), 1)
    assert ex.reruns() == 0
    ex.close()
    _check_conj(segs, filters, scorer, k, ref)
    os.environ["IRS_HIP_TRACE"] = "1"
    try:
        if capfd is not None:
            capfd.readouterr()
        b = _batch(readers, prep, k, stride=STRIDE, wand=True)
        got = _results(b.run(), 1)
        assert b.reruns() == 1 and b.path() == _lib.PATH_ITEMS, b.reruns()
        if capfd is not None:
            lines = _trace_status(capfd)
            # underflow, and no unit listed fewer docs than its hit count said
            assert len(lines) == 1 and "status 4, 0 units short of k" in lines[0], lines
    finally:
        os.environ.pop("IRS_HIP_TRACE", None)
    _same(got, ref, what="wand")
    again = _results(b.run(), 1)
    assert b.reruns() == 1
    _same(again, ref, what="wand, second run")
    b.close()
    readers[0].close()


# ---------------------------------------------------- misled pilot (phrases) --

def _misled_phrase_segment(L, layout, shift):
    """Leads 0 and 1 (docs 2, 4, ...): lead q has phrase frequency HOT_TF in the blocks sampled for
    unit q, 1 elsewhere — lead positions 1, 4, 7, ...; term 2 one after every lead position
    (and at 1 in the other docs), term 3 two after; term 4 (odd docs) never next to a lead."""
    n_docs = 2 * LEAD_BLOCKS * 128 + 100
    h = []
    leads = []
    for q in range(2):
        docs, tf = _lead((pilot_phase(q) + shift) % STRIDE)
        leads.append((docs, tf))
        h.append(tf)
    lead_docs = leads[0][0]
    reps = np.ones(n_docs + 1, np.int64)
    reps[lead_docs] = np.maximum(h[0], h[1])

    def pos_list(docs, counts, first):
        return np.concatenate([first + 3 * np.arange(int(c), dtype=np.uint32) for c in counts])
    lists = [(d, tf, pos_list(d, tf, 1)) for d, tf in leads]
    dense = np.arange(1, n_docs + 1, dtype=np.uint32)
    cnt = reps[1:].astype(np.uint32)
    lists.append((dense, cnt, pos_list(dense, cnt, 2)))
    lists.append((dense, cnt, pos_list(dense, cnt, 3)))
    odd = np.arange(1, 257, 2, dtype=np.uint32)
    lists.append((odd, np.ones(odd.size, np.uint32), np.full(odd.size, 5, np.uint32)))
    seg = synth.segment_from_lists(lists, n_docs, layout, norms=False)
    return seg, search.SegmentReader.from_synth(seg, L=L)


def case_phrase_pilot_misled(L, layout=synth.LAYOUT_SIMD4):
    """The same for phrases: hot phrase matches only in the lead blocks the pilot samples, k = 1000
    against 512 of them.  A batch of 2-word phrases (k_phrase2), one of 3-word phrases
    (k_phrase<4>) and one holding a variadic phrase (k_vphrase runs both its phrases): one re-run
    each, the oracle's results, bit for bit the stride-1 batch; the control does not re-run."""
    from test_variadic_phrase import _Pos, check as check_variadic
    k, scorer = MISLED_K, TFIDF(False)
    batches = [[by_phrase([0, 2]), by_phrase([1, 2])],
               [by_phrase([0, 2, 3]), by_phrase([1, 2, 3])],
               [by_phrase([0, 2]), by_phrase([1, [2, 4]])]]
    for shift, reruns in ((0, 1), (STRIDE // 2, 0)):
        seg, sr = _misled_phrase_segment(L, layout, shift)
        pos = _Pos(seg)
        for phrases in batches:
            prep = search.prepare(phrases, scorer, [parity.segment_stats(seg)])
            ref_b = sr.batch(prep, k).configure(0, 1, 0)
            ref = tuple(x.copy() for x in ref_b.run().results())
            assert ref_b.reruns() == 0
            ref_b.close()
            for q, ph in enumerate(phrases):
                if ph.variadic:
                    check_variadic(seg, pos, ph, prep[q], k, ref[0][q], ref[1][q], ref[2][q])
                else:
                    parity.check_phrase_segment(seg, [ph], scorer, k, ref[0][q:q + 1], ref[1][q:q + 1],
                                                ref[2][q:q + 1])
            assert int(ref[2].min()) == LEAD_BLOCKS * 128
            b = sr.batch(prep, k).configure(0, STRIDE, 0)
            got = tuple(x.copy() for x in b.run().results())
            assert b.reruns() == reruns and b.path() == _lib.PATH_ITEMS, (phrases, shift, b.reruns())
            _same(got, ref, what=(phrases, shift))
            again = tuple(x.copy() for x in b.run().results())
            assert b.reruns() == reruns
            _same(again, ref, what=(phrases, shift, "second run"))
            b.close()
        sr.close()


# ------------------------------------------- the blocks the follower walk decodes --

def case_walk_touched(L, layout=synth.LAYOUT_SIMD4):
    """Which blocks follow_list (lead.h) decodes, pinned by the bytes a counting run reports.  Term 0
    holds every doc: each of its blocks is all-equal in docs and in frequencies, 2 header bytes + 1
    + 1.  Term 1 is its first block alone.  A lead of one block, docs step, 2 * step, ..., 128 * step,
    ends on the LAST doc of block `step` - 1 of term 0: exactly `step` blocks of term 0 hold a lead
    doc and the next one starts right behind dhi.  Against term 1 the same lead decodes one such
    block, so the two runs differ by (step - 1) * 4 bytes whatever the lead block itself costs.
    step = 16: two docs per bucket, one directory round; step = 80: 80 wanted blocks, a second
    round.  A block decoded twice, or the block behind dhi, shows as 4 bytes more.  (Lead blocks
    uncut: a piece decodes the lead block again.)"""
    n_docs = 128 * 90
    dense = np.arange(1, n_docs + 1, dtype=np.uint32)
    steps = (16, 80)
    lists = [(dense, np.ones(dense.size, np.uint32)), (dense[:128], np.ones(128, np.uint32))]
    for step in steps:
        d = step * np.arange(1, 129, dtype=np.uint32)
        lists.append((d, np.ones(d.size, np.uint32)))
    seg = synth.segment_from_lists(lists, n_docs, layout, norms=False)
    sr = search.SegmentReader.from_synth(seg, L=L)
    st = [parity.segment_stats(seg)]

    def doc_bytes(flt, hits):
        b = sr.batch(search.prepare([flt], TFIDF(False), st), 200).set_path(_lib.PATH_ITEMS).profile(3)
        h, c, tot = b.run().results()
        assert int(tot[0]) == hits and b.path() == _lib.PATH_ITEMS and b.reruns() == 0, (flt, int(tot[0]))
        parity.check_single_segment(seg, [flt], TFIDF(False), 200, h, c, tot)
        got, positions = b.touched()
        b.close()
        assert positions == 0
        return got
    os.environ["IRS_HIP_CONJ_SPLIT_LOG2"] = "0"
    try:
        for t, step in enumerate(steps, start=2):
            whole = doc_bytes(And([by_term(t), by_term(0)]), 128)
            one = doc_bytes(And([by_term(t), by_term(1)]), 128 // step)
            print("walk touched: step %d, %d bytes against every doc, %d against its first block" % (step, whole, one))
            assert whole - one == (step - 1) * 4, (step, whole, one)
    finally:
        os.environ.pop("IRS_HIP_CONJ_SPLIT_LOG2", None)
    sr.close()


# ------------------------------------------------------- candidate overflow --

def _overflow_segments(L, layout, sizes, seed, missing=None):
    """Three terms of random density with tf 1..3 (few distinct scores: long ties); segment
    `missing` has no term 2."""
    segs, readers = [], []
    for i, n in enumerate(sizes):
        rng = np.random.default_rng(seed + i)
        lists = []
        for share in (0.6, 0.5, 0.3)[:2 if i == missing else 3]:
            d = np.nonzero(rng.random(n) < share)[0].astype(np.uint32) + 1
            lists.append((d, rng.integers(1, 4, d.size).astype(np.uint32)))
        seg = synth.segment_from_lists(lists, n, layout, norms=False)
        segs.append(seg)
        readers.append(search.SegmentReader.from_synth(seg, L=L))
    return segs, readers


def case_conj_overflow(L, layout=synth.LAYOUT_SIMD4, sizes=(20_000,), missing=None, k=10):
    """k_conj with a configured candidate cap far below the matches (cap 16 for k = 10), WAND off
    and on: the batch re-runs with a grown buffer and returns the uncapped batch's results —
    exact against the oracle — on one segment or on several in one batch (a term missing from
    one of them)."""
    scorer = TFIDF(False)
    segs, readers = _overflow_segments(L, layout, sizes, 41, missing)
    filters = [And([by_term(0), by_term(1)]), And([by_term(0), by_term(1), by_term(2)]),
               And([by_term(2), by_term(0)])]
    prep = search.prepare(filters, scorer, [parity.segment_stats(s) for s in segs])
    ref_b = _batch(readers, prep, k)
    ref = _results(ref_b.run(), len(segs))
    assert ref_b.reruns() == 0
    ref_b.close()
    _check_conj(segs, filters, scorer, k, ref)
    assert int(ref[2].max()) > 16 * 100
    for wand in (False, True):
        b = _batch(readers, prep, k, cap=16, wand=wand)
        got = _results(b.run(), len(segs))
        assert b.reruns() >= 1 and b.path() == _lib.PATH_ITEMS, (wand, b.reruns())
        _same(got, ref, totals=not wand, what=("capped", wand))
        b.close()
    for r in readers:
        r.close()


def case_conj_default_cap(L, layout=synth.LAYOUT_SIMD4, sizes=(40_000,)):
    """More than 16384 matches tie in one score bin (two terms holding every doc with tf 1,
    TF-IDF without norms): past the floor of default_cand_cap.  On fresh segments the batch
    overflows and re-runs once with a grown buffer; a fresh batch on the same segments then starts
    with that size (cand_cap_hint) and runs once.  WAND off and on, one segment or several (the
    third query's term is missing from the second segment)."""
    scorer, k = TFIDF(False), 10
    filters = [And([by_term(0), by_term(1)]), And([by_term(1), by_term(0), by_term(2)])]
    for wand in (False, True):
        segs, readers = [], []
        for i, n in enumerate(sizes):
            dense = (np.arange(1, n + 1, dtype=np.uint32), np.ones(n, np.uint32))
            lists = [dense, dense] + ([] if i == 1 else [dense])
            seg = synth.segment_from_lists(lists, n, layout, norms=False)
            segs.append(seg)
            readers.append(search.SegmentReader.from_synth(seg, L=L))
        assert min(sizes) > 16384
        prep = search.prepare(filters, scorer, [parity.segment_stats(s) for s in segs])
        first = _batch(readers, prep, k, wand=wand)
        res = _results(first.run(), len(segs))
        assert first.reruns() == 1 and first.path() == _lib.PATH_ITEMS, (wand, first.reruns())
        first.close()
        _check_conj(segs, filters, scorer, k, res)
        fresh = _batch(readers, prep, k, wand=wand)
        again = _results(fresh.run(), len(segs))
        assert fresh.reruns() == 0, ("cand_cap_hint", wand)
        _same(again, res, what=("fresh batch", wand))
        fresh.close()
        for r in readers:
            r.close()


# --------------------------------------------------------- config 5 in small --

def check_skip_entries(sr, seg, term):
    """term_blockmax of a list in a field with positions and MaxFreq wand data against its level-0
    skip entries (oracle.read_skip0): entry by entry (max freq; a frequency-only payload reads as
    norm == freq), the list's last full block — no entry — derived from the postings."""
    wc = int(seg.wand_count)
    sl, _, _, mf, nm = oracle.read_skip0(seg.doc_file, seg.metas[term], wc, True, has_pos=True)
    d, f = oracle.decode_term(seg.doc_file, seg.metas[term], seg.layout, wand_count=wc)
    gmf, gmn = sr.term_blockmax(term)
    assert len(gmf) == len(d) // 128 and len(sl) >= len(gmf) - 1 and len(sl) > 0
    assert np.array_equal(gmf[:len(sl)], mf[:len(gmf)]), "max freq of the skip entries"
    assert np.array_equal(gmn[:len(sl)], nm[:len(gmf)]), "norm of the skip entries"
    for b in range(len(sl), len(gmf)):
        blk = slice(128 * b, 128 * b + 128)
        assert gmf[b] == f[blk].max(), b
        assert gmn[b] == seg.norms[d[blk] - 1].min(), b
    return len(sl)


def config5_queries(n_and, n_phrase, lo, hi, set_index=0):
    """bench.py --config 5's query shapes: AND-of-2/3/4 (a third each) and 2-word phrases."""
    ands = []
    for n_terms in (2, 3, 4):
        for row in synth.make_queries((n_and + 2) // 3, n_terms, lo, hi,
                                      synth.SEED + 5 + n_terms + 100 * set_index):
            ands.append(And([by_term(int(r) - 1) for r in row]))
    phrases = [by_phrase([int(r) - 1 for r in row])
               for row in synth.make_queries(n_phrase, 2, lo, hi, synth.SEED + 9 + 100 * set_index)]
    return ands[:n_and], phrases


def case_config5_small(L, per=12_000, n_segs=8, n_and=24, n_phrase=24, lo=8, hi=256, k=100):
    """Config 5 in miniature: 8 consecutive segments with positions and MaxFreq wand data (the
    pairs WAND prunes with read from the index, k_wand_skip0), TF-IDF without norms, k = 100; one
    QueryBatch per class, WAND on the AND batch.  WAND == exhaustive bit for bit; every segment's
    lists == a single-segment batch on it and == the oracle with all segments' statistics; the
    merged top k == the oracle's harness run.  Returns the hits WAND did not evaluate.  (At these
    sizes that is 0: the pilot's sample floor, kPilotMinSample = 48 docs from every 64th lead
    block, puts the threshold far below the k-th score.  Pruning itself is checked by
    case_conj_pruned_only and cases.case_wand_equals_exhaustive.)"""
    scorer = TFIDF(False)
    segs = [synth.build_segment(per, 4096, first_doc=s * per, with_positions=True, wand_count=1,
                                wand_kind=synth.WAND_MAX_FREQ) for s in range(n_segs)]
    readers = [search.SegmentReader.from_synth(s, L=L) for s in segs]
    for sr in readers:
        assert sr.wand_source()[0] > 0
    longest = int(np.argmax(segs[0].metas["docs_count"]))
    assert check_skip_entries(readers[0], segs[0], longest) > 1
    stats = [parity.segment_stats(s) for s in segs]
    ands, phrases = config5_queries(n_and, n_phrase, lo, hi)
    for name, filters in (("and", ands), ("phrase", phrases)):
        prep = search.prepare(filters, scorer, stats)
        arrays = search.QueryArrays.from_prepared(readers, prep, k)
        b = search.QueryBatch(readers, arrays)
        if name == "and":
            b.set_wand(True)
        h, c, t = (x.copy() for x in b.run().results())
        assert b.path() == _lib.PATH_ITEMS
        b.close()
        if name == "and":
            ex = search.QueryBatch(readers, arrays)
            eh, ec, et = (x.copy() for x in ex.run().results())
            ex.close()
            assert np.array_equal(h, eh) and np.array_equal(c, ec), "WAND != exhaustive"
            assert (t <= et).all()
            pruned = int(et.sum() - t.sum())
            t = et
        assert int(c.sum()) > 0
        for s, (seg, sr) in enumerate(zip(segs, readers)):
            one = sr.batch(prep, k)
            if name == "and":
                one.set_wand(True)
            oh, oc, ot = one.run().results()
            one.close()
            assert np.array_equal(oh, h[s]) and np.array_equal(oc, c[s]), (name, s)
            if name == "phrase":
                assert np.array_equal(ot, t[s]), (name, s)
                parity.check_phrase_segment(seg, filters, scorer, k, h[s], c[s], t[s], all_segs=segs)
            else:
                parity.check_single_segment(seg, filters, scorer, k, h[s], c[s], t[s], all_segs=segs)
        merged = search.merge_topk_host([(h[s], c[s]) for s in range(n_segs)], k)
        ref = (parity.oracle_topk(segs, filters, scorer, k) if name == "and"
               else _phrase_topk(segs, filters, scorer, k))
        _check_merged(merged, ref, name)
    for r in readers:
        r.close()
    return pruned


# ------------------------------------------------------------------ emulator --

@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_conj_pilot_misled_emulated(simlib, layout, capfd):
    case_conj_pilot_misled(simlib, layout, capfd=capfd)


def test_conj_pilot_misled_segments_emulated(simlib, capfd):
    case_conj_pilot_misled(simlib, n_segs=3, capfd=capfd)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_conj_pruned_only_emulated(simlib, layout, capfd):
    case_conj_pruned_only(simlib, layout, capfd=capfd)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_phrase_pilot_misled_emulated(simlib, layout):
    case_phrase_pilot_misled(simlib, layout)


@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_walk_touched_emulated(simlib, layout):
    case_walk_touched(simlib, layout)


def test_conj_overflow_emulated(simlib):
    case_conj_overflow(simlib)


def test_conj_overflow_segments_emulated(simlib):
    case_conj_overflow(simlib, sizes=(20_000, 8_000, 30_000), missing=1)


def test_conj_default_cap_emulated(simlib):
    case_conj_default_cap(simlib)


def test_conj_default_cap_segments_emulated(simlib):
    case_conj_default_cap(simlib, sizes=(20_000, 17_000, 25_000))


def test_config5_small_emulated(simlib):
    case_config5_small(simlib)


# ----------------------------------------------------------------------- GPU --

@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_conj_pilot_misled_gpu(gpulib, layout, capfd):
    case_conj_pilot_misled(gpulib, layout, capfd=capfd)


@pytest.mark.gpu
def test_conj_pilot_misled_segments_gpu(gpulib, capfd):
    case_conj_pilot_misled(gpulib, n_segs=3, capfd=capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_conj_pruned_only_gpu(gpulib, layout, capfd):
    case_conj_pruned_only(gpulib, layout, capfd=capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_phrase_pilot_misled_gpu(gpulib, layout):
    case_phrase_pilot_misled(gpulib, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR])
def test_walk_touched_gpu(gpulib, layout):
    case_walk_touched(gpulib, layout)


@pytest.mark.gpu
def test_conj_overflow_gpu(gpulib):
    case_conj_overflow(gpulib, sizes=(200_000,))


@pytest.mark.gpu
def test_conj_overflow_segments_gpu(gpulib):
    case_conj_overflow(gpulib, sizes=(200_000, 60_000, 300_000), missing=1)


@pytest.mark.gpu
def test_conj_default_cap_gpu(gpulib):
    case_conj_default_cap(gpulib, sizes=(200_000,))


@pytest.mark.gpu
def test_conj_default_cap_segments_gpu(gpulib):
    case_conj_default_cap(gpulib, sizes=(40_000, 17_000, 120_000))


@pytest.mark.gpu
def test_config5_small_gpu(gpulib):
    case_config5_small(gpulib, per=250_000, n_and=96, n_phrase=96, lo=16, hi=2048)
