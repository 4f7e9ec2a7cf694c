"""The misled-pilot re-run on the kernel families that had no case built for it: wide units
(wide.h k_wide_pilot / k_wide_score), Ors of clauses (clauses.h k_clause_pilot / k_clause_score),
grouped conjunctions (conj_any.h k_conj_any), a phrase plus required terms (k_phrase_and) and a phrase
or optional terms (k_phrase_or, its term pass — a second batch of work items under doc sets — and
k_union_topk), and nested And / Or / Not trees (tree.h k_tree_pilot / k_tree_score).

Every pilot samples part of its unit — doc tiles {phase, phase + P, ...} or lead items, phase =
(unit * 7) % P, unit = segment * queries + query — and estimates the score bin that leaves about
kPilotMargin * k = 3 k candidates.  Here every high-scoring match of a unit lies in what the pilot
samples for THAT unit: the estimate is met by the sample, the full run lists fewer than k docs
although more match, k_select raises kStatusUnderflow and recover_now (irs_hip.hip) runs the batch
again with the sound threshold (margin == 0), which is the only place that branch of a pilot runs.

What every misled case asserts (_misled): a stride-1 batch does not re-run and passes the family's own
check against the oracle; the same prepared queries with the misleading stride re-run exactly as often
as stated, with exactly one `[irs_hip] re-run:` line per re-run (status 4, the stated number of units
short of k: a phase that is wrong for some units only shows here); hits, counts and totals are bit for
bit the stride-1 batch's; the unit counters and the path are unchanged; a second run() gives the same
arrays without another re-run.  The control holds the same lists with the hot part half a stride off
every unit's phase and does not re-run.  The "uncounted" cases are controls for what a pilot must
leave out of its histogram — docs with too few terms or clauses, deleted docs: each holds decoys that
would raise the estimate above every real match, so a pilot that counted them costs a re-run.

One body per case runs on the emulator (CPU tier) and on the GPU."""
from __future__ import annotations

import os

import numpy as np
import pytest

import oracle
import parity
import test_boolean_trees as bt
import test_multiterm as mt
import test_nested_boolean as nb
import test_or_clauses as oc
import test_phrase_and as pa
import test_phrase_or as po
from iresearch_amd import search, synth
from iresearch_amd.search import BM25, TFIDF, And, Not, Or, by_phrase, by_term, by_terms
from test_block_driven import (MISLED_K, STRIDE, _misled_conj_segments, _misled_phrase_segment, _same,
                               _trace_status, pilot_phase)

TILE = 12288         # docs per accumulator tile of the wide and clause kernels (kJoinTile)
WIDE_STRIDE = 4      # configure(0, 4, 0): wide_stride / clause_stride = min(4, 8 tiles / 2)
MARGIN = 3           # kPilotMargin
MIN_SAMPLE = 48      # kPilotMinSample
HOT_TF, DECOY_TF = 50, 200
SCORERS = (TFIDF(False), BM25(1.2, 0.0))     # the square-root form and the reciprocal form
LAYOUTS = [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR]


def pilot_need(k, sampled, total):
    """Docs the estimating pilot wants at or above its bin: ceil(margin * k * sampled / total),
    at least kPilotMinSample, at most k (k_pilot, k_wide_pilot, k_clause_pilot, k_conj_threshold)."""
    est = (MARGIN * k * sampled + total - 1) // total
    return min(max(est, MIN_SAMPLE), k)


def _docs_of(seg, term):
    d, _ = oracle.decode_term(seg.doc_file, seg.metas[term], seg.layout)
    return d


def _copy(b, multi):
    return tuple(x.copy() if multi else x.copy()[None] for x in b.results())


def _misled(make, multi, check, counters, capfd, reruns, short=(), listed=None, what=""):
    """The assertions every case shares.  make(stride) -> a configured batch of the same prepared
    queries; check(results) compares [segment][query] arrays with the oracle; counters(batch) ->
    what must not change; short: per expected re-run line the units short of k; listed: (listed,
    matches) of the first such unit in the first line.  Returns the stride-1 results."""
    if isinstance(what, tuple):
        what = tuple(type(x).__name__ if isinstance(x, (BM25, TFIDF)) else x for x in what)
    ref_b = make(1)
    ref = _copy(ref_b.run(), multi)
    assert ref_b.reruns() == 0, ("the stride-1 batch re-ran", what)
    want = counters(ref_b)
    ref_b.close()
    check(ref)
    os.environ["IRS_HIP_TRACE"] = "1"
    try:
        capfd.readouterr()
        b = make(None)
        assert b.reruns() == 0
        got = _copy(b.run(), multi)
        assert b.reruns() == reruns, (what, b.reruns())
        lines = _trace_status(capfd)
        print("pilot recovery %s: %d re-runs %s" % (what, b.reruns(), [ln.split("(first")[0] for ln in lines]))
        assert len(lines) == reruns, (what, lines)
        for ln, n in zip(lines, short):    # underflow alone
            assert "re-run: status 4, %d units short of k" % n in ln, (what, lines)
        if listed is not None:
            assert "listed %d of %d matches" % listed in lines[0], (what, lines)
    finally:
        os.environ.pop("IRS_HIP_TRACE", None)
    _same(got, ref, what=(what, "first run"))
    assert counters(b) == want, (what, counters(b), want)
    again = _copy(b.run(), multi)
    assert b.reruns() == reruns, ("a re-run batch keeps its sound threshold", what)
    _same(again, ref, what=(what, "second run"))
    b.close()
    return ref


# ------------------------------------------------ doc tiles: wide units, clauses --

def _in_tile(rng, tile, n, free):
    """n docs of `tile` out of the still free ones (a bool per doc id), taken."""
    ids = 1 + tile * TILE + np.nonzero(free[1 + tile * TILE:1 + (tile + 1) * TILE])[0]
    docs = np.sort(rng.choice(ids, n, replace=False))
    free[docs] = False
    return docs


def _sampled(unit, n_tiles, shift=0, stride=WIDE_STRIDE):
    first = (pilot_phase(unit, stride) + shift) % stride
    return list(range(first, n_tiles, stride))


def _hot(rng, n_tiles, unit, shift, free, k, tf=HOT_TF):
    """The hot list of `unit`: the same number of docs with frequency `tf` in every tile the pilot
    samples for it (shift 0) — 400 each where that is two tiles, 320 where it is three — so that
    pilot_need <= hot docs < k whatever the segment's tile count."""
    tiles = _sampled(unit, n_tiles, shift)
    per = {2: 400, 3: 320}[len(tiles)]
    assert per * len(tiles) < k and (shift or pilot_need(k, len(tiles), n_tiles) <= per * len(tiles)), \
        (k, tiles, n_tiles)
    docs = np.concatenate([_in_tile(rng, t, per, free) for t in tiles])
    return docs.astype(np.uint32), np.full(docs.size, tf, np.uint32)


def _cold_pair(rng, free, shared=2000, own=1000):
    """Terms 2 and 3: 3000 random docs each with frequency 1, 2000 of them common to both."""
    ids = np.nonzero(free)[0]
    ids = ids[ids > 0]
    pick = rng.choice(ids, shared + 2 * own, replace=False)
    out = []
    for part in (pick[:shared + own], np.concatenate([pick[:shared], pick[shared + own:]])):
        d = np.sort(part).astype(np.uint32)
        out.append((d, np.ones(d.size, np.uint32)))
    return out


def _tile_segments(L, layout, tiles, shift, k, nq=2, with3=None, seed=7, hot_in2=None):
    """Per segment of tiles[s] full tiles: terms 0 .. nq - 1 = the hot lists of its units
    s * nq + q, terms 2 and 3 = _cold_pair (segment `with3` False: no term 3), term 4 = every hot doc
    with frequency 1 (only where term 3 exists).  The hot docs hold none of the cold terms — except
    in a segment `hot_in2`: there term 2 holds every hot doc too (frequency 1) and there is no
    term 4."""
    segs, readers = [], []
    for s, n_tiles in enumerate(tiles):
        rng = np.random.default_rng(seed + s)
        n_docs = n_tiles * TILE
        free = np.ones(n_docs + 1, bool)
        lists = [_hot(rng, n_tiles, s * nq + q, shift, free, k) for q in range(nq)]
        cold = _cold_pair(rng, free)
        if with3 is not None and not with3[s]:
            lists += cold[:1]
        elif hot_in2 is not None and hot_in2[s]:
            d2 = np.sort(np.concatenate([cold[0][0]] + [d for d, _ in lists])).astype(np.uint32)
            lists += [(d2, np.ones(d2.size, np.uint32)), cold[1]]
        else:
            every = np.sort(np.concatenate([d for d, _ in lists])).astype(np.uint32)
            lists += cold + [(every, np.ones(every.size, np.uint32))]
        seg = synth.segment_from_lists(lists, n_docs, layout, norms=False)
        segs.append(seg)
        readers.append(search.SegmentReader.from_synth(seg, L=L))
    return segs, readers


def _maker(readers, prep, k, stride, tile_docs=0, ref_cap=0):
    """make(None): the batch under test, configure(tile_docs, stride, 0); make(1): the stride-1
    reference (ref_cap: its candidate slots, where the data overflows the default ones)."""
    multi = len(readers) > 1

    def make(s):
        b = search.QueryBatch(readers if multi else readers[0], prep, k)
        return b.configure(tile_docs, stride if s is None else s, 0 if s is None else ref_cap)
    return make


def _close(readers):
    for r in readers:
        r.close()


def _wide_counters(b):
    return (b.wide_units(), b.clause_units(), b.tree_units(), b.path())


def _check_family(mod, segs, filters, scorer, k):
    def check(res):
        h, c, t = res
        for s, seg in enumerate(segs):
            for q, flt in enumerate(filters):
                mod.check(flt, k, h[s, q], c[s, q], t[s, q], *mod.expected(seg, flt, scorer, segs))
    return check


def _check_wide_merged(segs, filters, scorer, k, res):
    """test_multiterm.case_multi's merged top k: against the oracle's own harness run."""
    h, c, t = res
    merged = search.merge_topk_host([(h[i], c[i]) for i in range(len(segs))], k)
    for q, flt in enumerate(filters):
        ent = mt.entries(flt)
        terms = [x for x, _ in ent]
        metas = np.stack([parity.metas_for(s, terms) for s in segs])
        ref, total = oracle.search([parity.oracle_view(s) for s in segs], metas, mt.oracle_op(flt),
                                   parity.oracle_scorer(scorer), k, [x for _, x in ent])
        assert int(t[:, q].sum()) == int(total), q
        got = np.array([r[0] for r in merged[q]])
        assert len(got) == len(ref), (q, len(got), len(ref))
        assert np.allclose(got, ref["score"], rtol=parity.REL_TOL, atol=0), q


def case_wide_misled(L, layout, capfd, tiles=(8,)):
    """k_wide_pilot / k_wide_score.  by_terms([(q, 1), (2, 1), (3, 1)], 1) for q = 0, 1 on segments
    of 8 (9, 10) tiles of 12288 docs, configure(0, 4, 0): wide_stride = min(4, 8 / 2) = 4.  Term q
    holds 400 docs with tf 50 in each of the 2 tiles sampled for its unit (320 in each of 3: units 0
    and 4 of the 9- and 10-tile segments), terms 2 and 3 3000 docs with tf 1.  k = 1000: the pilot
    wants need = ceil(3 * 1000 * 2 / 8) = 750 docs at or above its bin (667 for 2 of 9 tiles, 900 for
    3 of 10) and finds 800 (960) hot ones; the full run lists those 800 < k of 800 + 4000 matches:
    one re-run, every unit short of k.  Three segments: units s * 2 + q with phases 0, 3, 2, 1, 0, 3,
    term 3 absent from the middle one; per segment against the oracle with index-global statistics,
    and the merged top k.  Control: the hot tiles two tiles (half a stride) further."""
    k, nq = 1000, 2
    filters = [by_terms([(q, 1.0), (2, 1.0), (3, 1.0)], 1) for q in range(nq)]
    with3 = None if len(tiles) == 1 else [s != 1 for s in range(len(tiles))]
    for shift, reruns in ((0, 1), (WIDE_STRIDE // 2, 0)):
        segs, readers = _tile_segments(L, layout, tiles, shift, k, nq, with3)
        stats = [parity.segment_stats(s) for s in segs]
        for scorer in SCORERS:
            prep = search.prepare(filters, scorer, stats)

            def check(res):
                _check_family(mt, segs, filters, scorer, k)(res)
                assert int(res[1].min()) == k and int(res[2].min()) > 3 * k
                if len(segs) > 1:
                    _check_wide_merged(segs, filters, scorer, k, res)
            _misled(_maker(readers, prep, k, WIDE_STRIDE), len(segs) > 1, check, _wide_counters, capfd,
                    reruns, [nq * len(segs)] * reruns, what=("wide", tiles, shift, scorer))
        _close(readers)


def _decoys(rng, tiles, per, free, tf=DECOY_TF):
    docs = np.concatenate([_in_tile(rng, t, per, free) for t in tiles]).astype(np.uint32)
    return docs, np.full(docs.size, tf, np.uint32)


def _spread(rng, free, n, max_tf):
    ids = np.nonzero(free)[0]
    d = np.sort(rng.choice(ids[ids > 0], n, replace=False)).astype(np.uint32)
    return d, rng.integers(1, max_tf + 1, d.size).astype(np.uint32)


def _masked_hot_segment(L, layout, k, masked_tf, seed=19, n_tiles=8):
    """case_wide_misled's lists of one 8-tile segment, with every hot doc of the sampled tiles in
    the segment's doc_mask (frequency `masked_tf`) and 400 live hot docs (tf 50) in every other
    tile.  Returns (seg, reader, the masked docs)."""
    rng = np.random.default_rng(seed)
    n_docs = n_tiles * TILE
    free = np.ones(n_docs + 1, bool)
    lists, gone = [], []
    for q in range(2):
        d, f = _hot(rng, n_tiles, q, 0, free, k, masked_tf)
        gone.append(d)
        live = np.concatenate([_in_tile(rng, t, 400, free) for t in range(n_tiles)
                               if t not in _sampled(q, n_tiles)]).astype(np.uint32)
        order = np.argsort(np.concatenate([d, live]))
        lists.append((np.concatenate([d, live])[order],
                      np.concatenate([f, np.full(live.size, HOT_TF, np.uint32)])[order]))
    lists += _cold_pair(rng, free)
    every = np.sort(np.concatenate([d for d, _ in lists[:2]])).astype(np.uint32)
    lists.append((every, np.ones(every.size, np.uint32)))
    seg = synth.segment_from_lists(lists, n_docs, layout, norms=False)
    gone = np.sort(np.concatenate(gone)).astype(np.uint32)
    seg.doc_mask = gone
    return seg, search.SegmentReader.from_synth(seg, L=L), gone


def _uncounted(readers, segs, filters, scorer, k, mod, capfd, what, gone=None, **prep_kw):
    """A control: the misleading stride does not re-run, the results are the stride-1 batch's and
    the oracle's; no doc of `gone` is returned."""
    prep = search.prepare(filters, scorer, [parity.segment_stats(s) for s in segs], **prep_kw)
    ref = _misled(_maker(readers, prep, k, WIDE_STRIDE), False, _check_family(mod, segs, filters, scorer, k),
                  _wide_counters, capfd, 0, what=what)
    if gone is not None:
        h, c, t = ref
        for q in range(len(filters)):
            assert not np.isin(h[0, q, :int(c[0, q])]["doc"], gone).any(), ("a deleted doc returned", what)
    return ref


def case_wide_uncounted(L, layout, capfd):
    """What k_wide_pilot must leave out of its histogram; configure(0, 4, 0) on 8 tiles, no re-run.
      * min_match = 2: by_terms([(0, 1), (2, 1), (3, 1), (4, 1)], 2).  Terms 0, 2, 3 hold 6000 random
        docs each (tf 1 .. 5): about 1050 docs in every tile alike hold two of them.  Term 4 holds
        1000 docs with tf 200 in each of tiles 0 and 4 (unit 0's sample) that hold no other term:
        they are no hits.  k = 200, need = ceil(3 * 200 * 2 / 8) = 150 <= the ~260 sampled matches.
        A pilot that counted the 2000 decoys would put its bin above every match: 0 < k listed.
      * deleted docs: case_wide_misled's lists, the 800 hot docs of the sampled tiles deleted, 400
        live hot docs (tf 50) in each of the 6 other tiles; k = 1000.  Once with the deleted docs at
        tf 50 as the lists of case 1 have them (2400 live docs then share their bin), once at tf 200:
        a bin of their own above every live doc, so that counting them lists 0 < k docs."""
    rng = np.random.default_rng(5)
    n_tiles, k = 8, 200
    free = np.ones(n_tiles * TILE + 1, bool)
    decoy = _decoys(rng, _sampled(0, n_tiles), 1000, free)
    real = [_spread(rng, free, 6000, 5) for _ in range(3)]      # (`free`: no decoy among them)
    unused = (np.array([1], np.uint32), np.array([1], np.uint32))   # term 1
    lists = [real[0], unused, real[1], real[2], decoy]
    seg =synth.segment_from_lists(lists, n_tiles * TILE, layout, norms=False)
    sr = search.SegmentReader.from_synth(seg, L=L)
    flt = by_terms([(0, 1.0), (2, 1.0), (3, 1.0), (4, 1.0)], 2)
    assert pilot_need(k, 2, n_tiles) == 150
    for scorer in SCORERS:
        sc, m = mt.expected(seg, flt, scorer)
        per_tile = [int(m[1 + t * TILE:1 + (t + 1) * TILE].sum()) for t in range(n_tiles)]
        assert not m[decoy[0]].any() and min(per_tile) > 100 and sum(per_tile) > 4 * k, per_tile
        _uncounted([sr], [seg], [flt], scorer, k, mt, capfd, ("wide, min_match", scorer))
    sr.close()
    k = 1000
    filters = [by_terms([(q, 1.0), (2, 1.0), (3, 1.0)], 1) for q in range(2)]
    for masked_tf in (HOT_TF, DECOY_TF):
        seg, sr, gone = _masked_hot_segment(L, layout, k, masked_tf)
        for scorer in SCORERS:
            ref = _uncounted([sr], [seg], filters, scorer, k, mt, capfd, ("wide, deleted", masked_tf, scorer), gone)
            live = [np.setdiff1d(np.union1d(np.union1d(_docs_of(seg, q), _docs_of(seg, 2)), _docs_of(seg, 3)), gone).size
                    for q in range(2)]
            assert [int(x) for x in ref[2][0]] == live, "the totals exclude the deleted docs"
        sr.close()


def _clause_filters():
    """The hot list as a clause of one (its score arrives in pass 1), and as a member of a clause of
    two with term 4, which holds every hot doc (pass 2)."""
    return [Or([by_term(q), And([by_term(2), by_term(3)])]) for q in range(2)] + \
           [Or([And([by_term(q), by_term(4)]), by_term(2)]) for q in range(2)]


def case_clause_misled(L, layout, capfd):
    """k_clause_pilot / k_clause_score, prepared with and_clauses=True; case_wide_misled's geometry
    (8 tiles, configure(0, 4, 0), 400 docs with tf 50 in each of the 2 tiles sampled for the unit).
    Two batches of two units: Or([q, And([2, 3])]) — terms 2 and 3 share 2000 docs, 2800 matches —
    and Or([And([q, 4]), 2]) with term 4 on every hot doc, 3800 matches.  k = 1000, need = ceil(3 *
    1000 * 2 / 8) = 750 <= 800 sampled hot docs < k: one re-run, both units short of k.  Control: the
    hot tiles half a stride further."""
    k = 1000
    flts = _clause_filters()
    for shift, reruns in ((0, 1), (WIDE_STRIDE // 2, 0)):
        segs, readers = _tile_segments(L, layout, (8,), shift, k)
        stats = [parity.segment_stats(segs[0])]
        for filters in (flts[:2], flts[2:]):
            for scorer in SCORERS:
                prep = search.prepare(filters, scorer, stats, and_clauses=True)

                def check(res):
                    _check_family(oc, segs, filters, scorer, k)(res)
                    assert int(res[1].min()) == k and int(res[2].min()) > 2 * k
                _misled(_maker(readers, prep, k, WIDE_STRIDE), False, check, _wide_counters, capfd, reruns,
                        [2] * reruns, what=("clause", filters[0], shift, scorer))
        _close(readers)


def case_clause_uncounted(L, layout, capfd):
    """What k_clause_pilot must leave out; 8 tiles, configure(0, 4, 0), k = 1000 (need 750), no
    re-run.  Term 5 holds 1000 docs with tf 200 in each of tiles 0 and 4 (unit 0's sample) and none
    of them holds another term of the segment.
      * Or([And([5, 4]), 2]): a decoy holds term 5 without term 4 — it completes no clause.  The
        matches are the 3000 docs of term 2.
      * Or([5, And([2, 3]), 2], min_match=2): a decoy completes exactly one clause; the 2000 docs
        that hold terms 2 and 3 complete two.
      * deleted hot docs, as in case_wide_uncounted, for both shapes of case_clause_misled.
    A pilot that counted the 2000 decoys (>= need) would put its bin above every match."""
    k = 1000
    rng = np.random.default_rng(23)
    n_tiles = 8
    free = np.ones(n_tiles * TILE + 1, bool)
    decoy = _decoys(rng, _sampled(0, n_tiles), 1000, free)
    lists = [_hot(rng, n_tiles, q, WIDE_STRIDE // 2, free, k) for q in range(2)]
    lists += _cold_pair(rng, free)
    every = np.sort(np.concatenate([d for d, _ in lists[:2]])).astype(np.uint32)
    lists += [(every, np.ones(every.size, np.uint32)), decoy]
    seg = synth.segment_from_lists(lists, n_tiles * TILE, layout, norms=False)
    sr = search.SegmentReader.from_synth(seg, L=L)
    controls = [Or([And([by_term(5), by_term(4)]), by_term(2)]),
                Or([by_term(5), And([by_term(2), by_term(3)]), by_term(2)], min_match=2)]
    for flt, n_match in zip(controls, (3000, 2000)):
        for scorer in SCORERS:
            sc, m = oc.expected(seg, flt, scorer)
            assert not m[decoy[0]].any() and int(m.sum()) == n_match
            _uncounted([sr], [seg], [flt], scorer, k, oc, capfd, ("clause", flt, scorer), and_clauses=True)
    sr.close()
    flts = _clause_filters()
    for masked_tf in (HOT_TF, DECOY_TF):
        seg, sr, gone = _masked_hot_segment(L, layout, k, masked_tf)
        for filters in (flts[:2], flts[2:]):
            _uncounted([sr], [seg], filters, SCORERS[0], k, oc, capfd, ("clause, deleted", masked_tf, filters[0]),
                       gone, and_clauses=True)
        sr.close()


def case_underflow_then_overflow(L, layout, capfd):
    """An underflow whose sound re-run overflows (wide).  case_wide_misled's hot lists (8 tiles,
    configure(0, 4, 0), k = 1000, need 750 <= 800 hot docs < k) and, as term 2, 20000 docs with tf 1
    (norms off: one score), apart from the hot docs and from term 3 (3000 docs, boost 0.25: below
    the ties).  The first run lists 800 of 23800 matches: underflow.  recover_now's buffer is
    default_cand_cap = max(4 * stride 4 * k, 16384) = 16384 slots; the sound bin is the ties', 20800
    candidates: overflow, recover_overflow sizes the next buffer from the count.  results() is OK,
    the 200 places behind the hot docs are the smallest tied doc ids, reruns() == 1 (recover_now
    counts, recover_overflow does not), and a later batch on the same reader runs.  (The stride-1
    reference gets 32768 candidate slots: with the default ones the ties overflow it too.)"""
    k = 1000
    rng = np.random.default_rng(31)
    n_tiles = 8
    free = np.ones(n_tiles * TILE + 1, bool)
    lists = [_hot(rng, n_tiles, q, 0, free, k) for q in range(2)]
    ids = np.nonzero(free)[0]
    pick = rng.choice(ids[ids > 0], 23000, replace=False)
    tied = np.sort(pick[:20000]).astype(np.uint32)
    low = np.sort(pick[20000:]).astype(np.uint32)
    assert tied.size > 16384
    lists += [(tied, np.ones(tied.size, np.uint32)), (low, np.ones(low.size, np.uint32))]
    seg = synth.segment_from_lists(lists, n_tiles * TILE, layout, norms=False)
    sr = search.SegmentReader.from_synth(seg, L=L)
    filters = [by_terms([(q, 1.0), (2, 1.0), (3, 0.25)], 1) for q in range(2)]
    stats = [parity.segment_stats(seg)]
    for scorer in SCORERS:
        prep = search.prepare(filters, scorer, stats)
        ref = _misled(_maker([sr], prep, k, WIDE_STRIDE, ref_cap=32768), False,
                      _check_family(mt, [seg], filters, scorer, k), _wide_counters, capfd, 1, [2],
                      listed=(800, 23800), what=("under, then over", scorer))
        h, c, t = ref
        for q in range(2):
            assert int(c[0, q]) == k and int(t[0, q]) == 23800
            assert set(h[0, q, :800]["doc"].tolist()) == set(lists[q][0].tolist())
            assert np.array_equal(h[0, q, 800:k]["doc"], tied[:k - 800]), "tie order: smallest doc ids first"
        later = sr.batch(prep, k)
        lh, lc, lt = later.run().results()
        _same((lh[None], lc[None], lt[None]), ref, what="a later batch")
        later.close()
    sr.close()


# ------------------------------------------------------- doc tiles: tree units --

def _tree_filters():
    """(q AND (4 OR 2)) OR (2 AND 3): the hot list under a nested Or, beside a clause of the cold pair."""
    return [Or([And([by_term(q), Or([by_term(4), by_term(2)])]), And([by_term(2), by_term(3)])]) for q in range(2)]


def _has(seg, term):
    m = np.zeros(seg.num_docs + 1, bool)
    if term < len(seg.metas):
        m[_docs_of(seg, term)] = True
    return m


def case_tree_misled(L, layout, capfd, tiles=(8,)):
    """k_tree_pilot / k_tree_score (prepare(boolean_trees=True); without the keyword prepare refuses the
    shape).  Or([And([q, Or([4, 2])]), And([2, 3])]) for q = 0, 1 on segments of 8 (9, 10) tiles of
    12288 docs without norms, configure(0, 4, 0): tree_stride = min(4, 8 tiles / 2) = 4.  Term q holds
    400 docs with tf 50 in each of the 2 tiles sampled for its unit s * 2 + q (320 in each of 3: unit 4,
    10 tiles, phase 0), term 4 every hot doc (tf 1), terms 2 and 3 3000 docs with tf 1, 2000 of them
    common.  k = 1000: the pilot wants need = ceil(3 * 1000 * 2 / 8) = 750 docs at or above its bin
    (667 for 2 of 9 tiles, 900 for 3 of 10) and finds the 800 (960) hot ones; the full run lists those
    800 (960) < k of 2800 (2960) matches — the hot docs plus the 2000 of `2 AND 3`: exactly one re-run,
    every unit short of k (`2 units short of k`).
    Three segments of 8, 9, 10 tiles: units with the phases 0, 3, 2, 1, 0, 3.  The middle segment has
    matches of its own and a leaf absent all the same: it lacks term 4, and its term 2 holds the hot docs
    too (tf 1) — they match through `q AND 2`, 800 + 2000 = 2800 per unit — so that all six phases show
    in the count: `6 units short of k`.  Per segment against the composed expectation with index-global
    statistics, and the merged top k as test_boolean_trees.case_multi has it.
    Control: the hot tiles two tiles (half a stride) further, no re-run."""
    k, nq = 1000, 2
    filters = _tree_filters()
    assert all(bt.refused(f) for f in filters)
    hot_in2 = None if len(tiles) == 1 else [s == 1 for s in range(len(tiles))]
    for shift, reruns in ((0, 1), (WIDE_STRIDE // 2, 0)):
        segs, readers = _tile_segments(L, layout, tiles, shift, k, nq, hot_in2=hot_in2)
        stats = [parity.segment_stats(s) for s in segs]
        for s, seg in enumerate(segs):       # the numbers above, from the lists alone
            n_tiles = tiles[s]
            assert (len(seg.metas) == 4) == bool(hot_in2 and hot_in2[s])
            both = _has(seg, 2) & _has(seg, 3)
            assert int(both.sum()) == 2000
            for q in range(nq):
                hot = _has(seg, q)
                sampled = _sampled(s * nq + q, n_tiles)
                n_hot = {2: 800, 3: 960}[len(_sampled(s * nq + q, n_tiles, shift))]     # (_hot)
                matched = (hot & (_has(seg, 4) | _has(seg, 2))) | both
                assert int(hot.sum()) == n_hot < k and not (hot & both).any()
                assert int(matched.sum()) == n_hot + 2000 > 2 * k
                in_sample = sum(int(hot[1 + t * TILE:1 + (t + 1) * TILE].sum()) for t in sampled)
                assert in_sample == (0 if shift else n_hot)
                assert shift or pilot_need(k, len(sampled), n_tiles) <= in_sample
        assert pilot_need(k, 2, 8) == 750 and pilot_need(k, 2, 9) == 667 and pilot_need(k, 3, 10) == 900
        for scorer in SCORERS:
            prep = search.prepare(filters, scorer, stats, boolean_trees=True)
            per = [[bt.expected(seg, flt, scorer, segs) for flt in filters] for seg in segs]

            def check(res):
                h, c, t = res
                for s in range(len(segs)):
                    for q, flt in enumerate(filters):
                        bt.check(flt, k, h[s, q], c[s, q], t[s, q], *per[s][q])
                assert int(c.min()) == k and int(t.min()) >= 2800
                if len(segs) > 1:
                    merged = search.merge_topk_host([(h[i], c[i]) for i in range(len(segs))], k)
                    for q in range(nq):
                        allsc = np.concatenate([per[i][q][0][per[i][q][1]] for i in range(len(segs))])
                        ref = np.sort(allsc)[::-1][:k]
                        assert int(t[:, q].sum()) == allsc.size, q
                        got = np.array([r[0] for r in merged[q]])
                        assert len(got) == len(ref) == k
                        assert np.allclose(got, ref, rtol=parity.REL_TOL, atol=0), q

            def counters(b):
                assert b.tree_units() == nq * len(segs)
                return _wide_counters(b)
            _misled(_maker(readers, prep, k, WIDE_STRIDE), len(segs) > 1, check, counters, capfd,
                    reruns, [nq * len(segs)] * reruns, listed=(800, 2800) if reruns else None,
                    what=("tree", tiles, shift, scorer))
        _close(readers)


def case_tree_uncounted(L, layout, capfd):
    """What k_tree_pilot must leave out of its histogram; configure(0, 4, 0) on 8 tiles, no re-run.
    Terms 0, 2, 3 hold 12000 random docs each (tf 1 .. 5): `0 AND (2 OR 3)`, the real branch R of every
    filter, matches about 340 docs in every tile alike.  500 decoys in EVERY tile (1000 in any unit's
    sample of 2 tiles) hold term 4 with tf 200 and terms 5 and 6 with tf 1, and no other term; term 1
    holds 100 other docs.  k = 200, need = ceil(3 * 200 * 2 / 8) = 150 <= the ~680 sampled matches.  One
    batch of four units (phases 0, 3, 2, 1):
      * Or([And([4, 1]), R]): a decoy holds a leaf of an And whose sibling is missing;
      * Or([And([4, Not(5)]), R]): a decoy is barred by a Not leaf;
      * Or([And([4, Not(And([5, 6]))]), R]): ... by a Not(And(...)) subtree;
      * Or([And([4, 1]), And([5, Or([6, 2])]), R]): a decoy is a hit through the cheap branch `5 AND 6`
        and holds the tf-200 leaf of a branch that does not match: leaf 4 must not score, in the
        histogram or in the result.
    Scored through term 4 a decoy lies above every real match, and 1000 of them >= need: a pilot that
    counted them so puts its bin above every match, 0 < k listed.
      * deleted docs: case_tree_misled's lists and filters, the 800 hot docs of the sampled tiles
        deleted (at tf 50, and at tf 200: a bin of their own above every live doc), 400 live hot docs
        (tf 50) in each of the 6 other tiles; k = 1000.  No deleted doc returned, totals without them."""
    rng = np.random.default_rng(5)
    n_tiles, k = 8, 200
    free = np.ones(n_tiles * TILE + 1, bool)
    decoy = _decoys(rng, range(n_tiles), 500, free)
    real = [_spread(rng, free, 12000, 5) for _ in range(3)]      # (`free`: no decoy among them)
    few = _spread(rng, free, 100, 1)
    for d, _ in real + [few]:
        assert not np.isin(d, decoy[0]).any()
    ones = (decoy[0], np.ones(decoy[0].size, np.uint32))
    lists = [real[0], few, real[1], real[2], decoy, ones, ones]
    seg = synth.segment_from_lists(lists, n_tiles * TILE, layout, norms=False)
    sr = search.SegmentReader.from_synth(seg, L=L)
    T = by_term
    R = And([T(0), Or([T(2), T(3)])])
    filters = [Or([And([T(4, 4.0), T(1)]), R]),
               Or([And([T(4, 4.0), Not(T(5))]), R]),
               Or([And([T(4, 4.0), Not(And([T(5), T(6)]))]), R]),
               Or([And([T(4, 4.0), T(1)]), And([T(5), Or([T(6), T(2)])]), R])]
    assert pilot_need(k, 2, n_tiles) == 150
    for scorer in SCORERS:
        lv = bt.Leaves(seg, scorer)
        as4 = lv(4, np.float32(4))[1][decoy[0]]          # what a decoy would score through term 4
        cheap = lv(5, np.float32(1))[1] + lv(6, np.float32(1))[1]
        for i, flt in enumerate(filters):
            sc, m = bt.expected(seg, flt, scorer)
            real_m = m.copy()
            real_m[decoy[0]] = False
            per_tile = [int(real_m[1 + t * TILE:1 + (t + 1) * TILE].sum()) for t in range(n_tiles)]
            assert 2 * min(per_tile) >= pilot_need(k, 2, n_tiles) and sum(per_tile) > 4 * k, per_tile
            assert as4.min() > sc[real_m].max(), "counted through term 4, the decoys lie above every real match"
            if i < 3:
                assert not m[decoy[0]].any()
            else:
                assert m[decoy[0]].all() and np.array_equal(sc[decoy[0]], cheap[decoy[0]])
                assert (sc[decoy[0]] < as4).all() and (sc[decoy[0]] > 0).all()
        _uncounted([sr], [seg], filters, scorer, k, bt, capfd, ("tree, decoys", scorer), boolean_trees=True)
    sr.close()
    k = 1000
    filters = _tree_filters()
    for masked_tf in (HOT_TF, DECOY_TF):
        seg, sr, gone = _masked_hot_segment(L, layout, k, masked_tf)
        both = _has(seg, 2) & _has(seg, 3)
        live = []
        for q in range(2):
            m = (_has(seg, q) & (_has(seg, 4) | _has(seg, 2))) | both
            m[gone] = False
            live.append(int(m.sum()))
        assert live == [2400 + 2000] * 2
        for scorer in SCORERS:
            ref = _uncounted([sr], [seg], filters, scorer, k, bt, capfd, ("tree, deleted", masked_tf, scorer), gone,
                             boolean_trees=True)
            assert [int(x) for x in ref[2][0]] == live, "the totals exclude the deleted docs"
            assert [int(x) for x in ref[1][0]] == [k, k]
        sr.close()


def case_tree_under_then_over(L, layout, capfd):
    """case_underflow_then_overflow on a tree filter.  case_tree_misled's hot lists and filters (8 tiles,
    configure(0, 4, 0), k = 1000, need 750 <= 800 hot docs < k); term 2 holds 20000 docs with tf 1
    (norms off: one score) apart from the hot docs, term 3 the same docs and 3000 more that hold
    nothing else (`2 AND 3`: the 20000, all tied), term 4 every hot doc.  The first run lists 800 of
    20800 matches: underflow.  recover_now's buffer is default_cand_cap = 16384 slots; the sound bin is
    the ties', 20800 candidates: overflow, recover_overflow sizes the next buffer from the count.
    results() is OK, the 200 places behind the hot docs are the smallest tied doc ids, reruns() == 1,
    and a later batch on the same reader runs.  (The stride-1 reference gets 32768 candidate slots.)"""
    k = 1000
    rng = np.random.default_rng(37)
    n_tiles = 8
    free = np.ones(n_tiles * TILE + 1, bool)
    lists = [_hot(rng, n_tiles, q, 0, free, k) for q in range(2)]
    ids = np.nonzero(free)[0]
    pick = rng.choice(ids[ids > 0], 23000, replace=False)
    tied = np.sort(pick[:20000]).astype(np.uint32)
    more = np.sort(pick).astype(np.uint32)
    every = np.sort(np.concatenate([d for d, _ in lists])).astype(np.uint32)
    assert tied.size > 16384 and every.size == 1600
    lists += [(tied, np.ones(tied.size, np.uint32)), (more, np.ones(more.size, np.uint32)),
              (every, np.ones(every.size, np.uint32))]
    seg = synth.segment_from_lists(lists, n_tiles * TILE, layout, norms=False)
    sr = search.SegmentReader.from_synth(seg, L=L)
    filters = _tree_filters()
    stats = [parity.segment_stats(seg)]
    for scorer in SCORERS:
        prep = search.prepare(filters, scorer, stats, boolean_trees=True)
        ref = _misled(_maker([sr], prep, k, WIDE_STRIDE, ref_cap=32768), False,
                      _check_family(bt, [seg], filters, scorer, k), _wide_counters, capfd, 1, [2],
                      listed=(800, 20800), what=("tree: under, then over", scorer))
        h, c, t = ref
        for q in range(2):
            assert int(c[0, q]) == k and int(t[0, q]) == 20800
            assert set(h[0, q, :800]["doc"].tolist()) == set(lists[q][0].tolist())
            assert np.array_equal(h[0, q, 800:k]["doc"], tied[:k - 800]), "tie order: smallest doc ids first"
        later = sr.batch(prep, k)
        lh, lc, lt = later.run().results()
        assert later.tree_units() == 2
        _same((lh[None], lc[None], lt[None]), ref, what="a later batch")
        later.close()
    sr.close()


# ------------------------------------------------------ lead items: k_conj_any --

def case_grouped_misled(L, layout, capfd, n_segs=1):
    """k_conj_any on _misled_conj_segments(L, layout, n_segs, 2, shift): leads 0 and 1 hold the docs
    2, 4, ... in 64 full blocks each, lead q with tf 50 in the blocks b % 16 == phase of its unit,
    terms 2 and 3 hold every doc.  And([Or([0, 1]), 2]) and And([Or([1, 0]), Or([2, 3])]): the lead
    group is the cheaper one (build_lead_groups: 2 * 8192 docs against 16484 and more), its items
    numbered member after member in row order, a member's blocks in order and then its tail
    (k_vphrase_seek) — here 0 .. 63 the first member's blocks, 64 .. 127 the second's, which owns no
    doc since the first holds them all.  Stride 16: the pilot samples 8 of 128 items, the 4 of the
    first member are hot: 512 docs >= need = ceil(3 * 1200 * 8 / 128) = 225.  The full run lists the
    1024 docs hot in either lead < k = 1200 of 8192 matches: one re-run, every unit short of k.
    Control: the hot blocks 8 further (shift 8)."""
    k, scorer, nq = 1200, TFIDF(False), 2
    filters = [And([Or([by_term(0), by_term(1)]), by_term(2)]),
               And([Or([by_term(1), by_term(0)]), Or([by_term(2), by_term(3)])])]
    assert pilot_need(k, 8, 128) == 225
    for shift, reruns in ((0, 1), (STRIDE // 2, 0)):
        segs, readers = _misled_conj_segments(L, layout, n_segs, nq, shift)
        prep = search.prepare(filters, scorer, [parity.segment_stats(s) for s in segs])
        assert all(any(p.alts) for p in prep)

        def check(res):
            h, c, t = res
            for s, seg in enumerate(segs):
                for q, flt in enumerate(filters):
                    nb.check(seg, flt, scorer, k, h[s, q], c[s, q], t[s, q], segs)
            assert (t == 8192).all() and (c == k).all()
        _misled(_maker(readers, prep, k, STRIDE), n_segs > 1, check, lambda b: b.path(), capfd, reruns,
                [nq * n_segs] * reruns, listed=(1024, 8192) if reruns else None, what=("grouped", n_segs, shift))
        _close(readers)


# ------------------------------------------------ lead items: k_phrase_and / _or --

def case_phrase_and_misled(L, layout, capfd):
    """k_phrase_and (required_terms=True) on _misled_phrase_segment: And([by_phrase([q, 2]), 3]) for
    q = 0, 1 (3 entries: the <4> instantiation), and the same with six required terms (8 entries:
    kPhraseMaxTerms).  The lead is lead q, the rarest entry: 64 items, stride 16 samples 4, all hot:
    512 docs with phrase frequency 50 >= need = ceil(3 * 1000 * 4 / 64) = 188, and < k = MISLED_K =
    1000 of 8192 matches: one re-run, both units short of k.  Control: shift 8."""
    k, scorer = MISLED_K, TFIDF(False)
    assert pilot_need(k, 4, 64) == 188
    batches = [[And([by_phrase([q, 2]), by_term(3)]) for q in range(2)],
               [And([by_phrase([q, 2])] + [by_term(t) for t in (3, 2, 3, 2, 3, 2)]) for q in range(2)]]
    for shift, reruns in ((0, 1), (STRIDE // 2, 0)):
        seg, sr = _misled_phrase_segment(L, layout, shift)
        for filters in batches:
            prep = search.prepare(filters, scorer, [parity.segment_stats(seg)], required_terms=True)

            def check(res):
                _check_family(pa, [seg], filters, scorer, k)(res)
                assert (res[2] == 8192).all()
            _misled(_maker([sr], prep, k, STRIDE), False, check, lambda b: b.path(), capfd, reruns, [2] * reruns,
                    listed=(512, 8192) if reruns else None, what=("phrase and", len(prep[0].terms), shift))
        sr.close()


OPT_TILE = 4096      # the term pass's doc tile in the two-pass constructions
OPT_TILES = 32       # ... and its tiles: stride_eff = min(16, 32 / 2) = 16
OPT_HOT, OPT_COLD = 300, 3000


def _two_pass_segment(L, layout, lead_blocks, phrase_shift, term_shift, masked=False):
    """32 tiles of 4096 docs.  Leads 0 and 1 hold the docs 2, 4, ... in `lead_blocks` full blocks
    (positions 1, 4, ...), term 2 one position behind every lead position: "q 2" has phrase frequency
    50 in the lead blocks b % 16 == phase of unit q + phrase_shift (None: 1 everywhere).  Term 3 + q,
    the optional term of query q, holds odd docs only (no phrase match among them): 300 with tf 60 in
    each of the two 4096-doc tiles k_pilot samples for unit q (+ term_shift), 3000 random ones with
    tf 1.  masked: the hot docs of both terms are deleted."""
    n_docs = OPT_TILE * OPT_TILES
    rng = np.random.default_rng(43)
    docs = 2 * np.arange(1, lead_blocks * 128 + 1, dtype=np.uint32)
    blk = np.arange(docs.size) // 128

    def pos_list(counts, first, step=3):
        return np.concatenate([first + step * np.arange(int(c), dtype=np.uint32) for c in counts])
    leads = []
    for q in range(2):
        hot = np.zeros(docs.size, bool) if phrase_shift is None else \
            blk % STRIDE == (pilot_phase(q) + phrase_shift) % STRIDE
        leads.append(np.where(hot, 50, 1).astype(np.uint32))
    lists = [(docs, tf, pos_list(tf, 1)) for tf in leads]
    both = np.maximum(leads[0], leads[1])
    lists.append((docs, both, pos_list(both, 2)))
    gone = []
    for q in range(2):
        first = (pilot_phase(q) + term_shift) % STRIDE
        hot = []
        for t in range(first, OPT_TILES, STRIDE):
            odd = 1 + t * OPT_TILE + 2 * np.arange(OPT_TILE // 2)
            hot.append(np.sort(rng.choice(odd, OPT_HOT, replace=False)))
        gone.append(np.concatenate(hot))
    rest = np.setdiff1d(1 + 2 * np.arange(n_docs // 2), np.concatenate(gone))
    for q in range(2):
        hot = gone[q]
        cold = rng.choice(rest, OPT_COLD, replace=False)
        d = np.concatenate([hot, cold])
        f = np.concatenate([np.full(hot.size, 60), np.ones(cold.size, np.int64)])
        order = np.argsort(d)
        d, f = d[order].astype(np.uint32), f[order].astype(np.uint32)
        lists.append((d, f, pos_list(f, 200, 1)))
    seg = synth.segment_from_lists(lists, n_docs, layout, norms=False)
    if masked:
        seg.doc_mask = np.sort(np.concatenate(gone)).astype(np.uint32)
    return seg, search.SegmentReader.from_synth(seg, L=L)


def _opt_filters():
    # (the boost puts even a cold doc of the optional term above every phrase-only doc: the merged
    # top k then holds docs that only the term pass's re-run lists)
    return [Or([by_phrase([q, 2]), by_term(3 + q, 16.0)]) for q in range(2)]


def case_phrase_or_misled(L, layout, capfd):
    """k_phrase_or, its term pass and k_union_topk (optional_terms=True); reruns() adds both passes.
      * phrase pass only, on _misled_phrase_segment: Or([by_phrase([q, 2]), 4]), stride 16, k =
        MISLED_K = 1000: the lead's 4 sampled items hold the 512 hot matches >= need = ceil(3 * 1000 *
        4 / 64) = 188 and < k of 8192.  Term 4 holds 128 odd docs, none a phrase match: the term pass
        lists them all (and, with 5 tiles of 4096, samples with stride 2: need = k, sound anyway).
        One re-run — it runs the term pass and the union again — and 8320 matches in the union.
      * term pass only, on _two_pass_segment: 4 cold lead blocks = 512 phrase matches < k, all listed.
        configure(4096, 16, 0): 32 tiles, the term pass's stride_eff = 16, k_pilot samples 2 tiles with
        the 600 hot docs of the unit's optional term >= need = ceil(3 * 1000 * 2 / 32) = 188, < k =
        1000 < 3600 matches.  One re-run, the term pass's: its line reports the term pass's own
        numbers, 600 of 3600 listed (the phrase pass has 512 of 512).  Only the union is made again,
        and the merged list shows whether it was: the 400 places behind the hot docs belong to cold
        docs of the optional term, which the failed term pass did not list.
      * both passes: 64 lead blocks, hot on phase, and the optional terms hot on phase: two re-runs.
    Controls: each hot part half a stride off; and the optional terms' hot docs on phase but deleted
    (k_pilot must not count them: they would put the bin above every live doc)."""
    k, scorer = MISLED_K, TFIDF(False)
    assert pilot_need(k, 4, 64) == 188 and pilot_need(k, 2, OPT_TILES) == 188
    counters = lambda b: b.path()
    for shift, reruns in ((0, 1), (STRIDE // 2, 0)):
        seg, sr = _misled_phrase_segment(L, layout, shift)
        filters = [Or([by_phrase([q, 2]), by_term(4)]) for q in range(2)]
        prep = search.prepare(filters, scorer, [parity.segment_stats(seg)], optional_terms=True)

        def check(res):
            _check_family(po, [seg], filters, scorer, k)(res)
            assert (res[2] == 8192 + 128).all()
        _misled(_maker([sr], prep, k, STRIDE), False, check, counters, capfd, reruns, [2] * reruns,
                listed=(512, 8192) if reruns else None, what=("phrase or: phrase pass", shift))
        sr.close()
    filters = _opt_filters()
    n_opt = 2 * OPT_HOT + OPT_COLD
    for blocks, p_shift, t_shift, masked, reruns, short, listed in (
            (4, None, 0, False, 1, [2], (2 * OPT_HOT, n_opt)),         # the term pass alone
            (4, None, STRIDE // 2, False, 0, [], None),                # ... its control
            (4, None, 0, True, 0, [], None),                           # ... deleted hot docs
            (64, 0, 0, False, 2, [2, 2], (512, 8192)),                 # both passes
            (64, STRIDE // 2, STRIDE // 2, False, 0, [], None)):       # ... their control
        seg, sr = _two_pass_segment(L, layout, blocks, p_shift, t_shift, masked)
        prep = search.prepare(filters, scorer, [parity.segment_stats(seg)], optional_terms=True)
        n_all = blocks * 128 + (OPT_COLD if masked else n_opt)

        def check(res):
            _check_family(po, [seg], filters, scorer, k)(res)
            h, c, t = res
            assert (t == n_all).all() and (c == k).all()
            if masked:
                assert not np.isin(h["doc"], seg.doc_mask).any()
        ref = _misled(_maker([sr], prep, k, STRIDE, OPT_TILE), False, check, counters, capfd, reruns, short,
                      listed=listed, what=("phrase or: two passes", blocks, p_shift, t_shift, masked))
        if blocks == 4 and not masked:
            # docs that hold the optional term only fill the list: 600 hot ones, then cold ones
            for q in range(2):
                assert np.isin(ref[0][0, q]["doc"], _docs_of(seg, 3 + q)).all()
        sr.close()


# ------------------------------------------------------------------ emulator --

@pytest.mark.parametrize("layout", LAYOUTS)
def test_wide_misled_emulated(simlib, layout, capfd):
    case_wide_misled(simlib, layout, capfd)


def test_wide_misled_segments_emulated(simlib, capfd):
    case_wide_misled(simlib, synth.LAYOUT_SIMD4, capfd, tiles=(8, 9, 10))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_wide_uncounted_emulated(simlib, layout, capfd):
    case_wide_uncounted(simlib, layout, capfd)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_clause_misled_emulated(simlib, layout, capfd):
    case_clause_misled(simlib, layout, capfd)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_clause_uncounted_emulated(simlib, layout, capfd):
    case_clause_uncounted(simlib, layout, capfd)


def test_underflow_then_overflow_emulated(simlib, capfd):
    case_underflow_then_overflow(simlib, synth.LAYOUT_SIMD4, capfd)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_tree_misled_emulated(simlib, layout, capfd):
    case_tree_misled(simlib, layout, capfd)


def test_tree_misled_segments_emulated(simlib, capfd):
    case_tree_misled(simlib, synth.LAYOUT_SIMD4, capfd, tiles=(8, 9, 10))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_tree_uncounted_emulated(simlib, layout, capfd):
    case_tree_uncounted(simlib, layout, capfd)


def test_tree_under_then_over_emulated(simlib, capfd):
    case_tree_under_then_over(simlib, synth.LAYOUT_SIMD4, capfd)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_grouped_misled_emulated(simlib, layout, capfd):
    case_grouped_misled(simlib, layout, capfd)


def test_grouped_misled_segments_emulated(simlib, capfd):
    case_grouped_misled(simlib, synth.LAYOUT_SIMD4, capfd, n_segs=3)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrase_and_misled_emulated(simlib, layout, capfd):
    case_phrase_and_misled(simlib, layout, capfd)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrase_or_misled_emulated(simlib, layout, capfd):
    case_phrase_or_misled(simlib, layout, capfd)


# ----------------------------------------------------------------------- GPU --

@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_wide_misled_gpu(gpulib, layout, capfd):
    case_wide_misled(gpulib, layout, capfd)


@pytest.mark.gpu
def test_wide_misled_segments_gpu(gpulib, capfd):
    case_wide_misled(gpulib, synth.LAYOUT_SIMD4, capfd, tiles=(8, 9, 10))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_wide_uncounted_gpu(gpulib, layout, capfd):
    case_wide_uncounted(gpulib, layout, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_clause_misled_gpu(gpulib, layout, capfd):
    case_clause_misled(gpulib, layout, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_clause_uncounted_gpu(gpulib, layout, capfd):
    case_clause_uncounted(gpulib, layout, capfd)


@pytest.mark.gpu
def test_underflow_then_overflow_gpu(gpulib, capfd):
    case_underflow_then_overflow(gpulib, synth.LAYOUT_SIMD4, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_tree_misled_gpu(gpulib, layout, capfd):
    case_tree_misled(gpulib, layout, capfd)


@pytest.mark.gpu
def test_tree_misled_segments_gpu(gpulib, capfd):
    case_tree_misled(gpulib, synth.LAYOUT_SIMD4, capfd, tiles=(8, 9, 10))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_tree_uncounted_gpu(gpulib, layout, capfd):
    case_tree_uncounted(gpulib, layout, capfd)


@pytest.mark.gpu
def test_tree_under_then_over_gpu(gpulib, capfd):
    case_tree_under_then_over(gpulib, synth.LAYOUT_SIMD4, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_grouped_misled_gpu(gpulib, layout, capfd):
    case_grouped_misled(gpulib, layout, capfd)


@pytest.mark.gpu
def test_grouped_misled_segments_gpu(gpulib, capfd):
    case_grouped_misled(gpulib, synth.LAYOUT_SIMD4, capfd, n_segs=3)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrase_and_misled_gpu(gpulib, layout, capfd):
    case_phrase_and_misled(gpulib, layout, capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrase_or_misled_gpu(gpulib, layout, capfd):
    case_phrase_or_misled(gpulib, layout, capfd)
