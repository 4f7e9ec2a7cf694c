"""GPU tier: parity of the HIP path with the oracle through the C ABI on a real
MI355X.  Integer/byte/index work is compared bit-exactly; scores within 1e-5
relative (BASELINE.json north_star)."""
import numpy as np
import pytest

import cases
import parity
from iresearch_amd import search, synth
from iresearch_amd.search import BM25, TFIDF, And, Or, by_phrase, by_term

pytestmark = pytest.mark.gpu
LAYOUTS = [synth.LAYOUT_SIMD4, synth.LAYOUT_SCALAR]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_reference_lists(gpulib, layout):
    cases.case_decode_reference_lists(gpulib, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_reference_packed(gpulib, layout):
    cases.case_decode_reference_packed(gpulib, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_sizes(gpulib, layout):
    cases.case_decode_sizes(gpulib, layout, sizes=(1, 2, 117, 127, 128, 129, 255, 256, 319, 1024,
                                                   10_000, 32_768))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_edge_blocks(gpulib, layout):
    cases.case_decode_edge_blocks(gpulib, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_synth(gpulib, layout):
    cases.case_decode_synth(gpulib, layout, 200_000, 1024)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_queries_all_scorers(gpulib, layout):
    cases.case_queries_all_scorers(gpulib, 300_000, 1024, layout)


def test_two_host_threads_share_a_segment(gpulib):
    """The threading contract of include/irs_hip.h: a segment is immutable after open and
    shared by threads; every thread owns its batches (index-search --threads)."""
    import threading
    seg = synth.build_segment(300_000, 512)
    sr = search.SegmentReader.from_synth(seg, L=gpulib)
    filters = cases.standard_filters(512)
    prep = search.prepare(filters, BM25(), [parity.segment_stats(seg)])
    ref = sr.batch(prep, 100).run().results()
    out, errs = {}, []

    def work(i):
        try:
            for _ in range(4):
                b = sr.batch(prep, 100)
                out[i] = b.run().results()
                b.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for i in range(4):
        for a, b in zip(out[i], ref):
            assert np.array_equal(a, b)
    sr.close()


def test_queries_k_extremes(gpulib):
    """top-1 and top-IRS_HIP_MAX_K, boolean and phrase queries."""
    from iresearch_amd import _lib
    seg = synth.build_segment(400_000, 1024, with_positions=True)
    sr = search.SegmentReader.from_synth(seg, L=gpulib)
    for k in (1, _lib.MAX_K):
        cases.run_and_check(gpulib, seg, cases.standard_filters(1024), BM25(), k, sr=sr)
        cases.run_phrases(gpulib, seg, [by_phrase([0, 1]), by_phrase([5, 2, 0])], BM25(), k, sr=sr)
    sr.close()


def test_queries_tiles_and_strides(gpulib):
    cases.case_queries_tiles_and_strides(gpulib, 200_000, 512)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_queries_ragged(gpulib, layout):
    cases.case_queries_ragged(gpulib, layout)


def test_no_norms(gpulib):
    cases.case_no_norms(gpulib)


@pytest.mark.parametrize("width", [2, 4])
def test_wide_norms(gpulib, width):
    cases.case_wide_norms(gpulib, width)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_without_freq(gpulib, layout):
    cases.case_decode_without_freq(gpulib, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_header_chain(gpulib, layout):
    cases.case_header_chain(gpulib, layout)


@pytest.mark.parametrize("layout", [0, 1])
def test_wand_data(gpulib, layout):
    cases.case_wand_data(gpulib, layout)


@pytest.mark.parametrize("layout", [0, 1])
def test_bit_union(gpulib, layout):
    cases.case_bit_union(gpulib, layout)
    cases.case_bit_union(gpulib, layout, has_freq=False)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_positions(gpulib, layout):
    cases.case_decode_positions(gpulib, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrase_queries(gpulib, layout):
    cases.case_phrase_queries(gpulib, layout, 200_000)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_phrase_reference_vectors(gpulib, layout):
    cases.case_phrase_reference_vectors(gpulib, layout)


def test_phrase_ragged(gpulib):
    cases.case_phrase_ragged(gpulib)
    cases.case_phrase_ragged(gpulib, synth.LAYOUT_SCALAR)
    cases.case_phrase_ragged(gpulib, synth.LAYOUT_SIMD4, one_based=True)


def test_phrase_fuzz(gpulib):
    cases.case_phrase_fuzz(gpulib, iters=60, seed=2)


def test_phrase_multi_segment(gpulib):
    cases.case_phrase_multi_segment(gpulib, sizes=(120_000, 5_000, 300_000))


def test_phrase_errors(gpulib):
    cases.case_phrase_errors(gpulib)


def test_reference_score_orders(gpulib):
    cases.case_reference_score_orders(gpulib)


def test_boolean_reference_vectors(gpulib):
    cases.case_boolean_reference_vectors(gpulib, max_doc=120_000_000)


def test_many_items(gpulib):
    cases.case_many_items(gpulib, 300_000)


@pytest.mark.parametrize("joined", [False, True])
def test_pilot_misled(gpulib, joined):
    cases.case_pilot_misled(gpulib, joined=joined)


def test_accumulator_switch(gpulib):
    cases.case_accumulator_switch(gpulib)


@pytest.mark.parametrize("layout", [0, 1])
def test_join_edge_blocks(gpulib, layout):
    cases.case_join_edge_blocks(gpulib, layout)


@pytest.mark.parametrize("layout", [0, 1])
def test_paths_agree(gpulib, layout):
    cases.case_paths_agree(gpulib, layout=layout)


@pytest.mark.parametrize("layout", [0, 1])
def test_paired_tiles(gpulib, layout):
    cases.case_paired_tiles(gpulib, layout=layout)



@pytest.mark.parametrize("layout", [0, 1])
def test_paired_ties(gpulib, layout):
    cases.case_paired_ties(gpulib, layout=layout)


@pytest.mark.parametrize("layout", [0, 1])
def test_paired_window(gpulib, layout):
    cases.case_paired_window(gpulib, layout=layout)


@pytest.mark.parametrize("layout", [0, 1])
def test_paired_ceiling(gpulib, layout):
    cases.case_paired_ceiling(gpulib, layout=layout)


@pytest.mark.parametrize("layout", [0, 1])
def test_paired_lookups(gpulib, layout):
    cases.case_paired_lookups(gpulib, layout=layout)


def test_paired_forms(gpulib):
    cases.case_paired_forms(gpulib)


def test_paired_overflow(gpulib):
    cases.case_paired_overflow(gpulib)


def test_paired_groups(gpulib):
    cases.case_paired_groups(gpulib, sizes=(400_000, 12_000, 900_000), max_rank=512)

def test_scored_multiterm_expansion(gpulib):
    """Prefix3 / Wildcard as the reference harness builds them (scored_terms_limit): VERDICT r05
    missing 5."""
    cases.case_scored_expansion(gpulib, sizes=(600_000, 250_000), max_rank=512)


@pytest.mark.parametrize("layout", [0, 1])
def test_conjunctions_with_a_sparse_lead(gpulib, layout):
    cases.case_conj_sparse_lead(gpulib, layout=layout, n_docs=2_000_000)


@pytest.mark.parametrize("layout", [0, 1])
def test_deleted_documents(gpulib, layout):
    """5 % random deletions (+ runs, ends, a whole term): totals, doc sets and top-k equal the
    oracle's masked run on every path."""
    cases.case_doc_mask(gpulib, layout=layout, num_docs=400_000, max_rank=512)


def test_join_counts(gpulib):
    cases.case_join_counts(gpulib, num_docs=900_000, max_rank=1024)


def test_join_counts_boundary(gpulib):
    cases.case_join_counts_boundary(gpulib)


def test_shared_threshold(gpulib):
    cases.case_shared_threshold(gpulib)
    cases.case_shared_threshold_misled(gpulib)


def test_multi_segment(gpulib):
    cases.case_multi_segment(gpulib, 600_000, 1024, n_segs=4, k=1000)


def test_multi_segment_batch(gpulib):
    cases.case_multi_segment_batch(gpulib, sizes=(700_000, 90_000, 1_300_000), max_rank=1024, k=1000)


def test_merge_ties(gpulib):
    cases.case_merge_ties(gpulib)
    cases.case_merge_ties(gpulib, n_lists=8, nq=5, k=1000, seed=5)
    # the documented limits: 16 lists x 2048 = kMergeMax staged scores (131 KB of dynamic LDS)
    cases.case_merge_ties(gpulib, n_lists=16, nq=3, k=2048, seed=16)
    cases.case_merge_ties(gpulib, n_lists=16, nq=2, k=2048, seed=17, single=9)
    cases.case_merge_ties(gpulib, n_lists=5, nq=7, k=63, seed=3)       # odd n_lists * k: `hp` moves a word
    cases.case_merge_ties(gpulib, n_lists=5, nq=4, k=63, seed=4, single=0)
    cases.case_merge_ties(gpulib, n_lists=8, nq=3, k=1000, seed=6, single=7)
    cases.case_merge_limits(gpulib)


def test_full_vocabulary_million_terms(gpulib):
    """A segment with the WHOLE vocabulary indexed (2^20 terms, ~890 k of them tail-only, ~100 k
    single-doc): open, then disjunctions / conjunctions over short lists, against the oracle."""
    rep = {}
    cases.case_full_vocabulary(gpulib, num_docs=300_000, max_rank=1 << 20, n_queries=200, report=rep)
    print("full vocabulary:", rep)
    assert rep["terms"] == 1 << 20 and rep["short"] > 800_000


def test_legacy_norms(gpulib):
    cases.case_legacy_norms(gpulib)


def test_zero_boost(gpulib):
    cases.case_zero_boost(gpulib)


def test_max_and_min_score_merging(gpulib):
    cases.case_merge_types(gpulib)


def test_min_score_pushdown(gpulib):
    cases.case_min_score_pushdown(gpulib)


def test_plan_ahead(gpulib):
    cases.case_plan_ahead(gpulib)


@pytest.mark.gpu
def test_host_results(gpulib):
    cases.case_host_results(gpulib)


@pytest.mark.gpu
def test_fresh_batches_and_trim(gpulib):
    cases.case_fresh_batches_and_trim(gpulib)


def test_wand_equals_exhaustive(gpulib):
    cases.case_wand_equals_exhaustive(gpulib, num_docs=400_000, max_rank=512, ks=(10, 1000))


def test_errors(gpulib):
    cases.case_errors(gpulib)


def test_create_status(gpulib):
    cases.case_create_status(gpulib)


def test_config1_by_term_top10_100k(gpulib):
    """BASELINE config 1: single by_term BM25 top-10 on a 100k-doc index."""
    from iresearch_amd import _lib
    seg = synth.build_segment(100_000, 256)
    cases.run_and_check(gpulib, seg, [by_term(63)], BM25(), 10, expect_path=_lib.PATH_ITEMS,
                        expect_paired=False)


def test_config2_or2_top100_1m(gpulib):
    """BASELINE config 2: OR-of-2 BM25 top-100, 1M docs, 1 segment."""
    seg = synth.build_segment(1_000_000, 4096)
    ranks = synth.make_queries(40, 2, 16, 4096, synth.SEED + 1)
    filters = [Or([by_term(int(r) - 1) for r in row]) for row in ranks]
    from iresearch_amd import _lib
    cases.run_and_check(gpulib, seg, filters, BM25(), 100, expect_path=_lib.PATH_ITEMS,
                        expect_paired=False)


def test_config3_or8_top1000_subset(gpulib):
    """BASELINE config 3 shape (OR-of-8, top-1000) at 2M docs against the oracle,
    plus run-to-run determinism."""
    seg = synth.build_segment(2_000_000, 4096)
    ranks = synth.make_queries(24, 8, 16, 4096)
    filters = [Or([by_term(int(r) - 1) for r in row]) for row in ranks]
    from iresearch_amd import _lib
    sr = search.SegmentReader.from_synth(seg, L=gpulib)
    h1, c1, t1 = cases.run_and_check(gpulib, seg, filters, BM25(), 1000, sr=sr,
                                     expect_path=_lib.PATH_ITEMS, expect_paired=False)
    h2, c2, t2 = cases.run_and_check(gpulib, seg, filters, BM25(), 1000, 8192, 4, sr=sr,
                                     expect_path=_lib.PATH_ITEMS, expect_paired=False)
    assert np.array_equal(h1, h2) and np.array_equal(c1, c2) and np.array_equal(t1, t2)
    sr.close()


def test_config5_and_phrase_tfidf_wand(gpulib):
    """BASELINE config 5 at its per-GPU size: one 6.25 M-doc segment of the 50 M-doc index
    (50 M docs over 8 GPUs) with positions; AND-of-2..4 and 2/3-word phrases scored by TF-IDF
    without norms (MaxFreq wand data, tfidf.cpp:364-386), against the oracle; and the same AND
    batch with block-max WAND pruning must return the exhaustive top k."""
    seg = synth.build_segment(6_250_000, 4096, with_positions=True)
    sr = search.SegmentReader.from_synth(seg, L=gpulib)
    ands = []
    for n in (2, 3, 4):
        for row in synth.make_queries(6, n, 16, 2048, synth.SEED + 5 + n):
            ands.append(And([by_term(int(r) - 1) for r in row]))
    from iresearch_amd import _lib
    h0, c0, t0 = cases.run_and_check(gpulib, seg, ands, TFIDF(False), 100, sr=sr,
                                     expect_path=_lib.PATH_ITEMS, expect_paired=False)
    prep = search.prepare(ands, TFIDF(False), [parity.segment_stats(seg)])
    wb = sr.batch(prep, 100).set_wand(True)
    h1, c1, t1 = wb.run().results()
    wb.close()
    assert np.array_equal(c0, c1) and (t1 <= t0).all()
    for q in range(len(ands)):
        assert np.array_equal(h0[q, :int(c0[q])], h1[q, :int(c0[q])]), q
    phrases = [by_phrase([int(r) - 1 for r in row])
               for row in synth.make_queries(24, 2, 4, 512, synth.SEED + 9)]
    phrases += [by_phrase([int(r) - 1 for r in row])
                for row in synth.make_queries(8, 3, 2, 64, synth.SEED + 10)]
    _, _, totals, _ = cases.run_phrases(gpulib, seg, phrases, TFIDF(False), 100, sr=sr)
    assert int(totals.sum()) > 0
    sr.close()


def test_config3_full_size_properties(gpulib):
    """BASELINE config 3/4 at FULL size (10 M docs, OR-of-8, top-1000), checked through
    size-independent properties plus the oracle on a few queries.  48 queries: the cost rule
    (join_or_pays) keeps a batch this small on work items (k_score), and the test pins that; the
    benchmark's 1000-query batch on the joined, paired kernels is test_config3_headline_batch:
      * order (score desc, doc asc), counts = min(k, hits);
      * hits of an OR query == popcount of irs_hip_bit_union over its terms (an independent
        kernel that never looks at frequencies or scores);
      * bitwise the same answer for another tile size / pilot stride;
      * the index cut into 8 segments (private doc ids, global statistics) and merged on the
        device gives the same top-k as the single segment, doc ids mapped back;
      * full oracle parity for the first 24 queries."""
    import ctypes

    import torch

    from iresearch_amd import _lib, distributed
    n_docs, n_segs, k, nq = 10_000_000, 8, 1000, 48
    seg = synth.build_segment(n_docs, 4096)
    ranks = synth.make_queries(nq, 8, 16, 4096, synth.SEED + 2)
    filters = [Or([by_term(int(r) - 1) for r in row]) for row in ranks]
    sr = search.SegmentReader.from_synth(seg, L=gpulib)
    st = [parity.segment_stats(seg)]
    prep = search.prepare(filters, BM25(), st)
    b = sr.batch(prep, k)
    hits, counts, totals = b.run().results()
    assert b.reruns() == 0 and b.path() == _lib.PATH_ITEMS
    b.close()
    n_words = (n_docs + 64) // 64
    for q in range(nq):
        n = int(counts[q])
        assert n == min(k, int(totals[q]))
        s, d = hits[q, :n]["score"], hits[q, :n]["doc"]
        assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (d[:-1] < d[1:]))).all(), q
        assert d.min() >= 1 and d.max() <= n_docs and len(set(d.tolist())) == n
    for q in range(0, nq, 6):
        bits, cnt = sr.bit_union([int(r) - 1 for r in ranks[q]], n_words)
        assert int(np.unpackbits(bits.view(np.uint8)).sum()) == int(totals[q]), q
        assert cnt == sum(int(seg.metas[int(r) - 1]["docs_count"]) for r in ranks[q])
    b2 = sr.batch(prep, k).configure(4096, 16, 0)
    h2, c2, t2 = b2.run().results()
    b2.close()
    assert np.array_equal(hits, h2) and np.array_equal(counts, c2) and np.array_equal(totals, t2)
    parity.check_single_segment(seg, filters[:24], BM25(), k, hits[:24], counts[:24], totals[:24])
    sr.close()

    per = n_docs // n_segs
    segs = [synth.build_segment(per, 4096, first_doc=i * per) for i in range(n_segs)]
    assert sum(s.docs_with_field for s in segs) == seg.docs_with_field
    assert sum(s.total_term_freq for s in segs) == seg.total_term_freq
    prep8 = search.prepare(filters, BM25(), [parity.segment_stats(s) for s in segs])
    ex = distributed.TopkExchange(gpulib, 0, n_segs, 0, 1, nq, k, "cuda")
    readers, batches = [], []
    tot8 = np.zeros(nq, np.uint64)
    for i, s in enumerate(segs):
        r = search.SegmentReader.from_synth(s, L=gpulib)
        bb = r.batch(prep8, k).run()
        hp, cp = ex.slot(i)
        bb.results_to_device(hp, cp)
        tot8 += bb.results()[2]
        readers.append(r)
        batches.append(bb)
    oh, osg, oc = ex.run()
    torch.cuda.synchronize()
    gh = distributed.hits_from_int64(oh)
    gs, gc = osg.cpu().numpy(), oc.cpu().numpy()
    assert np.array_equal(tot8, totals)
    for q in range(nq):
        n = int(counts[q])
        assert int(gc[q]) == n
        glob = gh[q, :n]["doc"].astype(np.int64) + gs[q, :n].astype(np.int64) * per
        # same statistics, same postings => the same per-posting scores; the fixed-point
        # scale follows each segment's own score bound, so sums agree to the tolerance and
        # docs may only differ where scores tie with the k-th one
        a = dict(zip(hits[q, :n]["doc"].astype(np.int64).tolist(), hits[q, :n]["score"].tolist()))
        m = dict(zip(glob.tolist(), gh[q, :n]["score"].tolist()))
        assert np.allclose(gh[q, :n]["score"], hits[q, :n]["score"], rtol=parity.REL_TOL, atol=0), q
        kth = float(hits[q, n - 1]["score"])
        for d in set(a) ^ set(m):
            sc = a.get(d, m.get(d))
            assert abs(sc - kth) <= 4 * parity.REL_TOL * kth, (q, d, sc, kth)
        for d in set(a) & set(m):
            assert abs(a[d] - m[d]) <= parity.REL_TOL * a[d], (q, d)
        assert len(set(a) & set(m)) >= n - 8, q
    for bb in batches:
        bb.close()
    for r in readers:
        r.close()



def test_config3_headline_batch(gpulib, monkeypatch):
    """BASELINE config 3 as bench.py runs it: the 10 M-doc segment, 1000 OR-8 queries of set 0
    (seed + 2), BM25, top-1000, prepared by prepare_disjunctions, PATH_AUTO — and the library's
    own rule for paired tiles (the suite's conftest forces pairs: IRS_HIP_JOIN_HALF is removed
    before the batch is created, Knobs::from_env reads it there).  The batch joins, pairs, needs
    no re-run; 48 queries spread over the batch, incl. those with the most and the fewest hits,
    against the oracle; the same prepared batch on 32-bit tiles and on work items: bit for bit.
    Then config 4's on-GPU half: the index as 8 segments in ONE batch with one threshold per
    query — pairs by the same rule, bit for bit unpaired, merged top k = the single segment's."""
    from iresearch_amd import _lib
    monkeypatch.delenv("IRS_HIP_JOIN_HALF", raising=False)
    n_docs, n_segs, k, nq = 10_000_000, 8, 1000, 1000
    seg = synth.build_segment(n_docs, 4096)
    ranks = synth.make_queries(nq, 8, 16, 4096, synth.SEED + 2)
    rows = ranks.astype(np.int64) - 1
    filters = [Or([by_term(int(t)) for t in row]) for row in rows]
    sr = search.SegmentReader.from_synth(seg, L=gpulib)
    arrays = search.prepare_disjunctions(rows, BM25(), [parity.segment_stats(seg)], [sr], k)
    b = sr.batch(arrays, k)
    hits, counts, totals = b.run().results()
    assert b.path() == _lib.PATH_JOINED and b.paired_tiles() and b.reruns() == 0
    b.close()
    for setup, path in ((lambda x: x.set_paired_tiles(0), _lib.PATH_JOINED),
                        (lambda x: x.set_path(_lib.PATH_ITEMS), _lib.PATH_ITEMS)):
        b2 = setup(sr.batch(arrays, k))
        h2, c2, t2 = b2.run().results()
        assert b2.path() == path and not b2.paired_tiles() and b2.reruns() == 0
        assert np.array_equal(counts, c2) and np.array_equal(totals, t2), path
        assert np.array_equal(hits, h2), path
        b2.close()
    pick = set(np.linspace(0, nq - 1, 46).astype(int).tolist())
    pick |= {int(np.argmax(totals)), int(np.argmin(totals))}
    pick = sorted(pick)
    assert len(pick) >= 48
    parity.check_single_segment(seg, [filters[q] for q in pick], BM25(), k, hits[pick], counts[pick],
                                totals[pick])
    sr.close()

    per = n_docs // n_segs
    segs = [synth.build_segment(per, 4096, first_doc=i * per) for i in range(n_segs)]
    readers = [search.SegmentReader.from_synth(s, L=gpulib) for s in segs]
    arrays8 = search.prepare_disjunctions(rows, BM25(), [parity.segment_stats(s) for s in segs], readers, k)
    got = []
    for mode in (1, 0):
        bb = search.QueryBatch(readers, arrays8).set_shared_threshold(True).set_paired_tiles(mode)
        got.append(bb.run().results())
        assert bb.path() == _lib.PATH_JOINED and bb.paired_tiles() == bool(mode) and bb.reruns() == 0
        bb.close()
    for x, y in zip(*got):
        assert np.array_equal(x, y)
    h8, c8, t8 = got[0]
    assert np.array_equal(t8.sum(axis=0), totals)
    merged = search.merge_topk_host([(h8[i], c8[i]) for i in range(n_segs)], k)
    for q in range(nq):
        n = int(counts[q])
        assert len(merged[q]) == n, q
        # (same per-posting scores; the fixed-point scale follows each segment's own bound, so sums
        # agree to the tolerance and docs may only differ where scores tie with the k-th one)
        a = dict(zip(hits[q, :n]["doc"].astype(np.int64).tolist(), hits[q, :n]["score"].tolist()))
        m = {d + s * per: sc for sc, s, d in merged[q]}
        assert np.allclose([sc for sc, _, _ in merged[q]], hits[q, :n]["score"], rtol=parity.REL_TOL, atol=0), q
        kth = float(hits[q, n - 1]["score"])
        for d in set(a) ^ set(m):
            assert abs(a.get(d, m.get(d)) - kth) <= 4 * parity.REL_TOL * kth, (q, d)
        assert len(set(a) & set(m)) >= n - 8, q
    for r in readers:
        r.close()

def test_config5_headline_batch(gpulib, monkeypatch, capfd):
    """BASELINE config 5 as bench.py --config 5 runs its set 0: 8 consecutive 6.25 M-doc segments
    with positions and MaxFreq wand data, 1000 AND-of-2..4 (WAND) and 1000 2-word phrases,
    TF-IDF without norms, k = 100, one QueryBatch over the 8 segments per class.  Prints the
    re-runs and the recovery IRS_HIP_TRACE names.  32 spread queries of each class against the
    oracle per segment and merged; WAND == exhaustive on all 1000 ANDs; a second fresh batch ==
    the first; term_blockmax of the longest list of a segment == its skip entries (tens of
    thousands: k_wand_skip0 re-stages its LDS window many times).  About 40 s on one MI355X."""
    import time

    import test_block_driven as bd
    from iresearch_amd import _lib
    t0 = time.perf_counter()
    n_segs, docs, nq, k = 8, 50_000_000, 1000, 100
    per = docs // n_segs
    # (the builder's output does not depend on its thread count)
    segs = [synth.build_segment(per if s < n_segs - 1 else docs - per * (n_segs - 1), 4096,
                                first_doc=s * per, with_positions=True, wand_count=1,
                                wand_kind=synth.WAND_MAX_FREQ, threads=16) for s in range(n_segs)]
    t_build = time.perf_counter() - t0
    readers = [search.SegmentReader.from_synth(s, L=gpulib) for s in segs]
    for sr in readers:
        assert sr.wand_source()[0] > 0
    stats = [parity.segment_stats(s) for s in segs]
    ands, phrases = bd.config5_queries(nq, nq, 16, 4096)
    assert len(ands) == nq and len(phrases) == nq
    sc = TFIDF(False)
    arrays = {name: search.QueryArrays.from_prepared(readers, search.prepare(fl, sc, stats), k)
              for name, fl in (("and", ands), ("phrase", phrases))}

    def run(name, wand):
        b = search.QueryBatch(readers, arrays[name])
        if wand:
            b.set_wand(True)
        b.profile(True)
        res = tuple(x.copy() for x in b.run().results())
        info = (b.reruns(), b.path())
        b.close()
        return res, info

    monkeypatch.setenv("IRS_HIP_TRACE", "1")
    capfd.readouterr()
    first = {name: run(name, name == "and") for name in ("and", "phrase")}
    trace = [ln for ln in capfd.readouterr().err.splitlines() if "[irs_hip] re-run:" in ln]
    monkeypatch.delenv("IRS_HIP_TRACE")
    second = {name: run(name, name == "and") for name in ("and", "phrase")}
    exh, exh_info = run("and", False)
    # (the cost rule joins the conjunctions of two frequent terms at this size: join_and_saving)
    assert first["and"][1][1] == _lib.PATH_JOINED and first["phrase"][1][1] == _lib.PATH_ITEMS
    # On fresh segments the AND batch overflows the default candidate cap (more than 16384 tied
    # candidates in some units) and re-runs once with a grown buffer; the second batch starts with
    # that size (cand_cap_hint).  The phrase batch needs no re-run.
    assert first["and"][1][0] == 1 and first["phrase"][1][0] == 0, (first["and"][1], first["phrase"][1])
    assert second["and"][1][0] == 0 and second["phrase"][1][0] == 0 and exh_info[0] == 0
    assert len(trace) == 1 and "re-run: status 2," in trace[0], trace
    for name in ("and", "phrase"):
        for x, y in zip(first[name][0], second[name][0]):
            assert np.array_equal(x, y), ("second fresh batch", name)
    h, c, t = first["and"][0]
    assert np.array_equal(h, exh[0]) and np.array_equal(c, exh[1]), "WAND != exhaustive"
    assert (t <= exh[2]).all()
    pick = np.linspace(0, nq - 1, 32).astype(int)
    for name, fl, res in (("and", ands, exh), ("phrase", phrases, first["phrase"][0])):
        hh, cc, tt = res
        sel = [fl[q] for q in pick]
        for s, seg in enumerate(segs):
            check = parity.check_single_segment if name == "and" else parity.check_phrase_segment
            check(seg, sel, sc, k, hh[s][pick], cc[s][pick], tt[s][pick], all_segs=segs)
        merged = search.merge_topk_host([(hh[s][pick], cc[s][pick]) for s in range(n_segs)], k)
        ref = (parity.oracle_topk(segs, sel, sc, k) if name == "and" else bd._phrase_topk(segs, sel, sc, k))
        bd._check_merged(merged, ref, name)
    longest = int(np.argmax(segs[0].metas["docs_count"]))
    entries = bd.check_skip_entries(readers[0], segs[0], longest)
    for r in readers:
        r.close()
    with capfd.disabled():
        print("\nconfig 5 headline: built in %.1f s, test %.1f s; AND (WAND) reruns %d path %d, phrase "
              "reruns %d path %d; second batches reruns %d / %d; exhaustive AND reruns %d; WAND left "
              "%d of %d hits unevaluated; longest list %d: %d skip entries"
              % (t_build, time.perf_counter() - t0, first["and"][1][0], first["and"][1][1],
                 first["phrase"][1][0], first["phrase"][1][1], second["and"][1][0], second["phrase"][1][0],
                 exh_info[0], int(exh[2].sum() - t.sum()), int(exh[2].sum()), longest, entries))
        for ln in trace:
            print(ln)


def test_rccl_behind_the_c_abi(gpulib):
    """irs_hip_comm_* / irs_hip_topk_allgather on the real GPU: librccl is bound at first use,
    a one-rank communicator is created from a fresh id and the all-gather moves the send
    buffer (multi-rank runs need several GPUs: the 2-rank flow is covered on the CPU tier)."""
    import torch

    from iresearch_amd import distributed
    comm = distributed.Communicator(gpulib, 0, 0, 1)
    send = torch.arange(1 << 16, dtype=torch.int64, device="cuda")
    recv = torch.zeros_like(send)
    comm.all_gather(send.data_ptr(), recv.data_ptr(), send.numel() * 8)
    torch.cuda.synchronize()
    assert torch.equal(send, recv)
    # ... and irs_hip_batch_set_comm: the batch's two all-reduces (ncclAllReduce inside the run,
    # between the pilot and the scoring kernels and behind the selection) on a one-rank
    # communicator leave the result what it is without them
    import numpy as np

    import parity
    from iresearch_amd import search, synth
    from iresearch_amd.search import BM25, Or, by_term
    segs = [synth.build_segment(n, 256, first_doc=f) for n, f in ((70_000, 0), (30_000, 70_000))]
    readers = [search.SegmentReader.from_synth(s, L=gpulib) for s in segs]
    ranks = synth.make_queries(16, 8, 12, 256, synth.SEED + 9)
    filters = [Or([by_term(int(r) - 1) for r in row]) for row in ranks]
    prep = search.prepare(filters, BM25(), [parity.segment_stats(s) for s in segs])
    from iresearch_amd import _lib
    # (joined streams, whatever the cost rule makes of this small batch: groups need them)
    plain = search.QueryBatch(readers, prep, 300).set_shared_threshold(True).set_path(_lib.PATH_JOINED)
    ph, pc, pt = plain.run().results()
    across = search.QueryBatch(readers, prep, 300).set_comm(comm).set_path(_lib.PATH_JOINED)
    ah, ac, at = across.run().results()
    assert across.reruns() == 0 and np.array_equal(pt, at)
    assert (search.merge_topk_host([(ph[i], pc[i]) for i in range(2)], 300)
            == search.merge_topk_host([(ah[i], ac[i]) for i in range(2)], 300))
    assert int(ac.sum()) < 2 * 16 * 300      # (the two segments shared the work)
    plain.close()
    across.close()
    for r in readers:
        r.close()
    comm.close()

