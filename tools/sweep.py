#!/usr/bin/env python3
"""Dev utility: build the bench index once, then time several batch
configurations (tile size, pilot stride) back to back on one GPU.
  python tools/sweep.py --docs 10000000 --configs 8192:16,4096:16,16384:16,8192:64
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--configs", default="4096:16")
    ap.add_argument("--nocheck", action="store_true")
    ap.add_argument("--op", default="or", choices=["or", "and", "mm", "phrase", "terms", "tree"],
                    help="Or / And / Or(min_match=terms-1) / by_phrase of --terms consecutive words / "
                         "by_terms of --terms terms with --min-match (IRS_HIP_OP_MULTITERM, up to 64 terms) / "
                         "nested boolean trees over the --terms entries of every query (--shape)")
    ap.add_argument("--lo-rank", type=int, default=16)
    ap.add_argument("--hi-rank", type=int, default=4096)
    ap.add_argument("--terms", default="8",
                    help="terms per query; --op terms and --op or take a comma list (17,32,50,64): each is "
                         "timed on the same index, one line per count, then exits")
    ap.add_argument("--min-match", type=int, default=1, help="--op terms: by_terms_options::min_match")
    ap.add_argument("--shape", default="nest",
                    help="--op tree: comma list of SHAPEs over the --terms entries of every query "
                         "(IRS_HIP_TREE_NODE: k_tree_pilot / k_tree_score) — clause sizes as for --clauses "
                         "(2+2+2+2: an Or of Ands, sent as a tree), nest: an Or of (a AND (b OR (c AND d))) over "
                         "every four entries (depth 3), chain: a left-deep chain alternating And / Or over all "
                         "of them (--terms 16: 16 leaves, 15 nodes), not: nest with every d negated.  Times each "
                         "on the same entry lists (those of --op terms at the same --terms) and exits")
    ap.add_argument("--clauses", default="",
                    help="--op or: comma list of SPECs, each the clause sizes of an Or with And children over "
                         "the --terms entries of every query (IRS_HIP_CLAUSE_AND: k_clause_pilot / "
                         "k_clause_score) — 2+1+1 is one two-term clause and two single terms, 2x8 is eight "
                         "clauses of two; the sizes add up to --terms.  Times each on the same entry lists "
                         "(those of --op terms at the same --terms) and exits")
    ap.add_argument("--layout", type=int, default=1, help="0 = scalar (1_5), 1 = simd4 (1_5simd)")
    ap.add_argument("--scorer", default="bm25", choices=["bm25", "tfidf", "bm15"])
    ap.add_argument("--lib", default=None, help="alternative build of libirs_hip.so (A/B runs)")
    ap.add_argument("--wand", action="store_true", help="also time the batch with block-max pruning")
    ap.add_argument("--clustered", action="store_true", help="bursty posting lists (topic docs)")
    ap.add_argument("--path", default="auto", choices=["auto", "items", "joined"],
                    help="irs_hip_batch_set_path: work items / block-driven kernels, or joined streams "
                         "wherever a unit can take them")
    ap.add_argument("--touched", action="store_true",
                    help="And / by_phrase: one more run that counts the bytes actually decoded")
    ap.add_argument("--exclude", type=int, default=0,
                    help="And(query, Not(term)...): N excluded terms per query (IRS_HIP_EXCLUDE), drawn "
                         "from --lo-rank..--hi-rank; also times the plan stage without them (the "
                         "difference is k_excl_mask)")
    ap.add_argument("--alts", default="",
                    help="--op phrase: comma list N,...: every part but the first gets N members (the "
                         "word and N-1 ranks near it: a variadic phrase, IRS_HIP_PHRASE_ALT); 1 = the "
                         "plain phrase of the same words.  --op and: every term becomes an Or group of N "
                         "members from the same rank range (IRS_HIP_GROUP_ALT); 1 = the plain And.  "
                         "Times each and exits")
    ap.add_argument("--phrases", default="",
                    help="--op phrase: comma list N,...: And of N phrases (IRS_HIP_PHRASE_NEXT; 2..4 with "
                         "--terms 2) — every query's own phrase and those of the N-1 queries behind it; "
                         "1 = the plain phrases.  Times each and exits")
    ap.add_argument("--or-phrases", default="",
                    help="--op phrase: comma list N,...: Or of N phrases (IRS_HIP_PHRASE_OR; 2..4 with "
                         "--terms 2) — every query's own phrase and those of the N-1 queries behind it; "
                         "1 = the plain phrases, whose per-query times are the yardstick: the sum over a "
                         "query's phrases run alone.  Times each and exits")
    ap.add_argument("--required", default="",
                    help="--op phrase: comma list N,...: And([phrase, N by_terms]) — the same phrases with "
                         "N required terms each (IRS_HIP_PHRASE_REQUIRED), drawn from --lo-rank..--hi-rank; "
                         "0 = the plain phrases.  Times each and exits")
    ap.add_argument("--optional", default="",
                    help="--op phrase: comma list N,...: Or([phrase, N by_terms]) — the same phrases with "
                         "N optional terms each (IRS_HIP_PHRASE_OPTIONAL), drawn from --lo-rank..--hi-rank; "
                         "0 = the plain phrases.  Times each and exits")
    ap.add_argument("--unscored", action="store_true",
                    help="time irs_hip_batch_match_sets_to_device (every unit's full match set as a "
                         "bitset + its count, and the counts alone) instead of run + results; the scored "
                         "step of the same batch and, for --op or, irs_hip_bit_union_counts over the "
                         "same term sets are timed next to it; then exits")
    ap.add_argument("--score-docs", default="",
                    help="comma list N,...: time irs_hip_batch_score_docs_to_device for N docs per query — once "
                         "a uniform sample, once the run's own top N — beside the same batch's run "
                         "(--op or | and | mm | tree); then exits")
    ap.add_argument("--nested", default="",
                    help="comma list B,...: ByNestedFilter with the queries as the child filter and every "
                         "(B+1)-th doc a parent (B children per parent): times irs_hip_batch_nested_sets (rows + "
                         "counts), nested_sets_to_device and nested_topk under kMatchAny / SUM beside the same "
                         "batch's run (--op or | and); then exits")
    ap.add_argument("--doc-set", default="",
                    help="restrict every query to one doc set (irs_hip_batch_set_doc_sets): range:SHARE = a "
                         "contiguous doc range holding SHARE of the docs, random:SHARE = docs drawn uniformly, "
                         "none = unrestricted; a comma list times each on the same index, an entry may name "
                         "its own path (none@items: the unfiltered batch forced onto work items, the fair "
                         "comparison for --op or, whose restricted units leave the joined streams).  The "
                         "kernel times are those of profiled runs (HIP events around every stage); the skip "
                         "statistics printed next to them come from the timed runs (tiles) and from one more, "
                         "untimed counting run (lead pieces) (--op or | and | mm | phrase)")
    args = ap.parse_args()
    term_counts = [int(x) for x in str(args.terms).split(",")]
    args.terms = term_counts[0]
    if (args.op == "terms" or len(term_counts) > 1) and args.op not in ("terms", "or"):
        raise SystemExit("--terms takes a list with --op terms or --op or")
    import torch

    from iresearch_amd import _lib, search, synth
    from iresearch_amd.search import BM25, TFIDF, And, Not, Or, by_phrase, by_term, by_terms
    L = _lib.bind(ctypes.CDLL(args.lib)) if args.lib else _lib.lib()
    t0 = time.perf_counter()
    kw = dict(topic_docs=4096, topic_percent=85, topic_terms=12) if args.clustered else {}
    seg = synth.build_segment(args.docs, 4096, layout=args.layout,
                              with_positions=args.op == "phrase", **kw)
    t1 = time.perf_counter()
    sr = search.SegmentReader.from_synth(seg, L=L)
    print("index built in %.1f s, staged in %.2f s (%.0f MB .doc, %.0f MB .pos, %.0f MB in HBM)" % (
        t1 - t0, time.perf_counter() - t1, seg.doc_file.size / 1e6,
        0 if seg.pos_file is None else seg.pos_file.size / 1e6, sr.device_bytes() / 1e6),
        flush=True)
    ranks = synth.make_queries(args.queries, args.terms, args.lo_rank, args.hi_rank,
                               synth.SEED + 2)
    if args.op == "phrase":
        filters = [by_phrase([int(r) - 1 for r in row]) for row in ranks]
    elif args.op == "and":
        filters = [And([by_term(int(r) - 1) for r in row]) for row in ranks]
    elif args.op == "mm":
        filters = [Or([by_term(int(r) - 1) for r in row], min_match=args.terms - 1) for row in ranks]
    else:
        filters = [Or([by_term(int(r) - 1) for r in row]) for row in ranks]
    scorer = {"bm25": BM25(), "tfidf": TFIDF(True), "bm15": BM25(1.2, 0.0)}[args.scorer]
    st = search.SegmentStats(seg.docs_with_field, seg.total_term_freq,
                             np.asarray(seg.metas["docs_count"]))
    if args.score_docs:
        # irs_hip_batch_score_docs_to_device beside the same batch's run: per N, a uniform sample of N
        # docs per query and the run's own top N (sorted by doc); warm-up call, median of --steps
        if args.op not in ("or", "and", "mm", "tree") or len(term_counts) > 1:
            raise SystemExit("--score-docs goes with --op or | and | mm | tree and one --terms")
        counts = [int(x) for x in args.score_docs.split(",")]
        if min(counts) < 1 or max(counts) > _lib.MAX_K:
            raise SystemExit("--score-docs N: 1..%d" % _lib.MAX_K)
        flags = {}
        if args.op == "tree":   # --shape nest: an Or of (a AND (b OR (c AND d))) over every four entries
            if args.terms % 4:
                raise SystemExit("--op tree --score-docs: --terms is a multiple of 4")
            flags = {"boolean_trees": True}
            filters = []
            for row in ranks:
                lv = [by_term(int(r) - 1) for r in row]
                quads = [And([q[0], Or([q[1], And([q[2], q[3]])])]) for q in (lv[i:i + 4] for i in range(0, len(lv), 4))]
                filters.append(quads[0] if len(quads) == 1 else Or(quads))
        _, stride = (int(x) for x in args.configs.split(",")[0].split(":"))
        b = sr.batch(search.prepare(filters, scorer, [st], **flags), max(args.k, max(counts))).configure(0, stride, 0)
        b.set_async(False)   # (the whole run is queued when run() returns: a device synchronize times it)
        b.run()
        hits, cnt, totals = (x.copy() for x in b.results())
        steps = max(args.steps, 5)

        def median_ms(fn):
            fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(steps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ms)), float(np.min(ms))
        run_ms = median_ms(lambda: b.run())
        print("%s terms=%d  %d queries x %d docs  run (k=%d): median %.3f ms, min %.3f ms  hits/query mean %.0f" % (
            args.op, args.terms, len(filters), args.docs, b.k, *run_ms, float(np.mean(totals))), flush=True)
        rng = np.random.default_rng(synth.SEED + 6)
        for n in counts:
            lists = {"sample": [np.sort(rng.choice(args.docs, n, replace=False).astype(np.uint32) + 1) for _ in filters],
                     "top": [np.sort(hits[q, :min(n, int(cnt[q]))]["doc"].astype(np.uint32)) for q in range(len(filters))]}
            for name, per in lists.items():
                offs = np.concatenate([[0], np.cumsum([p.size for p in per])]).astype(np.uint64)
                flat = np.concatenate(per)
                d_docs = torch.from_numpy(flat.view(np.int32)).cuda()
                d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
                d_sc = torch.empty(flat.size, dtype=torch.float32, device="cuda")
                d_mt = torch.empty(flat.size, dtype=torch.uint8, device="cuda")
                ms = median_ms(lambda: b.score_docs_to_device(d_docs.data_ptr(), d_offs.data_ptr(), flat.size,
                                                             d_sc.data_ptr(), d_mt.data_ptr()))
                matched = int(d_mt.sum().item())
                if name == "top" and not args.nocheck:
                    assert matched == flat.size, "a hit of the run does not match"
                print("  score_docs N=%-5d %-6s  %8d docs  matched %8d  median %.3f ms, min %.3f ms  (run / call %.2f)" % (
                    n, name, flat.size, matched, *ms, run_ms[0] / ms[0]), flush=True)
        b.close()
        sys.exit(0)
    if args.nested:
        # the three nested calls beside the same batch's run: warm-up call, median of --steps; per B the
        # parents are the docs B + 1, 2 (B + 1), ...
        if args.op not in ("or", "and") or len(term_counts) > 1:
            raise SystemExit("--nested goes with --op or | and and one --terms")
        sizes = [int(x) for x in args.nested.split(",")]
        if min(sizes) < 1:
            raise SystemExit("--nested B: children per parent, 1 or more")
        _, stride = (int(x) for x in args.configs.split(",")[0].split(":"))
        b = sr.batch(search.prepare(filters, scorer, [st]), args.k).configure(0, stride, 0)
        b.set_async(False)   # (the whole run is queued when run() returns: a device synchronize times it)
        steps = max(args.steps, 5)

        def median_ms(fn):
            fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(steps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ms)), float(np.min(ms))
        run_ms = median_ms(lambda: b.run())
        print("%s terms=%d  %d queries x %d docs  run (k=%d): median %.3f ms, min %.3f ms" % (
            args.op, args.terms, len(filters), args.docs, b.k, *run_ms), flush=True)
        nw = b.match_words()
        d_sets = torch.empty((b.nq, nw), dtype=torch.int64, device="cuda")
        d_counts = torch.empty(b.nq, dtype=torch.int64, device="cuda")
        for bsz in sizes:
            par = np.zeros(64 * nw, bool)
            par[np.arange(bsz + 1, args.docs + 1, bsz + 1)] = True
            d_par = torch.from_numpy(np.packbits(par, bitorder="little").view(np.int64)).cuda()
            ptr = d_par.data_ptr()
            host = median_ms(lambda: b.nested_sets(ptr, n_words=nw))
            dev = median_ms(lambda: b.nested_sets_to_device(ptr, d_sets.data_ptr(), d_counts.data_ptr(), n_words=nw))
            top = median_ms(lambda: b.nested_topk(ptr, n_words=nw))
            totals = b.nested_topk(ptr, n_words=nw)[2]
            if not args.nocheck:
                assert np.array_equal(d_counts.cpu().numpy().astype(np.uint64), totals), "sets and top k disagree"
            print("  nested B=%-4d %8d parents  hits/query mean %.0f  sets %.3f / %.3f ms  sets_to_device %.3f / %.3f ms  "
                  "topk %.3f / %.3f ms  (median / min; run / topk %.2f)" % (
                      bsz, int(par.sum()), float(np.mean(totals)), *host, *dev, *top, run_ms[0] / top[0]), flush=True)
        b.close()
        sys.exit(0)
    if args.op == "tree":
        # one line per SHAPE: the rows of --op terms at the same --terms, put together as trees
        if len(term_counts) > 1 or not 2 <= args.terms <= 16:
            raise SystemExit("--op tree takes one --terms of 2..16")
        _, stride = (int(x) for x in args.configs.split(",")[0].split(":"))

        def tree_of(shape, row):
            leaves = [by_term(int(r) - 1) for r in row]
            if shape == "chain":
                node = And(leaves[:2])
                for i in range(2, len(leaves)):
                    node = (Or if i % 2 == 0 else And)([node, leaves[i]])
                return node
            if shape in ("nest", "not"):
                if len(leaves) % 4:
                    raise SystemExit("--shape %s: --terms is a multiple of 4" % shape)
                last = (lambda f: Not(f)) if shape == "not" else (lambda f: f)
                quads = [And([q[0], Or([q[1], And([q[2], last(q[3])])])])
                         for q in (leaves[i:i + 4] for i in range(0, len(leaves), 4))]
                return quads[0] if len(quads) == 1 else Or(quads)
            sizes = []
            for part in shape.split("+"):
                size, _, times = part.partition("x")
                sizes += [int(size)] * (int(times) if times else 1)
            if sum(sizes) != len(leaves) or min(sizes) < 1:
                raise SystemExit("--shape %s: the clause sizes add up to --terms %d" % (shape, len(leaves)))
            at, subs = 0, []
            for size in sizes:
                subs.append(leaves[at] if size == 1 else And(leaves[at:at + size]))
                at += size
            return Or(subs, min_match=args.min_match)

        for shape in args.shape.split(","):
            fl = [tree_of(shape, row) for row in ranks]
            b = sr.batch(search.prepare(fl, scorer, [st], boolean_trees=True), args.k).configure(0, stride, 0).profile(True)
            b.run()
            _, _, totals = b.results()
            ms = []
            t0 = time.perf_counter()
            for _ in range(args.steps):
                b.run()
                ms.append(b.timings())
            dt = (time.perf_counter() - t0) / args.steps
            avg = np.mean(ms, axis=0)
            alg, post = b.work()
            print("tree terms=%d shape=%s  tree units %d  step %.2f ms  plan %.2f pilot %.2f score %.2f "
                  "select %.2f  %.1f M postings  streams (distinct, decoded) %s  hits/query mean %.0f  reruns=%d" % (
                      args.terms, shape, b.tree_units(), dt * 1e3, *avg, post / 1e6,
                      b.stream_counts(), float(np.mean(totals)), b.reruns()), flush=True)
            b.close()
        sys.exit(0)
    if args.clauses:
        # one line per SPEC: the rows of --op terms at the same --terms, cut into clauses
        if args.op != "or" or len(term_counts) > 1:
            raise SystemExit("--clauses goes with --op or and one --terms")
        _, stride = (int(x) for x in args.configs.split(",")[0].split(":"))
        for spec in args.clauses.split(","):
            sizes = []
            for part in spec.split("+"):
                size, _, times = part.partition("x")
                sizes += [int(size)] * (int(times) if times else 1)
            if sum(sizes) != args.terms or min(sizes) < 1:
                raise SystemExit("--clauses %s: the clause sizes add up to --terms %d" % (spec, args.terms))
            fl = []
            for row in ranks:
                at, subs = 0, []
                for size in sizes:
                    members = [by_term(int(r) - 1) for r in row[at:at + size]]
                    subs.append(members[0] if size == 1 else And(members))
                    at += size
                fl.append(Or(subs, min_match=args.min_match))
            b = sr.batch(search.prepare(fl, scorer, [st], and_clauses=True), args.k).configure(0, stride, 0).profile(True)
            b.run()
            _, _, totals = b.results()
            ms = []
            t0 = time.perf_counter()
            for _ in range(args.steps):
                b.run()
                ms.append(b.timings())
            dt = (time.perf_counter() - t0) / args.steps
            avg = np.mean(ms, axis=0)
            alg, post = b.work()
            print("or terms=%d clauses=%s min_match=%d  clause units %d  step %.2f ms  plan %.2f pilot %.2f score %.2f "
                  "select %.2f  %.1f M postings  streams (distinct, decoded) %s  hits/query mean %.0f  reruns=%d" % (
                      args.terms, spec, args.min_match, b.clause_units(), dt * 1e3, *avg, post / 1e6,
                      b.stream_counts(), float(np.mean(totals)), b.reruns()), flush=True)
            b.close()
        sys.exit(0)
    if args.op == "terms" or len(term_counts) > 1:
        # one line per term count: by_terms on the wide kernels (k_wide_pilot / k_wide_score in the
        # pilot / score stages) or the Or of as many by_terms on the paths it takes today
        tile, stride = (int(x) for x in args.configs.split(",")[0].split(":"))
        paths = {"auto": _lib.PATH_AUTO, "items": _lib.PATH_ITEMS, "joined": _lib.PATH_JOINED}
        for n in term_counts:
            rows = synth.make_queries(args.queries, n, args.lo_rank, args.hi_rank, synth.SEED + 2)
            if args.op == "terms":
                fl = [by_terms([int(r) - 1 for r in row], min(args.min_match, n)) for row in rows]
            else:
                fl = [Or([by_term(int(r) - 1) for r in row]) for row in rows]
            b = sr.batch(search.prepare(fl, scorer, [st]), args.k).configure(0 if args.op == "terms" else tile, stride, 0)
            b.set_path(paths[args.path]).profile(True)
            b.run()
            _, _, totals = b.results()
            ms = []
            t0 = time.perf_counter()
            for _ in range(args.steps):
                b.run()
                ms.append(b.timings())
            dt = (time.perf_counter() - t0) / args.steps
            avg = np.mean(ms, axis=0)
            alg, post = b.work()
            print("%s terms=%d%s  %s  step %.2f ms  plan %.2f pilot %.2f score %.2f select %.2f  %.1f M postings  "
                  "streams (distinct, decoded) %s  hits/query mean %.0f  reruns=%d" % (
                      args.op, n, " min_match=%d" % min(args.min_match, n) if args.op == "terms" else "",
                      "wide units %d" % b.wide_units() if args.op == "terms" else
                      "path %s" % ("joined" if b.path() == _lib.PATH_JOINED else "items"),
                      dt * 1e3, *avg, post / 1e6, b.stream_counts(), float(np.mean(totals)), b.reruns()), flush=True)
            b.close()
        sys.exit(0)
    plain_prep = None
    if args.exclude:
        rng = np.random.default_rng(synth.SEED + 3)
        plain_prep = search.prepare(filters, scorer, [st])
        filters = [And([f] + [Not(by_term(int(r) - 1))
                              for r in rng.integers(args.lo_rank, args.hi_rank + 1, args.exclude)])
                   for f in filters]
    if args.alts and args.op == "and":
        for n_alt in (int(x) for x in args.alts.split(",")):
            rng = np.random.default_rng(synth.SEED + 4)
            gf = []
            for row in ranks:
                groups = []
                for r in row:
                    near = [int(r) - 1]
                    while len(near) < n_alt:
                        x = int(rng.integers(args.lo_rank, args.hi_rank + 1)) - 1
                        if x not in near:
                            near.append(x)
                    groups.append(Or([by_term(x) for x in near]) if n_alt > 1 else by_term(near[0]))
                gf.append(And(groups))
            b = sr.batch(search.prepare(gf, scorer, [st]), args.k).profile(True)
            b.run()
            _, _, totals = b.results()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                b.run()
                b.results()
            dt = (time.perf_counter() - t0) / args.steps
            print("alts=%d  %s  step %.2f ms  = %.2f ms per 1000 queries  hits/query mean %.0f  reruns=%d"
                  % (n_alt, "grouped" if n_alt > 1 else "plain", dt * 1e3, dt * 1e3 * 1000 / len(gf),
                     float(np.mean(totals)), b.reruns()), flush=True)
            b.close()
        sys.exit(0)
    if args.optional and args.op == "phrase":
        for n_opt in (int(x) for x in args.optional.split(",")):
            rng = np.random.default_rng(synth.SEED + 7)
            of = []
            for row in ranks:
                ph = by_phrase([int(r) - 1 for r in row])
                opt = []
                while len(opt) < n_opt:
                    x = int(rng.integers(args.lo_rank, args.hi_rank + 1)) - 1
                    if x not in opt:
                        opt.append(x)
                of.append(Or([ph] + [by_term(x) for x in opt]) if n_opt else ph)
            b = sr.batch(search.prepare(of, scorer, [st], optional_terms=True), args.k).profile(True)
            b.run()
            _, _, totals = b.results()
            ms = []
            t0 = time.perf_counter()
            for _ in range(args.steps):
                b.run()
                b.results()
                ms.append(b.timings())
            dt = (time.perf_counter() - t0) / args.steps
            avg = np.mean(ms, axis=0)
            # (the stage timings are the phrase pass's; the step holds both passes and the union)
            print("optional=%d  step %.2f ms  = %.2f ms per 1000 phrases  (phrase pass: plan %.2f pilot %.2f "
                  "score %.2f select %.2f)  hits/query mean %.1f  reruns=%d"
                  % (n_opt, dt * 1e3, dt * 1e3 * 1000 / len(of), *avg, float(np.mean(totals)), b.reruns()),
                  flush=True)
            b.close()
        sys.exit(0)
    if args.required and args.op == "phrase":
        for n_req in (int(x) for x in args.required.split(",")):
            rng = np.random.default_rng(synth.SEED + 6)
            rf = []
            for row in ranks:
                ph = by_phrase([int(r) - 1 for r in row])
                req = []
                while len(req) < n_req:
                    x = int(rng.integers(args.lo_rank, args.hi_rank + 1)) - 1
                    if x not in req:
                        req.append(x)
                rf.append(And([ph] + [by_term(x) for x in req]) if n_req else ph)
            b = sr.batch(search.prepare(rf, scorer, [st], required_terms=True), args.k).profile(True)
            b.run()
            _, _, totals = b.results()
            ms = []
            t0 = time.perf_counter()
            for _ in range(args.steps):
                b.run()
                b.results()
                ms.append(b.timings())
            dt = (time.perf_counter() - t0) / args.steps
            avg = np.mean(ms, axis=0)
            print("required=%d  step %.2f ms  = %.2f ms per 1000 phrases  (plan %.2f pilot %.2f score %.2f "
                  "select %.2f)  hits/query mean %.1f  reruns=%d"
                  % (n_req, dt * 1e3, dt * 1e3 * 1000 / len(rf), *avg, float(np.mean(totals)), b.reruns()),
                  flush=True)
            b.close()
        sys.exit(0)
    if args.phrases and args.op == "phrase":
        for n_ph in (int(x) for x in args.phrases.split(",")):
            # query q: its own phrase and those of the n_ph - 1 queries behind it, in one And
            pf = []
            for q in range(len(ranks)):
                phs = [by_phrase([int(r) - 1 for r in ranks[(q + j) % len(ranks)]]) for j in range(n_ph)]
                pf.append(And(phs) if n_ph > 1 else phs[0])
            b = sr.batch(search.prepare(pf, scorer, [st], phrase_conjunctions=True), args.k).profile(True)
            b.run()
            _, _, totals = b.results()
            ms = []
            t0 = time.perf_counter()
            for _ in range(args.steps):
                b.run()
                b.results()
                ms.append(b.timings())
            dt = (time.perf_counter() - t0) / args.steps
            avg = np.mean(ms, axis=0)
            print("phrases=%d  step %.2f ms  = %.2f ms per 1000 queries  (plan %.2f pilot %.2f score %.2f "
                  "select %.2f)  hits/query mean %.1f  reruns=%d  conj units %d"
                  % (n_ph, dt * 1e3, dt * 1e3 * 1000 / len(pf), *avg, float(np.mean(totals)), b.reruns(),
                     b.phrase_conj_units()), flush=True)
            b.close()
        sys.exit(0)
    if args.or_phrases and args.op == "phrase":
        from iresearch_amd.search import Or
        hits_alone = None
        for n_ph in (int(x) for x in args.or_phrases.split(",")):
            # query q: its own phrase and those of the n_ph - 1 queries behind it, in one Or
            pf = []
            for q in range(len(ranks)):
                phs = [by_phrase([int(r) - 1 for r in ranks[(q + j) % len(ranks)]]) for j in range(n_ph)]
                pf.append(Or(phs) if n_ph > 1 else phs[0])
            b = sr.batch(search.prepare(pf, scorer, [st], phrase_disjunctions=True), args.k).profile(True)
            b.run()
            _, _, totals = b.results()
            totals = np.asarray(totals, np.int64).reshape(-1)
            if n_ph == 1:
                hits_alone = totals
            ms = []
            t0 = time.perf_counter()
            for _ in range(args.steps):
                b.run()
                b.results()
                ms.append(b.timings())
            dt = (time.perf_counter() - t0) / args.steps
            avg = np.mean(ms, axis=0)
            shared = ""
            if hits_alone is not None and n_ph > 1:
                # the phrases' own hits minus the union's: a doc that p phrases match counts p - 1 times
                # (two phrases: the docs both match)
                alone = sum(np.roll(hits_alone, -j) for j in range(n_ph))
                shared = "  matches beyond a doc's first phrase: %d in all, in %d queries" % (
                    int((alone - totals).sum()), int(((alone - totals) > 0).sum()))
            print("or-phrases=%d  step %.2f ms  = %.2f ms per 1000 queries  (plan %.2f pilot %.2f score %.2f "
                  "select %.2f)  hits/query mean %.1f  reruns=%d  disj units %d%s"
                  % (n_ph, dt * 1e3, dt * 1e3 * 1000 / len(pf), *avg, float(np.mean(totals)), b.reruns(),
                     b.phrase_disj_units(), shared), flush=True)
            b.close()
        sys.exit(0)
    if args.alts and args.op == "phrase":
        for n_alt in (int(x) for x in args.alts.split(",")):
            rng = np.random.default_rng(synth.SEED + 4)
            vf = []
            for row in ranks:
                words = [int(r) - 1 for r in row]
                parts = [words[0]]
                for w in words[1:]:
                    near = [w]
                    while len(near) < n_alt:
                        x = int(np.clip(w + rng.integers(-8, 9), 0, 4095))
                        if x not in near:
                            near.append(x)
                    parts.append(sorted(near) if n_alt > 1 else w)
                vf.append(by_phrase(parts))
            b = sr.batch(search.prepare(vf, scorer, [st]), args.k).profile(True)
            b.run()
            _, _, totals = b.results()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                b.run()
                b.results()
            dt = (time.perf_counter() - t0) / args.steps
            print("alts=%d  %s  step %.2f ms  = %.2f ms per 1000 phrases  hits/query mean %.0f  reruns=%d"
                  % (n_alt, "variadic" if n_alt > 1 else "plain", dt * 1e3, dt * 1e3 * 1000 / len(vf),
                     float(np.mean(totals)), b.reruns()), flush=True)
            b.close()
        sys.exit(0)
    prep = search.prepare(filters, scorer, [st])
    if args.unscored:
        b = sr.batch(prep, args.k)
        nq, n_words = len(filters), b.match_words()
        ds = torch.empty((nq, n_words), dtype=torch.int64, device="cuda")
        dc = torch.empty((nq,), dtype=torch.int64, device="cuda")

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            out = []
            for _ in range(max(args.steps, 3)):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                out.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(out)), float(np.min(out))
        alg, post = b.work()
        # the bytes the match kernels decode: the DOC part of every full block of every entry (one
        # header byte + 16 bytes per bit of its widest delta, 2 bytes when all deltas are equal —
        # worked out from the decoded lists), 4 bytes per decoded tail doc; no frequency payload, no
        # norm.  (Phrases: what the conjunction of their terms would read in full — an upper bound,
        # the phrase kernels skip blocks without a lead doc.)
        doc_part = {}

        def doc_bytes(t):
            if t not in doc_part:
                d, _ = sr.decode_term(t, want_freq=False)
                d = d.astype(np.int64)
                nb = d.size // 128
                delta = np.diff(np.concatenate([[1], d[:nb * 128]])).reshape(nb, 128) if nb else np.zeros((0, 128), np.int64)
                if nb:   # (a block's first delta is relative to the last doc of the block before it)
                    delta[0, 0] = d[0] - 1
                bits = np.where(delta.max(axis=1) > 0, np.floor(np.log2(np.maximum(delta.max(axis=1), 1))) + 1, 0)
                same = (delta.max(axis=1) == delta.min(axis=1))
                doc_part[t] = int(np.where(same, 2, 1 + 16 * bits).sum()) + 4 * (d.size - nb * 128)
            return doc_part[t]
        terms_of = [sorted({int(r) - 1 for r in row}) if args.op == "or" else [int(r) - 1 for r in row]
                    for row in ranks]
        dbytes = sum(doc_bytes(t) for row in terms_of for t in row)
        both = timed(lambda: b.match_sets_to_device(ds.data_ptr(), n_words, dc.data_ptr()))
        only = timed(lambda: b.match_sets_to_device(None, n_words, dc.data_ptr()))
        counts = dc.cpu().numpy().view(np.uint64)
        scored = timed(lambda: b.run().results())
        _, _, totals = b.results()
        print("unscored %s x %d terms, %d queries, %d docs: sets + counts %.2f ms (min %.2f)  counts only "
              "%.2f ms (min %.2f)  = %.1f / %.1f GB/s over the %.1f MB of doc-block bytes of the entries (A(q) "
              "with frequency blocks and norms: %.1f MB)  %.1f MB of sets  counts == scored totals: %s" % (
                  args.op, args.terms, nq, args.docs, *both, *only, dbytes / both[0] / 1e6,
                  dbytes / only[0] / 1e6, dbytes / 1e6, alg / 1e6, nq * n_words * 8 / 1e6,
                  bool(np.array_equal(counts, totals))), flush=True)
        print("   scored step of the same batch (run + results, k = %d), for context: %.2f ms (min %.2f)  "
              "hits/query mean %.0f" % (args.k, *scored, float(np.mean(totals))), flush=True)
        if args.op == "or" and not args.exclude:
            sets = [np.unique(np.asarray([int(r) - 1 for r in row], np.uint32)) for row in ranks]
            base = timed(lambda: sr.bit_union_counts(sets))
            same = bool(np.array_equal(np.asarray(sr.bit_union_counts(sets), np.uint64), counts))
            print("   irs_hip_bit_union_counts over the same term sets: %.2f ms (min %.2f)  same counts: %s  "
                  "match sets / bit union: %.2fx (counts only %.2fx)" % (
                      *base, same, both[0] / base[0], only[0] / base[0]), flush=True)
        b.close()
        sys.exit(0)
    paths = {"auto": _lib.PATH_AUTO, "items": _lib.PATH_ITEMS, "joined": _lib.PATH_JOINED}

    def doc_set(spec):
        """u64[1][words] of `range:SHARE` / `random:SHARE`, or None."""
        if spec in ("", "none"):
            return None
        kind, share = spec.split(":")
        n = max(1, int(float(share) * args.docs))
        if kind == "range":
            lo = (args.docs - n) // 2 + 1
            docs = np.arange(lo, lo + n, dtype=np.int64)
        elif kind == "random":
            docs = np.random.default_rng(synth.SEED + 9).choice(args.docs, n, replace=False).astype(np.int64) + 1
        else:
            raise SystemExit("--doc-set: range:SHARE, random:SHARE or none")
        row = np.zeros((1, args.docs // 64 + 1), np.uint64)
        np.bitwise_or.at(row[0], docs // 64, np.uint64(1) << (docs % 64).astype(np.uint64))
        return row
    for spec in [x for x in args.doc_set.split(",") if x]:
        tile, stride = (int(x) for x in args.configs.split(",")[0].split(":"))
        what, _, own = spec.partition("@")
        row = doc_set(what)
        b = sr.batch(prep, args.k).configure(tile, stride, 0).set_path(paths[own or args.path]).profile(True)
        if row is not None:
            b.set_doc_sets(row, np.zeros(len(filters), np.uint32))
        b.run()
        _, _, totals = b.results()
        ms = []
        t0 = time.perf_counter()
        for _ in range(args.steps):
            b.run()
            ms.append(b.timings())
        dt = (time.perf_counter() - t0) / args.steps
        avg = np.mean(ms, axis=0)
        line = "doc-set %-14s path %-6s step %.2f ms  plan %.2f pilot %.2f score %.2f select %.2f  hits/query mean %.0f  reruns=%d" % (
            spec, "joined" if b.path() == _lib.PATH_JOINED else "items", dt * 1e3, *avg, float(np.mean(totals)), b.reruns())
        if row is not None:
            s = b.doc_set_stats()
            b.profile(3).run()   # (a counting run: the lead pieces)
            b.results()
            c = b.doc_set_stats()
            line += "  tiles %d skipped %d  leads %d skipped %d" % (s["tiles"], s["tiles_skipped"], c["leads"], c["leads_skipped"])
        print(line, flush=True)
        b.close()
    if args.doc_set:
        sys.exit(0)
    ref = None
    for cfg in args.configs.split(","):
        tile, stride = (int(x) for x in cfg.split(":"))
        path = paths[args.path]
        b = sr.batch(prep, args.k).configure(tile, stride, 0).set_path(path).profile(True)
        b.run()
        hits, counts, totals = b.results()
        print("   path: %s" % ("joined" if b.path() == _lib.PATH_JOINED else "items"), flush=True)
        if ref is None:
            ref = hits.copy()
        same = bool(np.array_equal(ref, hits))
        ms = []
        t0 = time.perf_counter()
        for _ in range(args.steps):
            b.run()
            ms.append(b.timings())
        dt = (time.perf_counter() - t0) / args.steps
        avg = np.mean(ms, axis=0)
        alg, post = b.work()
        print("tile=%d stride=%d  step %.2f ms  qps %.0f  plan %.2f pilot %.2f score %.2f select %.2f"
              "  score GB/s %.1f  same_hits=%s reruns=%d" % (tile, stride, dt * 1e3, args.queries / dt,
                                                              *avg, alg / avg[2] / 1e6, same,
                                                              b.reruns()), flush=True)
        print("   hits/query: mean %.0f max %d" % (float(np.mean(totals)), int(np.max(totals))),
              flush=True)
        if plain_prep is not None:
            pb = sr.batch(plain_prep, args.k).configure(tile, stride, 0).set_path(path).profile(True)
            pb.run()
            pb.results()
            pms = []
            for _ in range(args.steps):
                pb.run()
                pms.append(pb.timings())
            pavg = np.mean(pms, axis=0)
            print("   without the exclusions: plan %.3f ms (path %s)  ->  mask build ~%.3f ms for %d "
                  "masks" % (pavg[0], "joined" if pb.path() == _lib.PATH_JOINED else "items",
                             avg[0] - pavg[0], args.queries), flush=True)
            pb.close()
        if args.touched:
            b.profile(3).run()
            td, tp = b.touched()
            print("   touched: %.1f MB .doc + norms (%.1f%% of the terms' %.1f MB), %.1f MB positions; "
                  "%.1f GB/s of touched bytes" % (td / 1e6, 100.0 * td / max(1, alg), alg / 1e6,
                                                  tp / 1e6, (td + tp) / avg[2] / 1e6), flush=True)
        b.close()
        if args.wand:
            b = sr.batch(prep, args.k).configure(tile, stride, 0).set_wand(True).profile(True)
            b.run()
            whits, wcounts, wtotals = b.results()
            ms = []
            t0 = time.perf_counter()
            for _ in range(args.steps):
                b.run()
                ms.append(b.timings())
            dt = (time.perf_counter() - t0) / args.steps
            avg = np.mean(ms, axis=0)
            print("   WAND: step %.2f ms  plan %.2f pilot %.2f score %.2f select %.2f  same top-k=%s  "
                  "docs evaluated %.1f%% of the exhaustive run's hits" % (
                      dt * 1e3, *avg, bool(np.array_equal(whits, hits)),
                      100.0 * float(np.sum(wtotals)) / max(1.0, float(np.sum(totals)))), flush=True)
            b.close()


if __name__ == "__main__":
    main()
