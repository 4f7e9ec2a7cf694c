"""k_join_score<kJKHalf> with its leaner requests and epilogue (join.h join_load4, the match count
of join_pairs): a group's request is the four slabs from its first on whatever its
size — a slab past the group's last is read and never used — and the epilogue counts matches with
plain 32-bit adds on two 16-bit counters.  Neither may move a reported figure.

The segment has 2 x 16320 + 7000 docs: three image tiles, so the last pair has a lone tile.
Lists: pieces of exactly 1, 2, 3, 4, 5 and 9 slabs (64 .. 576 postings) and the same counts - 1 and
+ 1, so that shares end in groups of 1, 2 and 3 slabs and start in the middle of a piece; a term
present only in the lone last tile; a term on every doc of the second tile (every lane of the
epilogue's partial fourth iteration counts); a term whose image ends in a
one-slab piece and is the only — so the last — image of its allocation when it is queried alone:
the three unused slabs of its last request lie in the slack behind it.  Queries of 1, 2, 8 and 16
terms; BM25 and TF-IDF with norms; k = 3, 100, 1000.  (The full-tile term is queried alone and in
a pair: among 16 terms under TF-IDF its small weight puts the query beyond what 32-bit accumulators
resolve, and the library deals such a query to its other kernels — test_join_slab_images.)

Every batch: paired against set_paired_tiles(0) bit for bit and against the oracle (hits, scores,
order, counts, totals), replayed; the same with the share split over 1, 4 and 16 wavefronts and
with chunks of 1 and 3 tiles; the same with the cache warm, off, and with a budget for the streams
only (private images).  The two new wave:: primitives (hip/wave_join.h, which carries its own plain
C++ forms) against one plain statement each, through tests/probe/lean_probe.hip as the emulator
compiles them and on the GPU.  One body per case, emulator and
GPU; under 300 k postings."""
from __future__ import annotations

import ctypes as C
import fcntl
import re
import shlex
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import cases
import parity
from iresearch_amd import _lib, search, synth
from iresearch_amd.search import BM25, TFIDF, Or, by_term
from test_join_slab_images import _Budget, _Env, _both, _decades, _run, _same

BT = 16320                      # docs per image tile (kJoinBoundTile)
TILE_DOCS = (BT, BT, 7000)
N_DOCS = sum(TILE_DOCS)
N_TILES = 3
SLAB = 64
SLABS = (1, 2, 3, 4, 5, 9)
PIECES = tuple(SLAB * s + d for s in SLABS for d in (-1, 0, 1))       # 63 .. 577
EDGE_TERMS = tuple(tuple(PIECES[3 * i + t] for t in range(N_TILES)) for i in range(len(SLABS)))
LAST = (65, 0, 1)               # two slabs, nothing, one slab: the image ends in a one-slab group
FULL = (0, BT, 0)


def _piece(rng, t, n):
    """n docs of image tile t, its first and its last doc among them (n >= 2)."""
    if n == 0:
        return np.zeros(0, np.int64)
    if n == 1:
        off = np.array([TILE_DOCS[t] - 1])
    else:
        inner = 1 + np.sort(rng.choice(TILE_DOCS[t] - 2, n - 2, replace=False))
        off = np.concatenate(([0], inner, [TILE_DOCS[t] - 1]))
    return 1 + t * BT + off


def _segment():
    rng = np.random.default_rng(2311)
    lists, terms, sizes = [], {}, []

    def add(name, per_tile):
        terms[name] = len(lists)
        d = np.concatenate([_piece(rng, t, n) for t, n in enumerate(per_tile)]).astype(np.uint32)
        lists.append((d, rng.integers(1, 4, d.size).astype(np.uint32)))
        sizes.append(sum(per_tile))

    for i, per_tile in enumerate(EDGE_TERMS):
        add(("edge", i), per_tile)
    add("lone", (0, 0, 900))
    add("full", FULL)
    add("last", LAST)
    add("big", (3000, 2500, 1500))
    for j in range(16):
        add(("or16", j), tuple(PIECES[(j + 5 * t) % len(PIECES)] for t in range(N_TILES)))
    seen = {n for i in range(len(SLABS)) for n in EDGE_TERMS[i]}
    assert seen == set(PIECES) and len(PIECES) == 18
    assert sum(sizes) < 300_000
    norms = rng.integers(40, 60, N_DOCS).astype(np.uint8)
    return lists, norms, terms, sizes


_SEGMENT = []


def _open(L):
    if not _SEGMENT:
        _SEGMENT.append(_segment())
    lists, norms, terms, sizes = _SEGMENT[0]
    seg, sr = cases.open_lists(L, lists, N_DOCS, synth.LAYOUT_SIMD4, norms=norms)
    return seg, sr, terms, sizes


def _filters(t):
    or16 = [t["or16", j] for j in range(16)]
    edges = [t["edge", i] for i in range(len(SLABS))]
    one = [by_term(j) for j in edges] + [by_term(t["lone"]), by_term(t["full"]), by_term(t["last"]),
                                         by_term(t["big"])]
    two = [Or([by_term(edges[0]), by_term(t["lone"])]), Or([by_term(t["last"]), by_term(edges[5])]),
           Or([by_term(t["full"]), by_term(edges[2])]),
           Or([by_term(t["big"], 5.0), by_term(edges[1], 0.2)])]
    eight = [Or([by_term(j) for j in or16[:8]]),
             Or([by_term(j, w) for j, w in zip(or16[8:], _decades(8))]),
             Or([by_term(j, w) for j, w in zip(edges + [t["lone"], t["last"]], reversed(_decades(8)))])]
    sixteen = [Or([by_term(j) for j in or16]),
               Or([by_term(j, w) for j, w in zip(or16, _decades(16, 0.5))]),
               Or([by_term(j, w) for j, w in zip(edges + [t["lone"], t["last"], t["big"]] + or16[:7],
                                                 reversed(_decades(16, 0.5)))])]
    return one + two + eight + sixteen


SCORERS = (BM25, lambda: TFIDF(True))
N_ONE = len(SLABS) + 4


def case_scorers(L):
    seg, sr, terms, sizes = _open(L)
    filters = _filters(terms)
    st = [parity.segment_stats(seg)]
    for make in SCORERS:
        scorer = make()
        prep = search.prepare(filters, scorer, st)
        for k in (3, 100, 1000):
            _, _, totals = _both(sr, prep, k, lambda h, c, t: parity.check_single_segment(
                seg, filters, scorer, k, h, c, t), (type(scorer).__name__, k))
            assert [int(x) for x in totals[:len(SLABS)]] == [sum(p) for p in EDGE_TERMS]
            assert [int(x) for x in totals[len(SLABS):N_ONE]] == [900, BT, sum(LAST), 7000]
    sr.close()


def case_last_image(L):
    """The term whose image ends in a one-slab piece, queried ALONE: its image is the only one of
    the batch, so the last of its cache slab (cold, warm) or of the batch's private buffer (cache
    off) — the three slabs its last request over-reads are the slack behind the allocation's
    images.  The same for the lone-tile term (one piece, in the last pair's only tile)."""
    seg, sr, terms, sizes = _open(L)
    st = [parity.segment_stats(seg)]
    for name, total in (("last", sum(LAST)), ("lone", 900)):
        filters = [by_term(terms[name])]
        for make in SCORERS:
            scorer = make()
            prep = search.prepare(filters, scorer, st)
            for budget in (64 << 20, 0):
                with _Budget(L, budget):
                    for k in (3, 100):
                        _, _, totals = _both(sr, prep, k, lambda h, c, t: parity.check_single_segment(
                            seg, filters, scorer, k, h, c, t), (name, type(scorer).__name__, k, budget))
                        assert int(totals[0]) == total
    sr.close()


def case_splits_and_chunks(L):
    """Share boundaries (the wavefronts a pair's slabs are dealt to) and chunk boundaries on every
    group size: the share split over 1, 4 and 16 wavefronts, chunks of 1 and 3 tiles — against
    results that were held to the 32-bit tiles and the oracle."""
    seg, sr, terms, sizes = _open(L)
    filters = _filters(terms)
    st = [parity.segment_stats(seg)]
    for make, k in ((BM25, 100), (lambda: TFIDF(True), 1000), (BM25, 3)):
        scorer = make()
        prep = search.prepare(filters, scorer, st)
        ref = _both(sr, prep, k, lambda h, c, t: parity.check_single_segment(
            seg, filters, scorer, k, h, c, t), ("default", k))
        for env in ({"IRS_HIP_JOIN_SPLIT_LOG2": 0}, {"IRS_HIP_JOIN_SPLIT_LOG2": 2},
                    {"IRS_HIP_JOIN_SPLIT_LOG2": 4}, {"IRS_HIP_JOIN_CHUNK": 1},
                    {"IRS_HIP_JOIN_CHUNK": 3, "IRS_HIP_JOIN_SPLIT_LOG2": 1}):
            with _Env(**env):
                b, out = _run(sr, prep, k)
            _same(ref, out, (env, k))
            _same(ref, b.run().results(), (env, k, "replayed"))
            b.close()
    sr.close()


def case_cache(L):
    """Where the images live: in cache slabs (cold, then warm), in the batch's private buffer
    (cache off; a budget that holds the streams and not the images) — the memory behind a
    request differs, the results may not."""
    seg, sr, terms, sizes = _open(L)
    filters = _filters(terms)
    used = sorted({s.term for f in filters for s in search._terms_of(f)[1]})
    n = len(used)
    st = [parity.segment_stats(seg)]
    for make, k in ((BM25, 100), (lambda: TFIDF(True), 3), (BM25, 1000)):
        scorer = make()
        prep = search.prepare(filters, scorer, st)
        check = lambda h, c, t: parity.check_single_segment(seg, filters, scorer, k, h, c, t)  # noqa: E731
        with _Budget(L, 64 << 20) as bud:
            search.set_stream_cache(0, L)                     # off
            ref = _both(sr, prep, k, check, ("off", k))
            search.set_stream_cache(bud.nbytes, L)
            b, out = _run(sr, prep, k, paired=False)          # the streams alone
            b.close()
            streams_only = search.stream_cache_stats(L)["bytes_held"]
            assert streams_only > 0 and search.cached_images(L) == 0
            for what in ("cold", "warm"):
                b, out = _run(sr, prep, k)
                _same(ref, out, (what, k))
                assert b.image_counts() == (n, n if what == "cold" else 0), what
                _same(ref, b.run().results(), (what, k, "replayed"))
                b.close()
            _lib.check(L, L.irs_hip_device_trim(0), "irs_hip_device_trim")
            b, out = _run(sr, prep, k, paired=False)
            b.close()
            search.set_stream_cache(streams_only, L)          # a budget for the streams only
            for what in ("tight", "tight, again"):
                b, out = _run(sr, prep, k)
                _same(ref, out, (what, k))
                assert b.stream_counts() == (n, 0) and b.image_counts() == (n, n), what
                _same(ref, b.run().results(), (what, k, "replayed"))
                b.close()
    sr.close()


CASES = (case_scorers, case_last_image, case_splits_and_chunks, case_cache)


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_lean_score_emulated(simlib, case):
    case(simlib)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__[5:])
def test_lean_score_gpu(gpulib, case):
    case(gpulib)


# ---- the two new wave:: primitives ------------------------------------------------------------

ROOT = Path(__file__).resolve().parents[1]
PROBE = ROOT / "tests" / "probe"
SRC = PROBE / "lean_probe.hip"
SIM_SO = PROBE / "liblean_probe_sim.so"
HIP_SO = PROBE / "liblean_probe_hip.so"
HIP_ASM = PROBE / "lean_probe_gfx950.s"
CSRC = ROOT / "iresearch_amd" / "csrc"


def _stale(target: Path, deps) -> bool:
    return not target.exists() or any(d.stat().st_mtime > target.stat().st_mtime for d in deps)


def _locked():
    lock = open(PROBE / ".build.lock", "w")
    fcntl.flock(lock, fcntl.LOCK_EX)   # (pytest-xdist workers: one builds, the others wait)
    return lock


def build_sim() -> Path:
    """The g++ line of tests/sim/build_sim.sh with the probe in place of the product source."""
    with _locked():
        deps = [SRC, CSRC / "types.h", CSRC / "hip" / "wave_join.h", ROOT / "tests" / "sim" / "sim_switch.S"] + \
            list((ROOT / "tests" / "sim").glob("*.h"))
        if _stale(SIM_SO, deps):
            text = (ROOT / "tests" / "sim" / "build_sim.sh").read_text().replace("\\\n", " ")
            line = [l for l in text.splitlines() if l.startswith("exec g++")]
            assert len(line) == 1, "build_sim.sh: one g++ line expected"
            cmd = shlex.split(line[0])[1:]
            assert "tests/sim/libirs_hip_sim.so" in cmd and "iresearch_amd/csrc/irs_hip.hip" in cmd
            cmd = [{"tests/sim/libirs_hip_sim.so": str(SIM_SO),
                    "iresearch_amd/csrc/irs_hip.hip": str(SRC)}.get(a, a) for a in cmd]
            subprocess.run(cmd, check=True, cwd=ROOT)
    return SIM_SO


def build_hip() -> Path:
    """hipcc for gfx950 with the flags of iresearch_amd/_build.py (cross-compiles without a GPU);
    the device assembly is kept next to the library."""
    from iresearch_amd import _build
    with _locked():
        deps = [SRC, CSRC / "types.h"] + list((CSRC / "hip").glob("*.h"))
        if _stale(HIP_SO, deps) or _stale(HIP_ASM, deps):
            hipcc = _build.hipcc_path()
            assert hipcc, "hipcc not found"
            with tempfile.TemporaryDirectory() as tmp:
                out = Path(tmp) / HIP_SO.name
                subprocess.run(
                    [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread",
                     "-ffp-contract=off", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function", "-save-temps=obj",
                     "-I", str(ROOT / "include"), "-I", str(CSRC), "-I", str(CSRC / "hip"),
                     "-o", str(out), str(SRC)], check=True, cwd=tmp)
                asm = list(Path(tmp).glob("*gfx950*.s"))
                assert len(asm) == 1, asm
                shutil.copyfile(asm[0], HIP_ASM)
                shutil.copyfile(out, HIP_SO)
    return HIP_SO


def _bind(path: Path):
    P = C.CDLL(str(path))
    u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
    for name, args in (("lp_arch", [C.c_char_p, C.c_size_t]), ("lp_halves_nc", [vp, u32, vp]),
                       ("lp_gload_imm", [vp, u64, vp, u32, vp])):
        fn = getattr(P, name)
        fn.argtypes, fn.restype = args, C.c_int
    return P


@pytest.fixture(scope="module")
def probe_sim():
    P = _bind(build_sim())
    buf = C.create_string_buffer(64)
    assert P.lp_arch(buf, 64) == 0 and buf.value == b"gfx950-sim"
    return P


@pytest.fixture(scope="module")
def probe_gpu():
    """The probe against iresearch_amd/csrc/hip on a real GPU; fails (does not skip) without one."""
    import torch  # noqa: F401  (one HIP runtime per process: iresearch_amd/_lib.py)
    P = _bind(build_hip())
    buf = C.create_string_buffer(64)
    assert P.lp_arch(buf, 64) == 0, "no usable HIP device"
    assert buf.value.decode().startswith("gfx950"), buf.value
    return P


def _ptr(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def halves_cases():
    """[5][n] = acc, a, b, c, d.  The domain of count_nonzero_halves4_nc: neither counter of acc
    overflows — counters up to 0xFFFB here, so that + 4 still fits."""
    rng = np.random.default_rng(77)
    n = 4096
    x = rng.integers(0, 2**32, (5, n), dtype=np.uint64)
    x[1, 1::4] &= np.uint64(0xFFFF)          # halves that are zero in some of the counted values
    x[2, 2::4] &= np.uint64(0xFFFF0000)
    x[3, 3::8] = 0
    x[4, ::16] = 0
    x[1:, 5::32] = 0                          # nothing to count
    x[1:, 6::32] |= np.uint64(0x00010001)     # everything counts
    lo, hi = x[0] & np.uint64(0xFFFF), x[0] >> np.uint64(16)
    lo, hi = np.minimum(lo, 0xFFFB), np.minimum(hi, 0xFFFB)
    lo[::7], hi[::11] = 0xFFFB, 0xFFFB        # the largest counters of the domain
    lo[::13], hi[::17] = 0, 0
    x[0] = lo | (hi << np.uint64(16))
    return np.ascontiguousarray(x.astype(np.uint32))


def state_halves(x):
    """acc's low counter += the values among a..d with a non-zero low half, its high counter += those
    with a non-zero high half."""
    v = x.astype(np.uint64)
    lo = (v[0] & np.uint64(0xFFFF)) + sum(((v[i] & np.uint64(0xFFFF)) != 0).astype(np.uint64) for i in range(1, 5))
    hi = (v[0] >> np.uint64(16)) + sum(((v[i] >> np.uint64(16)) != 0).astype(np.uint64) for i in range(1, 5))
    assert int(lo.max()) == 0xFFFF and int(hi.max()) == 0xFFFF      # (the domain's edge is among the cases)
    return (lo | (hi << np.uint64(16))).astype(np.uint32)


def check_halves(P):
    x = halves_cases()
    out = np.zeros(x.shape[1], np.uint32)
    assert P.lp_halves_nc(_ptr(x), x.shape[1], _ptr(out)) == 0
    want = state_halves(x)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, ("count_nonzero_halves4_nc", int(bad[0]), [hex(int(v)) for v in x[:, bad[0]]],
                           hex(int(out[bad[0]])), hex(int(want[bad[0]])))


IMMS = (0, 256, 512, 768, 4092)


def check_gload_imm(P):
    """gload_u32_imm<IMM>(base, off): the 4 bytes at base + off + IMM, little-endian."""
    rng = np.random.default_rng(78)
    nbytes = 1 << 20
    buf = rng.integers(0, 2**32, nbytes // 4, dtype=np.uint64).astype(np.uint32)
    top = nbytes - 4096
    offs = np.concatenate([np.arange(64) * 4, [top, top - 4, 252, 256, 260, 0xFFC, 0x1000, 0xFF00],
                           rng.integers(0, top // 4 + 1, 2000) * 4]).astype(np.uint32)
    out = np.zeros((offs.size, len(IMMS)), np.uint32)
    assert P.lp_gload_imm(_ptr(buf), nbytes, _ptr(offs), offs.size, _ptr(out)) == 0
    want = np.stack([buf[(offs.astype(np.int64) + imm) // 4] for imm in IMMS], axis=1)
    bad = np.argwhere(out != want)
    assert bad.size == 0, ("gload_u32_imm", IMMS[bad[0][1]], hex(int(offs[bad[0][0]])),
                           hex(int(out[tuple(bad[0])])), hex(int(want[tuple(bad[0])])))


def test_halves_nc_twin(probe_sim):
    check_halves(probe_sim)


@pytest.mark.gpu
def test_halves_nc_gpu(probe_gpu):
    check_halves(probe_gpu)


def test_gload_imm_twin(probe_sim):
    check_gload_imm(probe_sim)


@pytest.mark.gpu
def test_gload_imm_gpu(probe_gpu):
    check_gload_imm(probe_gpu)


def test_lean_probe_cross_compiles_in_the_promised_forms():
    """Compile only (no GPU): gload_u32_imm is ONE load in the saddr form with IMM in its offset
    field, count_nonzero_halves4_nc four packed minima and two three-operand adds."""
    build_hip()
    text = HIP_ASM.read_text()

    def body(name):
        m = re.search(r"^(_ZN5probe\w*%s\w*):.*?\n(.*?)s_endpgm" % name, text, re.M | re.S)
        assert m, name
        return "\n".join(l for l in m.group(2).splitlines() if not l.lstrip().startswith(";"))
    g = body("k_gload_imm")
    loads = re.findall(r"global_load_dword\s+v\d+, v\d+, s\[\d+:\d+\](?: offset:(\d+))?", g)
    assert sorted(int(o or 0) for o in loads) == sorted(IMMS), loads
    assert "flat_load" not in g
    h = body("k_halves_nc")
    assert len(re.findall(r"v_pk_min_u16", h)) == 4 and len(re.findall(r"v_add3_u32", h)) == 2
    assert "v_pk_add_u16" not in h
