"""The layer above the kernels: the few kernels EVERY execution path ends in, each launched
unmodified on operands of the test's own making and held to one plain statement in numpy
(uint64 / float64 / Python ints):

  k_select (kernels.h)                      the exact top k of a unit's candidate keys
  k_conj_threshold (conj.h),
  k_group_threshold (join.h)                the threshold bin b* out of a pilot histogram
  k_group_sums + k_group_verdict (join.h)   "fewer than k" for a group of units
  k_conj_hits (conj.h)                      a block-driven unit's hits, summed over its lead items
  k_union_topk (phrase.h)                   the union of the two passes of Or([by_phrase, by_term...])
  from_fixed, score_bin, bin_threshold (score.h)   the integer pre-filter in front of the float bins

through tests/probe/select_probe.hip, built the way the CPU emulator is built (g++, tests/sim:
test_*_twin) and for gfx950 (hipcc: test_*_gpu).  One case table per kernel, the same for both
builds; the one difference is named at BIG_TWIN below.  The constants (kBins, kMaxK,
kPilotMinSample, kPilotMargin, kSelectStage, the status bits) are read from the sources."""
from __future__ import annotations

import ctypes as C
import fcntl
import itertools
import re
import shlex
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
PROBE = ROOT / "tests" / "probe"
SRC = PROBE / "select_probe.hip"
SIM_SO = PROBE / "libselect_probe_sim.so"
HIP_SO = PROBE / "libselect_probe_hip.so"
CSRC = ROOT / "iresearch_amd" / "csrc"
HEADERS = ("kernels.h", "score.h", "join.h", "lead.h", "phrase.h", "conj.h", "types.h")

u32, u64, f32 = np.uint32, np.uint64, np.float32


def _const(name: str) -> int:
    """`NAME = <integer>u` of the kernel headers and batch.h (constexpr or enumerator)."""
    for h in HEADERS + ("batch.h",):
        m = re.search(r"\b%s\s*=\s*(\d+)u?\s*[;,]" % name, (CSRC / h).read_text())
        if m:
            return int(m.group(1))
    raise AssertionError(name)


K_BINS = _const("kBins")
MAX_K = _const("kMaxK")
MIN_SAMPLE = _const("kPilotMinSample")
MARGIN = _const("kPilotMargin")
SELECT_STAGE = _const("kSelectStage")
SUM_WORDS = _const("kGroupSumWords")
ST_CORRUPT, ST_OVER, ST_UNDER = _const("kStatusCorrupt"), _const("kStatusOverflow"), _const("kStatusUnderflow")
CAND_CAP, CAND_CAP_MAX = 16384, 262144       # default_cand_cap (batch.h): its floor and its ceiling
FILL32, FILL64 = 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE
NONE = 0xFFFFFFFF
# (the emulator runs the 262144-key launch at full size too: well under a second)
BIG_TWIN = CAND_CAP_MAX


def test_the_caps_are_the_products_rule():
    """What the tables take for the product's rule is still what run_select / default_cand_cap say."""
    run_h, batch_h = (CSRC / "run.h").read_text(), (CSRC / "batch.h").read_text()
    assert "uint32_t sort_cap = 64;\n  while (sort_cap < b->k_max) sort_cap <<= 1;" in run_h
    assert "stage_cap = std::min<uint32_t>(b->cand_cap, kSelectStage)" in run_h
    assert "size_t(sort_cap + stage_cap) * sizeof(uint64_t)" in run_h
    assert "{per_k * b->k_max, %d, learned}), %d)" % (CAND_CAP, CAND_CAP_MAX) in batch_h
    assert (K_BINS, MAX_K, SELECT_STAGE) == (512, 4096, 8192) and MIN_SAMPLE < MAX_K and MARGIN > 0


# ---- the two builds ------------------------------------------------------------------------------

def _stale(target: Path, deps) -> bool:
    return not target.exists() or any(d.stat().st_mtime > target.stat().st_mtime for d in deps)


def _locked():
    lock = open(PROBE / ".build.lock", "w")
    fcntl.flock(lock, fcntl.LOCK_EX)   # (pytest-xdist workers: one builds, the others wait)
    return lock


def _deps(hip_dir: Path):
    return [SRC] + [CSRC / h for h in HEADERS] + [CSRC / "hip" / "wave_join.h"] + list(hip_dir.glob("*.h"))


def build_sim() -> Path:
    """The g++ line of tests/sim/build_sim.sh with the probe in place of the product source."""
    with _locked():
        sim = ROOT / "tests" / "sim"
        if _stale(SIM_SO, _deps(CSRC / "hip") + [sim / "sim_switch.S"] + list(sim.glob("*.h"))):
            text = (sim / "build_sim.sh").read_text().replace("\\\n", " ")
            line = [l for l in text.splitlines() if l.startswith("exec g++")]
            assert len(line) == 1, "build_sim.sh: one g++ line expected"
            cmd = shlex.split(line[0])[1:]
            assert "tests/sim/libirs_hip_sim.so" in cmd and "iresearch_amd/csrc/irs_hip.hip" in cmd
            cmd = [{"tests/sim/libirs_hip_sim.so": str(SIM_SO),
                    "iresearch_amd/csrc/irs_hip.hip": str(SRC)}.get(a, a) for a in cmd]
            subprocess.run(cmd, check=True, cwd=ROOT)
    return SIM_SO


def build_hip() -> Path:
    """hipcc for gfx950 with the flags of iresearch_amd/_build.py (cross-compiles without a GPU)."""
    from iresearch_amd import _build
    with _locked():
        if _stale(HIP_SO, _deps(CSRC / "hip")):
            hipcc = _build.hipcc_path()
            assert hipcc, "hipcc not found"
            with tempfile.TemporaryDirectory() as tmp:
                out = Path(tmp) / HIP_SO.name
                subprocess.run(
                    [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread",
                     "-ffp-contract=off", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
                     "-I", str(ROOT / "include"), "-I", str(CSRC), "-I", str(CSRC / "hip"),
                     "-o", str(out), str(SRC)], check=True, cwd=tmp)
                shutil.copyfile(out, HIP_SO)
    return HIP_SO


def _bind(path: Path):
    P = C.CDLL(str(path))
    i, vp = C.c_uint32, C.c_void_p
    for name, args in (
            ("sp_arch", [C.c_char_p, C.c_size_t]),
            ("sp_select", [vp, i, i, vp, vp, vp, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp]),
            ("sp_union", [vp, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
            ("sp_conj_threshold", [vp, i, vp, vp, i, vp, i, i, vp, vp]),
            ("sp_group_threshold", [vp, i, vp, i, i, vp, i, vp, vp]),
            ("sp_group_verdict", [vp, i, vp, i, i, vp, vp, vp, vp, vp, vp]),
            ("sp_conj_hits", [vp, vp, vp, i, i, i, vp]),
            ("sp_bins", [vp, vp, vp, vp, i, C.c_int, vp, vp, vp])):
        fn = getattr(P, name)
        fn.argtypes, fn.restype = args, C.c_int
    return P


@pytest.fixture(scope="module")
def probe_sim():
    P = _bind(build_sim())
    buf = C.create_string_buffer(64)
    assert P.sp_arch(buf, 64) == 0 and buf.value == b"gfx950-sim"
    return P


@pytest.fixture(scope="module")
def probe_gpu():
    """The probe against the product headers on a real GPU; fails (does not skip) without one."""
    import torch  # noqa: F401  (one HIP runtime per process: iresearch_amd/_lib.py)
    P = _bind(build_hip())
    buf = C.create_string_buffer(64)
    assert P.sp_arch(buf, 64) == 0, "no usable HIP device"
    assert buf.value.decode().startswith("gfx950"), buf.value
    return P


def test_select_probe_cross_compiles():
    """Compile only (no GPU): the gfx950 build of the probe, so that the GPU tier finds it built."""
    assert build_hip().exists()


def _a(x, dtype):
    return np.ascontiguousarray(np.asarray(x, dtype=dtype))


def _p(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


# ---- keys ----------------------------------------------------------------------------------------

def make_keys(scores, docs):
    """types.h make_key: descending key order == (score descending, doc ascending)."""
    bits = _a(scores, f32).view(u32).astype(u64)
    return (bits << u64(32)) | (u64(NONE) - _a(docs, u64))


def hits_of(keys):
    """types.h key_hit as two 32-bit words per hit: the score's bits, the doc."""
    keys = _a(keys, u64)
    return np.stack([(keys >> u64(32)).astype(u32), (u64(NONE) - (keys & u64(NONE))).astype(u32)], axis=-1)


def scores_of(keys):
    return (_a(keys, u64) >> u64(32)).astype(u32).view(f32)


def docs_for(rng, n):
    """n distinct docs in 1 .. 2^32 - 2, in random order."""
    return rng.permutation(n).astype(u64) * u64(16381) + u64(1 + int(rng.integers(0, 700)))


def random_keys(rng, n, top=100.0):
    return make_keys((rng.random(n) * top + 1e-3).astype(f32), docs_for(rng, n))


def sort_cap_of(k_max):
    cap = 64
    while cap < k_max:
        cap <<= 1
    return cap


class Row:
    """One query of a k_select launch.  `count` defaults to the keys given; `hits` to what is listed."""

    def __init__(self, name, keys, k, count=None, hits=None, pruned=0, bstar=7, min_bin=0, min_score=0.0,
                 grouped=0):
        self.name, self.keys, self.k = name, _a(keys, u64), int(k)
        self.count = len(self.keys) if count is None else int(count)
        self.hits = None if hits is None else int(hits)
        self.pruned, self.bstar, self.min_bin, self.min_score, self.grouped = pruned, bstar, min_bin, min_score, grouped


def state_select(rows, cand_cap, k_max, with_min_bin, with_min_score, with_groups, status_in=0):
    """The plain statement of k_select (the comment above it in kernels.h): per query the first
    min(k, n') of the n' = min(count, cand_cap) keys sorted descending, cut where the score falls
    below a caller's min_score > 0; the rest of the row untouched; the two status bits."""
    out = np.full((len(rows), k_max, 2), FILL32, u32)
    count = np.zeros(len(rows), u32)
    status = status_in
    for q, r in enumerate(rows):
        n = min(r.count, cand_cap)
        keys = np.sort(r.keys[:n])[::-1]
        assert len(np.unique(keys)) == n, (r.name, "keys are unique: the kernel's contract")
        top = keys[:min(r.k, n)]
        if with_min_score and r.min_score > 0:
            top = top[scores_of(top) >= f32(r.min_score)]
        out[q, :len(top)] = hits_of(top)
        count[q] = len(top)
        if r.count > cand_cap:
            status |= ST_OVER
        hits = n if r.hits is None else r.hits
        callers = with_min_bin and r.min_bin != 0 and r.bstar == r.min_bin
        grouped = with_groups and r.grouped != 0
        if n < r.k and (hits > n or r.pruned) and not callers and not grouped:
            status |= ST_UNDER
    return out, count, status


def run_select(P, name, rows, cand_cap=CAND_CAP, stage_cap=None, k_max=None, with_min_bin=False,
               with_min_score=False, with_groups=False, status_in=0):
    """One launch of k_select on `rows`, compared with the statement."""
    nq = len(rows)
    k_max = max(r.k for r in rows) if k_max is None else k_max
    sort_cap = sort_cap_of(k_max)
    stage_cap = min(cand_cap, SELECT_STAGE) if stage_cap is None else stage_cap
    cands = np.empty((nq, cand_cap), u64)
    # (slots behind a row's count: keys above every real one — a kernel that read them would list them)
    cands[:] = (u64(0x7F7FFFFF) << u64(32)) | np.arange(1, cand_cap + 1, dtype=u64)
    for q, r in enumerate(rows):
        assert len(r.keys) >= min(r.count, cand_cap), r.name
        m = min(len(r.keys), cand_cap)
        cands[q, :m] = r.keys[:m]
    count = _a([r.count for r in rows], u32)
    hits = _a([min(r.count, cand_cap) if r.hits is None else r.hits for r in rows], u64)
    k = _a([r.k for r in rows], u32)
    bstar, pruned = _a([r.bstar for r in rows], u32), _a([r.pruned for r in rows], u32)
    min_bin = _a([r.min_bin for r in rows], u32) if with_min_bin else None
    min_score = _a([r.min_score for r in rows], f32) if with_min_score else None
    group_of = _a([r.grouped for r in rows], u32) if with_groups else None
    out = np.zeros((nq, k_max, 2), u32)
    out_count = np.zeros(nq, u32)
    status = _a([status_in], u32)
    rc = P.sp_select(_p(cands), nq, cand_cap, _p(count), _p(hits), _p(k), k_max, stage_cap, sort_cap, _p(bstar),
                     _p(min_bin), _p(pruned), _p(min_score), _p(group_of), _p(out), _p(out_count), _p(status))
    assert rc == 0, (name, rc)
    want, want_count, want_status = state_select(rows, cand_cap, k_max, with_min_bin, with_min_score, with_groups,
                                                 status_in)
    for q, r in enumerate(rows):
        what = (name, r.name, "n", r.count, "k", r.k, "caps", cand_cap, stage_cap, sort_cap)
        assert int(out_count[q]) == int(want_count[q]), what + ("count", int(out_count[q]), int(want_count[q]))
        bad = np.argwhere(out[q] != want[q])
        assert bad.size == 0, what + ("slot", int(bad[0][0]), [hex(int(v)) for v in out[q, bad[0][0]]],
                                      [hex(int(v)) for v in want[q, bad[0][0]]])
    assert int(status[0]) == want_status, (name, "status", int(status[0]), want_status)


def sizes_around(k, cand_cap, stage_cap):
    sc = sort_cap_of(k)
    ns = {0, 1, k - 1, k, k + 1, sc - 1, sc, sc + 1, stage_cap - 1, stage_cap, stage_cap + 1, cand_cap}
    return sorted(n for n in ns if 0 <= n <= cand_cap)


KS = (1, 3, 63, 64, 65, 100, 1000, 1024, MAX_K)


def check_select_sizes(P):
    """Every k of the list as k_max under the default caps: n at every edge of k, sort_cap, stage_cap
    and cand_cap in ONE launch, a smaller k at two of them; then a count beyond cand_cap in front of
    a plain query."""
    rng = np.random.default_rng(4101)
    for k in KS:
        ns = sizes_around(k, CAND_CAP, SELECT_STAGE)
        rows = [Row("n=%d" % n, random_keys(rng, n), k) for n in ns]
        sc = sort_cap_of(k)
        for kq in sorted({1, k // 2 + 1, k - 1} - {0, k}):
            rows += [Row("k=%d of k_max, n=%d" % (kq, n), random_keys(rng, n), kq) for n in (sc, sc + 1, CAND_CAP)]
        run_select(P, "sizes k_max=%d" % k, rows, k_max=k)
        run_select(P, "beyond cand_cap, k_max=%d" % k,
                   [Row("count=cap+5", random_keys(rng, CAND_CAP), k, count=CAND_CAP + 5),
                    Row("plain", random_keys(rng, CAND_CAP // 3) | u64(1 << 62), k)], k_max=k)


def check_select_unstaged(P):
    """A reduced stage_cap (256 under a cand_cap of 2048): the passes that re-read global memory, with
    few keys; in input order ascending, descending and shuffled."""
    rng = np.random.default_rng(4102)
    cap, stage = 2048, 256
    for k in (3, 64, 100, 1000):
        rows = []
        for n in sizes_around(k, cap, stage) + [cap // 2 + 77]:
            keys = random_keys(rng, n)
            rows += [Row("n=%d shuffled" % n, keys, k), Row("n=%d ascending" % n, np.sort(keys), k),
                     Row("n=%d descending" % n, np.sort(keys)[::-1], k)]
        run_select(P, "unstaged k_max=%d" % k, rows, cand_cap=cap, stage_cap=stage, k_max=k)
    run_select(P, "unstaged, beyond cand_cap",
               [Row("count=cap+1", random_keys(rng, cap), 100, count=cap + 1),
                Row("plain", random_keys(rng, 300) | u64(1 << 62), 100)], cand_cap=cap, stage_cap=stage)


PREFIX = (0x3F, 0x12, 0x34, 0x56, 0x9A, 0xBC, 0xDE)   # a positive float's bytes, then doc bytes


def pass_set(rng, p, wanted, above, below, digit, digit_above):
    """Keys that share their first p bytes; at byte p `above` keys carry digit_above, `wanted` keys
    `digit`, `below` keys smaller digits; the bytes behind are random and distinct.  With
    k = above + wanted the radix select needs the bucket `digit` WHOLE at exactly pass p — and not
    before: passes 0 .. p-1 see one bucket of all the keys."""
    rest = 7 - p
    n = above + wanted + below
    lows = digit - 1 - (np.arange(below) % min(digit, 9))
    digits = np.concatenate([np.full(above, digit_above), np.full(wanted, digit), lows]).astype(u64)
    if rest:
        tail = rng.choice(min(1 << (8 * rest), 1 << 40), n, replace=False).astype(u64)
    else:
        tail = np.zeros(n, u64)
        assert len(np.unique(digits)) == n
    head = u64(0)
    for b in PREFIX[:p]:
        head = (head << u64(8)) | u64(b)
    keys = (((head << u64(8)) | digits) << u64(8 * rest)) | tail
    keys |= u64(1) if p < 4 else u64(0)     # (a doc below 0xFFFFFFFF; in the doc bytes the prefix sees to it)
    assert len(np.unique(keys)) == n
    return rng.permutation(keys)


def check_select_passes(P):
    """For every pass p = 0 .. 7 a set whose needed bucket is needed whole at exactly pass p (the early
    exit) — digit 0x3F / 100 for thread 192 / 155, seven keys above it in another wavefront's digit —
    and the same set with one key more in that bucket (no exit; at pass 7 a bucket holds one key at
    most, so there is none).  A k-th key alone in its bucket; one score for all docs; 256 keys that
    differ in the lowest byte only, k = 1, 64 and in between, in three input orders."""
    rng = np.random.default_rng(4103)
    rows = []
    for p in range(7):
        d, da = (0x3F, 0x41) if p == 0 else (100, 250)
        rows.append(Row("exit at pass %d" % p, pass_set(rng, p, 33, 7, 60, d, da), 40))
        rows.append(Row("one more at pass %d" % p, pass_set(rng, p, 34, 7, 60, d, da), 40))
        rows.append(Row("k-th alone at pass %d" % p, pass_set(rng, p, 1, 39, 60, d, da), 40))
        rows.append(Row("nothing above, pass %d" % p, pass_set(rng, p, 40, 0, 60, d, da), 40))
    low = rng.choice(256, 100, replace=False)       # (at pass 7 a bucket holds one key: needed whole)
    head = u64(0)
    for b in PREFIX:
        head = (head << u64(8)) | u64(b)
    rows.append(Row("exit at pass 7", rng.permutation((head << u64(8)) | low.astype(u64)), 40))
    run_select(P, "passes", rows, k_max=40)
    lowest = (head << u64(8)) | np.arange(256, dtype=u64)
    docs = docs_for(rng, 3000)
    same = make_keys(np.full(3000, 2.5, f32), docs)
    near = rng.permutation(make_keys(np.full(300, 2.5, f32), u64(0x123456F0) + np.arange(300, dtype=u64)))
    for k in (1, 33, 64):
        rows = [Row("lowest byte, shuffled", rng.permutation(lowest), k),
                Row("lowest byte, ascending", lowest, k), Row("lowest byte, descending", lowest[::-1], k),
                Row("one score, 3000 docs", same, k), Row("one score, 300 docs in a row", near, k),
                Row("one score, ascending", np.sort(same), k), Row("one score, descending", np.sort(same)[::-1], k)]
        run_select(P, "ties k=%d" % k, rows, k_max=k)
        run_select(P, "ties k=%d, unstaged" % k, rows, cand_cap=4096, stage_cap=128, k_max=k)


def check_select_range(P):
    """Scores across the positive float range — denormals, 0.0 (zero boosts exist), the largest finite
    float — and the docs 1, 2^31 and 0xFFFFFFFE, where the doc decides."""
    rng = np.random.default_rng(4104)
    edge_docs = _a([1, 2, 1 << 31, (1 << 31) - 1, (1 << 31) + 1, 0xFFFFFFFE, 0xFFFFFFFD], u64)
    rows = []
    for n, k in ((40, 100), (500, 100), (500, 7), (9000, 100), (9000, 1)):
        bits = rng.integers(0, 0x7F800000, n, dtype=np.uint64).astype(u32)
        bits[: n // 8] = 0                                # score 0.0
        bits[n // 8: n // 6] = rng.integers(1, 1 << 23, n // 6 - n // 8)   # denormals
        bits[-1] = 0x7F7FFFFF
        docs = docs_for(rng, n) + u64(10)                 # (11 .. 2^28: none of the edge docs)
        docs[:7] = edge_docs
        bits[:7] = (0, 0, 0x3F800000, 0x3F800000, 0x3F800000, 0, 0x3F800000)
        rows.append(Row("range n=%d k=%d" % (n, k), make_keys(bits.view(f32), docs), k))
        tied = make_keys(np.zeros(n, f32), np.concatenate([edge_docs, docs[7:]]))
        rows.append(Row("all 0.0 n=%d k=%d" % (n, k), rng.permutation(tied), k))
    run_select(P, "range", rows, k_max=100)


def check_select_min_score(P):
    """min_score: absent, 0, below all, exactly the k-th score, a score several docs inside the top k
    share, above all — on the direct sort, the staged and the unstaged select."""
    rng = np.random.default_rng(4105)
    for n, cap, stage, k in ((50, CAND_CAP, SELECT_STAGE, 64), (3000, CAND_CAP, SELECT_STAGE, 64),
                             (3000, CAND_CAP, SELECT_STAGE, 1000), (1500, 2048, 256, 100)):
        levels = (np.arange(1, 1 + min(40, max(4, n // 12)), dtype=np.float64) * 0.37).astype(f32)   # scores shared
        keys = make_keys(levels[rng.integers(0, len(levels), n)], docs_for(rng, n))
        srt = scores_of(np.sort(keys)[::-1])
        kth = float(srt[min(k, n) - 1])
        inside = float(srt[min(k, n) // 2])
        assert np.count_nonzero(srt[:min(k, n)] == f32(inside)) > 1 and np.count_nonzero(srt == f32(kth)) > 1
        values = {"0": 0.0, "below all": float(levels[0]) / 2, "the k-th score": kth,
                  "just above the k-th": float(np.nextafter(f32(kth), f32(np.inf))), "shared inside": inside,
                  "just above it": float(np.nextafter(f32(inside), f32(np.inf))),
                  "the best": float(srt[0]), "above all": float(levels[-1]) * 2, "negative": -1.0}
        rows = [Row("min_score %s" % what, keys, k, min_score=v) for what, v in values.items()]
        run_select(P, "min_score n=%d k=%d" % (n, k), rows, cand_cap=cap, stage_cap=stage, k_max=k,
                   with_min_score=True)
        run_select(P, "min_score absent n=%d k=%d" % (n, k), rows, cand_cap=cap, stage_cap=stage, k_max=k)
        # with fewer than k above it, a cut list is no underflow of its own: only n, hits and pruned decide
        run_select(P, "min_score and more hits n=%d k=%d" % (n, k),
                   [Row("above all", keys, k, min_score=values["above all"], hits=n + 5, pruned=1)],
                   cand_cap=cap, stage_cap=stage, k_max=k, with_min_score=True)


def check_select_flags(P):
    """The whole truth table of {hits > n, pruned, the threshold is the caller's, grouped} at n < k and
    at n >= k, one launch per line (a launch has one status word), behind a plain query; the arrays
    absent; a min_bin of 0 and one that is not b*; the status bits that were there stay."""
    rng = np.random.default_rng(4106)
    plain = Row("plain", random_keys(rng, 30), 9)
    for n, k in ((5, 9), (0, 1), (12, 9), (9, 9), (200, 9)):
        keys = random_keys(rng, n)
        for more, pruned, callers, grouped in itertools.product((0, 1), repeat=4):
            row = Row("more=%d pruned=%d callers=%d grouped=%d" % (more, pruned, callers, grouped), keys, k,
                      hits=n + more, pruned=pruned * 3, bstar=9, min_bin=9 if callers else 4, grouped=grouped * 2)
            run_select(P, "flags n=%d k=%d" % (n, k), [plain, row], with_min_bin=True, with_groups=True)
            if (n, k) == (5, 9):
                run_select(P, "flags, no arrays", [plain, row])
                run_select(P, "flags, min_bin only", [row, plain], with_min_bin=True)
                run_select(P, "flags, groups only", [row, plain], with_groups=True, status_in=ST_CORRUPT)
    for min_bin, bstar in ((0, 0), (0, 9), (9, 10), (511, 511)):
        run_select(P, "callers min_bin=%d bstar=%d" % (min_bin, bstar),
                   [plain, Row("short", random_keys(rng, 5), 9, hits=6, bstar=bstar, min_bin=min_bin)],
                   with_min_bin=True)
    for st in (ST_CORRUPT, ST_OVER, ST_UNDER, ST_CORRUPT | ST_OVER | ST_UNDER):
        run_select(P, "status carried %d" % st, [plain], status_in=st)
    run_select(P, "two short queries", [Row("short %d" % i, random_keys(rng, 5), 9, hits=5 + i) for i in range(2)])


def check_select_largest(P, cap=CAND_CAP_MAX):
    """One query on the largest candidate buffer: n = cand_cap = 262144, k = 4096."""
    rng = np.random.default_rng(4107)
    run_select(P, "largest", [Row("n=cap", random_keys(rng, cap, 3.0), MAX_K)], cand_cap=cap)


# ---- the threshold pick --------------------------------------------------------------------------

def need_of(k, margin, sampled, total):
    """score.h above k_pilot: sound (margin 0) k; estimated ceil(margin * k * sampled / total), never
    less than kPilotMinSample, never more than k."""
    if not margin:
        return k
    est = -(-(margin * k * sampled) // total) if total else 0
    return min(max(est, MIN_SAMPLE), k)


def sampled_of(unit, stride, total):
    """the pilot's sample {phase, phase + stride, ...} below total, phase = 7 * unit mod stride"""
    phase = (unit * 7) % stride
    return len(range(phase, total, stride))


def pick(hist, need):
    """the largest bin whose suffix sum reaches need, else 0"""
    suffix = np.cumsum(np.asarray(hist, np.uint64)[::-1])       # suffix[i] = docs in bins >= kBins - 1 - i
    reach = np.flatnonzero(suffix >= np.uint64(need))
    return K_BINS - 1 - int(reach[0]) if reach.size else 0


def _hist(**bins):
    h = np.zeros(K_BINS, np.uint64)
    for b, v in bins.items():
        h[int(b[1:])] = v
    return h


def _met_at(b, short):
    """`need` (one less: short) reached exactly at bin b: half of it nine bins up (another 8-bin chunk),
    single docs in the odd bins below"""
    def make(need):
        h = np.zeros(K_BINS, np.uint64)
        up = need // 2 if b + 9 < K_BINS else 0
        if up:
            h[b + 9] = up
        h[b] = need - up - short
        if b % 2:
            h[:b] = 1
        if b and short:
            h[b - 1] = 1
        return h
    return make


def _by_total(short):
    def make(need):
        h = _hist(b1=need // 7, b200=need // 3, b511=need // 2)
        h[0] = max(need - need // 2 - need // 3 - need // 7 - short, 0)
        return h
    return make


# (name, need -> histogram): what one unit's pick is looked for in
HIST_CASES = [("empty", lambda need: _hist()),
              ("all mass in bin 0", lambda need: _hist(b0=5 * need + 3)),
              ("all mass in bin 511", lambda need: _hist(b511=5 * need + 3))] + \
    [("need %s at bin %d" % ("one short" if short else "met exactly", b), _met_at(b, short))
     for b in (8, 15, 16, 0, 7, 504, 511, 263, 264) for short in (0, 1)] + \
    [("need met only by the total", _by_total(0)), ("need not met at all", _by_total(1)),
     ("total 2^32 - 1", lambda need: _hist(b511=5, b300=1 << 31, b0=(1 << 32) - 1 - 5 - (1 << 31))),
     ("2^32 - 1 in one bin", lambda need: _hist(b3=(1 << 32) - 1)),
     ("five per bin", lambda need: np.full(K_BINS, 5, np.uint64)),
     ("one per bin", lambda need: np.full(K_BINS, 1, np.uint64))]


def random_hist(rng):
    kind = rng.integers(0, 4)
    if kind == 0:
        return rng.integers(0, 40, K_BINS).astype(np.uint64)
    h = np.zeros(K_BINS, np.uint64)
    m = int(rng.integers(1, 60))
    at = rng.integers(0, K_BINS, m)
    np.add.at(h, at, rng.integers(1, (3, 300, 100000)[kind - 1], m).astype(np.uint64))
    return h


def threshold_units(rng, margin, stride, first_unit):
    """(name, hist, k, total, min_bin) per unit of one launch (stride, margin).  A unit's `need`
    depends on its NUMBER through the phase of its sample, so its histogram is made for the number
    it gets: first_unit + its place.  (total = the unit's lead items, up to 2^31.)"""
    units = []

    def add(name, k, total, make):
        need = need_of(k, margin, sampled_of(first_unit + len(units), stride, total), total)
        units.append(("%s; k=%d total=%d need=%d" % (name, k, total, need), make(need), k, total, 0))

    for k in (1, 3, MIN_SAMPLE - 1, MIN_SAMPLE, MIN_SAMPLE + 1, 100, 1000, MAX_K):
        for total in sorted({0, 1, 2, max(stride - 1, 0), stride, stride + 1, 100, 1000, 100000, 1 << 31}):
            for name, make in HIST_CASES:
                add(name, k, total, make)
    for i in range(300):
        k = int(rng.choice((1, 10, 100, 1000, int(rng.integers(1, MAX_K + 1)))))
        total = int(rng.choice((int(rng.integers(0, 50)), int(rng.integers(50, 5000)), int(rng.integers(1, 1 << 31)))))
        add("random %d" % i, k, total, lambda need: random_hist(rng))
    return units


def with_min_bins(rng, units, pick_of):
    """every third unit a min_bin above its pick, every third one below, the rest 0"""
    out = []
    for i, (name, h, k, total, _) in enumerate(units):
        b = pick_of(i)
        mb = (0, min(b + 1 + i % 5, K_BINS - 1), max(b - 1 - i % 5, 0))[i % 3]
        out.append((name + "; min_bin=%d" % mb, h, k, total, mb))
    return out


def check_conj_threshold(P):
    """k_conj_threshold: sound and estimated picks at strides 1 .. 1000 (phase >= total, stride 1,
    total 0 among them), min_bin absent, above and below, the units listed in another order than
    their numbers and not all of them: the others' b* stay untouched."""
    rng = np.random.default_rng(4201)
    for margin, stride in ((0, 1), (0, 16), (MARGIN, 1), (MARGIN, 4), (MARGIN, 16), (MARGIN, 1000), (1, 3)):
        spare = 5
        units = threshold_units(rng, margin, stride, spare)
        for given in (False, True):
            need = [need_of(k, margin, sampled_of(spare + i, stride, total), total)
                    for i, (_, _, k, total, _) in enumerate(units)]
            if given:
                units = with_min_bins(rng, units, lambda i: pick(units[i][1], need[i]))
            nc, nq = len(units), len(units) + 2 * spare
            order = rng.permutation(nc)
            hist = rng.integers(0, 1000, (nq, K_BINS)).astype(u32)     # (the spare units' rows: never read)
            kq = np.full(nq, 77, u32)
            min_bin = np.full(nq, 300, u32)
            for i, (_, h, k, _, mb) in enumerate(units):
                hist[spare + i], kq[spare + i], min_bin[spare + i] = h.astype(u32), k, mb
            conj_units = _a(spare + order, u32)
            n_items = _a([units[i][3] for i in order], u32)
            bstar = np.zeros(nq, u32)
            rc = P.sp_conj_threshold(_p(kq), nq, _p(conj_units), _p(n_items), nc, _p(hist), stride, margin,
                                     _p(min_bin) if given else None, _p(bstar))
            assert rc == 0, rc
            for i, (name, h, k, total, mb) in enumerate(units):
                want = max(pick(h, need[i]), mb if given else 0)
                assert int(bstar[spare + i]) == want, ("k_conj_threshold", margin, stride, name, "unit", spare + i,
                                                       int(bstar[spare + i]), want)
            rest = np.concatenate([bstar[:spare], bstar[spare + nc:]])
            assert (rest == FILL32).all(), ("k_conj_threshold wrote a unit it was not given", margin, stride)


def check_group_threshold(P):
    """k_group_threshold: n_segs 1, 2 and 64; members missing first, last, here and there and
    everywhere; every member gets the group's bin (or its own min_bin above it), nobody else."""
    rng = np.random.default_rng(4202)
    for margin, n_segs in ((0, 1), (MARGIN, 1), (MARGIN, 2), (0, 2), (MARGIN, 64), (0, 64), (MARGIN, 5)):
        groups = []   # (name, hist, k, sampled, tiles)
        for k in (1, 3, MIN_SAMPLE, 100, 1000, MAX_K):
            for sampled, tiles in ((1, 1), (1, 16), (7, 100), (100, 100), (0, 9), (3, 0xFFFFFFFF), (40000, 600000)):
                need = need_of(k, margin, sampled, tiles)
                groups += [("%s; k=%d sampled=%d tiles=%d need=%d" % (what, k, sampled, tiles, need), make(need), k,
                            sampled, tiles) for what, make in HIST_CASES]
        for i in range(200):
            tiles = int(rng.integers(1, 100000))
            groups.append(("random %d" % i, random_hist(rng), int(rng.integers(1, MAX_K + 1)),
                           int(rng.integers(0, tiles + 1)), tiles))
        ng = len(groups)
        nq = ng * n_segs + 3
        unit_of = rng.permutation(nq)[: ng * n_segs].reshape(ng, n_segs)
        members = unit_of.astype(u32)
        for g in range(ng):
            how = g % 6
            if n_segs > 1 and how == 1:
                members[g, 0] = NONE
            elif n_segs > 1 and how == 2:
                members[g, -1] = NONE
            elif n_segs > 2 and how == 3:
                members[g, rng.random(n_segs) < 0.5] = NONE
            elif how == 4 and g % 5 == 4:
                members[g, :] = NONE
            elif n_segs > 1 and how == 5:
                members[g, :-1] = NONE
        group_hist = np.zeros((ng, K_BINS + 2), u32)
        kq = np.full(nq, 4000, u32)
        for g, (_, h, k, sampled, tiles) in enumerate(groups):
            group_hist[g, :K_BINS], group_hist[g, K_BINS], group_hist[g, K_BINS + 1] = h.astype(u32), sampled, tiles
            first = [u for u in members[g] if u != NONE][:1]
            kq[unit_of[g]] = rng.integers(1, 5000, n_segs)      # (only the first present member's k counts)
            if first:
                kq[first[0]] = k
        members = np.ascontiguousarray(members)
        for given in (False, True):
            min_bin = rng.integers(0, K_BINS, nq).astype(u32)
            min_bin[rng.random(nq) < 0.4] = 0
            bstar = np.zeros(nq, u32)
            rc = P.sp_group_threshold(_p(kq), nq, _p(members), n_segs, ng, _p(group_hist), margin,
                                      _p(min_bin) if given else None, _p(bstar))
            assert rc == 0, rc
            want = np.full(nq, FILL32, np.int64)
            for g, (name, h, k, sampled, tiles) in enumerate(groups):
                b = pick(h, need_of(k, margin, sampled, tiles))
                for u in members[g]:
                    if u != NONE:
                        want[u] = max(b, int(min_bin[u])) if given else b
            bad = np.flatnonzero(bstar.astype(np.int64) != want)
            if bad.size:
                g = [g for g in range(ng) if bad[0] in unit_of[g]]
                assert False, ("k_group_threshold", margin, n_segs, given, groups[g[0]][0] if g else "a spare unit",
                               "unit", int(bad[0]), int(bstar[bad[0]]), int(want[bad[0]]))


# ---- the group verdict ---------------------------------------------------------------------------

def state_group(k, members, out_count, hits, bstar, min_bin, status_in):
    """join.h above k_group_sums: per group the entries listed, the docs matched (at most k per unit)
    and the units whose threshold is the caller's own, then the run's two status bits so far; the
    verdict raises the underflow for a group that lists fewer than k although more matched, unless
    some unit's threshold is the caller's."""
    ng = len(members)
    sums = np.zeros(ng * SUM_WORDS + 2, u32)
    status = status_in
    for g, row in enumerate(members):
        got = matched = callers = 0
        for u in row:
            if u == NONE:
                continue
            got += int(out_count[u])
            matched += min(int(hits[u]), int(k[u]))
            callers += int(min_bin is not None and min_bin[u] != 0 and bstar[u] == min_bin[u])
        sums[g * SUM_WORDS: (g + 1) * SUM_WORDS] = (got, matched, callers)
        if got < int(k[g]) and matched > got and not callers:
            status |= ST_UNDER
    sums[ng * SUM_WORDS:] = (int(bool(status_in & ST_UNDER)), int(bool(status_in & ST_OVER)))
    return sums, status


def run_group(P, name, k, members, out_count, hits, bstar, min_bin, status_in):
    k, members, out_count = _a(k, u32), _a(members, u32), _a(out_count, u32)
    hits, bstar = _a(hits, u64), _a(bstar, u32)
    min_bin = None if min_bin is None else _a(min_bin, u32)
    ng, n_segs = members.shape
    sums = np.zeros(ng * SUM_WORDS + 2, u32)
    status = _a([status_in], u32)
    rc = P.sp_group_verdict(_p(k), len(k), _p(members), n_segs, ng, _p(out_count), _p(hits), _p(bstar), _p(min_bin),
                            _p(status), _p(sums))
    assert rc == 0, (name, rc)
    want, want_status = state_group(k, members, out_count, hits, bstar, min_bin, status_in)
    assert (sums == want).all(), (name, "sums", sums.tolist(), want.tolist())
    assert int(status[0]) == want_status, (name, "status", int(status[0]), want_status)


def check_group_verdict(P):
    """The truth table of (got < k, matched > got, callers) for one group of three segments among
    plain groups, with every status word carried in; matched capped at k per unit (hits of 2^40);
    members missing; 70 groups (two workgroups)."""
    rng = np.random.default_rng(4203)
    ng, n_segs, k = 3, 3, 10
    nq = ng * n_segs
    unit = lambda s, g: s * ng + g  # noqa: E731
    members = np.array([[unit(s, g) for s in range(n_segs)] for g in range(ng)])
    for short, more, callers, where in itertools.product((0, 1), (0, 1), (0, 1), range(ng)):
        for status_in in (0, ST_UNDER, ST_OVER, ST_CORRUPT, ST_UNDER | ST_OVER | ST_CORRUPT):
            out_count = np.full(nq, 4)          # plain groups: 12 listed, 12 matched
            hits = np.full(nq, 4)
            bstar, min_bin = np.full(nq, 9), np.full(nq, 5)
            us = members[where]
            out_count[us] = (3, 2, 4) if short else (3, 3, 4)
            hits[us] = out_count[us] + (np.array((0, 1, 0)) if more else 0)
            if callers:
                min_bin[us[2]] = 9
            name = "verdict short=%d more=%d callers=%d group=%d status=%d" % (short, more, callers, where, status_in)
            run_group(P, name, np.full(nq, k), members, out_count, hits, bstar, min_bin, status_in)
            run_group(P, name + ", no min_bin", np.full(nq, k), members, out_count, hits, bstar, None, status_in)
    # matched is capped at k per unit: two units of 2^40 hits and k = 10 are 20 matched, the group lists 9
    big = 1 << 40
    run_group(P, "capped, short", [10, 10], [[0, 1]], [5, 4], [big, big], [3, 3], [0, 0], 0)
    run_group(P, "capped, full", [10, 10], [[0, 1]], [5, 5], [big, big], [3, 3], [0, 0], 0)
    run_group(P, "hits a multiple of 2^32", [10, 10], [[0, 1]], [0, 0], [1 << 32, 0], [3, 3], None, 0)
    run_group(P, "min_bin 0 is nobody's threshold", [10, 10], [[0, 1]], [2, 2], [5, 2], [0, 0], [0, 0], 0)
    run_group(P, "members missing", [10] * 6, [[NONE, 2, NONE], [1, NONE, 3], [NONE, NONE, NONE]],
              [9, 1, 2, 3, 9, 9], [9, 1, 9, 3, 9, 9], [3] * 6, None, 0)
    ng, n_segs = 70, 2
    nq = ng * n_segs
    members = np.array([[g, ng + g] for g in range(ng)])
    for it in range(6):
        kq = np.tile(rng.integers(1, 40, ng), 2)
        out_count = np.minimum(rng.integers(0, 30, nq), kq)
        hits = out_count + rng.integers(0, 2, nq) * (it % 2)
        bstar, min_bin = rng.integers(0, 3, nq), rng.integers(0, 3, nq)
        if it < 2:     # one group decides, in the second workgroup
            out_count[:], hits[:] = kq, kq
            out_count[[69, 139]], hits[[69, 139]] = 0, (it, 0)
        run_group(P, "70 groups, round %d" % it, kq, members, out_count, hits, bstar, min_bin, 0)


# ---- k_conj_hits ---------------------------------------------------------------------------------

def check_conj_hits(P):
    """hits[unit] = the exact 64-bit sum of the unit's items: 0, 1, 63, 64, 65 and several thousand
    items, values that carry across the kernel's 24-bit split and totals beyond 2^32; the units in
    another order than their numbers, the others untouched."""
    rng = np.random.default_rng(4301)
    lists = []
    for n in (0, 1, 63, 64, 65, 127, 128, 129, 5000):
        lists.append(rng.integers(0, 1 << 32, n, dtype=np.uint64))
        lists.append(np.full(n, 0xFFFFFF, np.uint64))
        lists.append(np.full(n, 0x1000000, np.uint64))
        lists.append(np.full(n, 0xFFFFFFFF, np.uint64))
        lists.append(rng.integers(0, 3, n, dtype=np.uint64))
        one = np.zeros(n, np.uint64)
        one[-1:] = 0xFFFFFFFF
        lists.append(one)
    nc = len(lists)
    nq = nc + 7
    item_base = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(u32)
    item_hits = np.concatenate(lists).astype(u32)
    conj_units = _a(3 + rng.permutation(nc), u32)
    hits = np.zeros(nq, u64)
    assert P.sp_conj_hits(_p(conj_units), _p(item_base), _p(item_hits), nc, len(item_hits), nq, _p(hits)) == 0
    want = np.full(nq, FILL64, u64)
    for c, l in enumerate(lists):
        want[conj_units[c]] = sum(int(v) for v in l)
    assert max(sum(int(v) for v in l) for l in lists) > 1 << 44
    bad = np.flatnonzero(hits != want)
    assert bad.size == 0, ("k_conj_hits", "unit", int(bad[0]), hex(int(hits[bad[0]])), hex(int(want[bad[0]])))


# ---- k_union_topk --------------------------------------------------------------------------------

def check_union(P):
    """out = the first min(k, na + nb, k_max) of the two lists merged in key order, na = min(ca, k_max);
    totals added in 64 bits; the row behind it untouched."""
    rng = np.random.default_rng(4401)
    k_max = 300
    rows = []      # (name, keys a, ca, keys b, cb, k, ta, tb)

    def split(name, keys, in_a, k, ca=None, cb=None, ta=None, tb=None):
        keys = np.sort(keys)[::-1]
        a, b = keys[in_a][:k_max], keys[~in_a][:k_max]
        rows.append((name, a, len(a) if ca is None else ca, b, len(b) if cb is None else cb, k,
                     int(rng.integers(0, 1 << 20)) if ta is None else ta,
                     int(rng.integers(0, 1 << 20)) if tb is None else tb))

    for n, k in ((0, 5), (1, 5), (7, 100), (300, 300), (300, 299), (301, 300), (600, 300), (600, 1), (257, 256),
                 (513, 200)):
        keys = random_keys(rng, n)
        mask = rng.random(n) < 0.5
        split("random n=%d k=%d" % (n, k), keys, mask, k)
        split("a empty n=%d k=%d" % (n, k), keys[:k_max], np.zeros(min(n, k_max), bool), k)
        split("b empty n=%d k=%d" % (n, k), keys[:k_max], np.ones(min(n, k_max), bool), k)
        first = np.arange(n) < n // 2
        split("all of a before b n=%d k=%d" % (n, k), keys, first, k)
        split("all of b before a n=%d k=%d" % (n, k), keys, ~first, k)
        split("alternating n=%d k=%d" % (n, k), keys, np.arange(n) % 2 == 0, k)
        tied = make_keys((rng.integers(1, 4, n) * 0.5).astype(f32), docs_for(rng, n))
        split("equal scores, the doc decides n=%d k=%d" % (n, k), tied, mask, k)
        one = make_keys(np.full(n, 1.0, f32), np.arange(1, n + 1))
        split("one score, docs alternating n=%d k=%d" % (n, k), one, np.arange(n) % 2 == 1, k)
    keys = random_keys(rng, 2 * k_max)
    half = np.arange(2 * k_max) % 2 == 0
    split("ca > k_max is clamped", keys, half, 300, ca=k_max + 50, cb=k_max)
    split("cb > k_max is clamped", keys, half, 250, ca=10, cb=NONE)
    split("totals above 2^32", keys, half, 20, ta=(1 << 32) + 5, tb=(1 << 33) + (1 << 32) - 1)
    split("totals that carry", keys, half, 20, ta=0xFFFFFFFF, tb=1)
    nq = len(rows)
    poison = np.array([0x7F7FFFFF, 7], u32)       # (behind a list's count: never read)
    a, b = np.tile(poison, (nq, k_max, 1)), np.tile(poison, (nq, k_max, 1))
    for q, (_, ka, _, kb, _, _, _, _) in enumerate(rows):
        a[q, :len(ka)], b[q, :len(kb)] = hits_of(ka), hits_of(kb)
    ca, cb = _a([r[2] for r in rows], u32), _a([r[4] for r in rows], u32)
    ta, tb = _a([r[6] for r in rows], u64), _a([r[7] for r in rows], u64)
    k = _a([r[5] for r in rows], u32)
    out, out_count, out_total = np.zeros((nq, k_max, 2), u32), np.zeros(nq, u32), np.zeros(nq, u64)
    rc = P.sp_union(_p(k), nq, k_max, _p(a), _p(ca), _p(ta), _p(b), _p(cb), _p(tb), _p(out), _p(out_count),
                    _p(out_total))
    assert rc == 0, rc
    for q, (name, ka, na, kb, nb, kq, sa, sb) in enumerate(rows):
        na, nb = min(na, k_max), min(nb, k_max)
        merged = np.sort(np.concatenate([ka[:na], kb[:nb]]))[::-1]
        keep = min(kq, na + nb, k_max)
        want = np.full((k_max, 2), FILL32, u32)
        want[:keep] = hits_of(merged[:keep])
        assert int(out_count[q]) == keep, ("k_union_topk", name, "count", int(out_count[q]), keep)
        assert int(out_total[q]) == sa + sb, ("k_union_topk", name, "total", int(out_total[q]), sa + sb)
        bad = np.argwhere(out[q] != want)
        assert bad.size == 0, ("k_union_topk", name, "slot", int(bad[0][0]), out[q, bad[0][0]].tolist(),
                               want[bad[0][0]].tolist())


# ---- bins ----------------------------------------------------------------------------------------

def bin_domains():
    """(U, e, bin_scale, fx_inv 64-bit, fx_inv 32-bit) as units.h unit_scale / widen_fixed_point make
    them: U < 2^e, bin_scale = float(kBins / U), fx_inv = 2^(e - 61) and 2^(e - 30)."""
    rng = np.random.default_rng(4501)
    us = list(10.0 ** rng.uniform(-3, 4, 40)) + [1e-3, 1e4]
    for j in range(-10, 14):
        p = f32(2.0) ** f32(j)
        us += [float(p), float(np.nextafter(p, f32(0))), float(np.nextafter(p, f32(np.inf)))]
    out = []
    for U in us:
        e = int(np.frexp(U)[1])
        assert 2.0 ** (e - 1) <= U < 2.0 ** e
        out.append((U, e, f32(float(K_BINS) / U), f32(2.0 ** (e - 61)), f32(2.0 ** (e - 30))))
    return out


def bins_of(P, acc, bs, scale, fx_inv, wide):
    n = len(acc)
    acc, bs, scale, fx_inv = _a(acc, u64), _a(bs, u32), _a(scale, f32), _a(fx_inv, f32)
    val, b, thr = np.zeros(n, f32), np.zeros(n, u32), np.zeros(n, u64)
    assert P.sp_bins(_p(acc), _p(bs), _p(scale), _p(fx_inv), n, int(wide), _p(val), _p(b), _p(thr)) == 0
    return val, b, thr


def state_bins(acc, scale, fx_inv):
    """score.h in float32: from_fixed = float(acc) * fx_inv, score_bin = uint32(min(v * scale, kBins - 1))"""
    v = _a(acc, u64).astype(f32) * _a(fx_inv, f32)
    return v, np.minimum(v * _a(scale, f32), f32(K_BINS - 1)).astype(u32)


def state_threshold(bs, scale, fx_inv, wide):
    """bin_threshold in float64: 1 for bin 0, else the bin's lower edge in accumulator units less 1e-6
    of it, truncated."""
    edge = _a(bs, np.float64) / _a(scale, f32).astype(np.float64) / _a(fx_inv, f32).astype(np.float64)
    t = edge * (1.0 - 1e-6)
    return np.where(_a(bs, u32) == 0, u64(1), t.astype(u64))


def check_bins(P, tier="twin"):
    """1. exact: from_fixed and score_bin equal the float32 restatement bit for bit (accumulators near
    2^64, the clamp at 511, acc = 0), bin_threshold the float64 one; 2. monotone in acc; 3. sound:
    for every bs in 1 .. 511 and both accumulator types the smallest acc whose float bin is >= bs
    (bisection over the probe's own output) is >= bin_threshold(bs); 4. not loose: it is at most
    1.25e-6 * acc + 2 above it."""
    rng = np.random.default_rng(4502)
    doms = bin_domains()
    for wide in (True, False):
        top = 62 if wide else 31        # the bisection's upper end: acc = 2^top lies in bin 511 in every domain
        full = 64 if wide else 32
        # 1. and 2.
        per = 600
        accs, scales, fxs = [], [], []
        for U, e, scale, fx64, fx32 in doms:
            a = np.concatenate([
                rng.integers(0, 1 << (top - 1), per // 2, dtype=np.uint64),
                (rng.random(per // 2) * 2.0 ** (top - 1) * rng.random(per // 2) ** 4).astype(u64),
                np.array([0, 1, 2, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << full) - 1, (1 << full) - 2,
                          ((1 << 24) - 1) << (full - 24), (((1 << 25) - 1) << (full - 25)), 1 << (full - 1),
                          (1 << (full - 1)) - 1, 1 << top, (1 << top) - 1], dtype=np.uint64),
                u64((1 << full) - 1) - rng.integers(0, 1 << (full - 20), 20, dtype=np.uint64)])
            a = np.sort(a)
            accs.append(a)
            scales.append(np.full(len(a), scale, f32))
            fxs.append(np.full(len(a), fx64 if wide else fx32, f32))
        acc, scale, fx = np.concatenate(accs), np.concatenate(scales), np.concatenate(fxs)
        bs = (np.arange(len(acc)) % K_BINS).astype(u32)
        val, b, thr = bins_of(P, acc, bs, scale, fx, wide)
        want_val, want_bin = state_bins(acc, scale, fx)
        bad = np.flatnonzero((val.view(u32) != want_val.view(u32)) | (b != want_bin))
        assert bad.size == 0, ("bins: exact", "wide" if wide else "32-bit", hex(int(acc[bad[0]])), float(scale[bad[0]]),
                               float(fx[bad[0]]), float(val[bad[0]]), float(want_val[bad[0]]), int(b[bad[0]]),
                               int(want_bin[bad[0]]))
        assert b.max() == K_BINS - 1 and b.min() == 0
        at = 0
        for a in accs:      # (sorted per domain)
            seg = slice(at, at + len(a))
            assert (np.diff(b[seg].astype(np.int64)) >= 0).all() and (np.diff(val[seg]) >= 0).all(), \
                ("bins: monotone", wide, "domain", at // len(a))
            at += len(a)
        # 3. and 4.: per (domain, bs) the smallest acc with bin >= bs, by bisection
        nd = len(doms)
        bs = np.tile(np.arange(1, K_BINS, dtype=u32), nd)
        scale = np.repeat(_a([d[2] for d in doms], f32), K_BINS - 1)
        fx = np.repeat(_a([d[3] if wide else d[4] for d in doms], f32), K_BINS - 1)
        lo = np.zeros(len(bs), u64)                    # bin(lo) < bs   (bin(0) = 0)
        hi = np.full(len(bs), 1 << top, u64)           # bin(hi) >= bs
        _, b_hi, thr = bins_of(P, hi, bs, scale, fx, wide)
        assert (b_hi == K_BINS - 1).all()
        for _ in range(top):
            mid = lo + (hi - lo) // u64(2)
            _, b_mid, _ = bins_of(P, mid, bs, scale, fx, wide)
            up = b_mid >= bs
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid)
        assert (hi - lo == 1).all()
        _, b_lo, _ = bins_of(P, lo, bs, scale, fx, wide)
        _, b_hi, _ = bins_of(P, hi, bs, scale, fx, wide)
        assert (b_lo < bs).all() and (b_hi >= bs).all()
        smallest = hi.astype(np.float64)
        unsound = np.flatnonzero(hi < thr)
        gap = smallest - thr.astype(np.float64)       # (exact enough: the bound has 25 % to spare on 1e-6)
        rel = (gap - 2.0) / smallest
        print("bins property 4 (%s, %s accumulators): largest (smallest - threshold - 2) / smallest = %.4g; "
              "unsound pairs %d of %d" % (tier, "64-bit" if wide else "32-bit", float(rel.max()), unsound.size, len(bs)))
        i = unsound[0] if unsound.size else 0
        assert unsound.size == 0, ("bins: sound", wide, "U", doms[i // (K_BINS - 1)][0], "bs", int(bs[i]),
                                   "smallest", int(hi[i]), "threshold", int(thr[i]), unsound.size, "pairs")
        loose = np.flatnonzero(gap > 1.25e-6 * smallest + 2.0)
        i = loose[0] if loose.size else 0
        assert loose.size == 0, ("bins: not loose", wide, "U", doms[i // (K_BINS - 1)][0], "bs", int(bs[i]),
                                 "smallest", int(hi[i]), "threshold", int(thr[i]), float(rel.max()))
        # (and the header's formula itself, in float64: the properties above do not depend on this)
        want_thr = state_threshold(bs, scale, fx, wide)
        bad = np.flatnonzero(thr != want_thr)
        assert bad.size == 0, ("bin_threshold: float64 restatement", wide, int(bs[bad[0]]), float(scale[bad[0]]),
                               float(fx[bad[0]]), int(thr[bad[0]]), int(want_thr[bad[0]]))


# ---- both builds run every table -----------------------------------------------------------------

CHECKS = (check_select_sizes, check_select_unstaged, check_select_passes, check_select_range,
          check_select_min_score, check_select_flags, check_select_largest, check_conj_threshold,
          check_group_threshold, check_group_verdict, check_conj_hits, check_union, check_bins)


@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__[6:])
def test_select_layer_twin(probe_sim, check):
    if check is check_select_largest:
        check(probe_sim, BIG_TWIN)
    else:
        check(probe_sim)


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__[6:])
def test_select_layer_gpu(probe_gpu, check):
    if check is check_bins:
        check(probe_gpu, "gpu")
    else:
        check(probe_gpu)
