"""The wavefront primitives (`wave::`) against one plain statement each, on both builds.

Every kernel of the library is written against `wave::` and `rt::`; the product compiles them
against `iresearch_amd/csrc/hip/{wave,gpu_rt}.h`, the CPU tier against the same-named twins in
`tests/sim`.  `tests/probe/wave_probe.hip` calls every primitive on the caller's operands and is
built both ways here (fixtures below); each family has ONE statement in numpy (uint64 / float64,
written from the header's comment) and ONE case table, run through the twin on the CPU and through
`hip/wave.h` on the GPU — so the two headers are pinned to one meaning, inside the domains the
header documents:

  * cross-lane operations: all 64 lanes of the wavefront active (what every kernel guarantees at
    its call sites); lane / source indices 0..63 and wave-uniform;
  * `mul24`: operands below 2^24; `funnel`: s in 0..31; `bfe`: 1 <= bits <= 31;
  * `fast_rcp` on [1, 2^25], `fast_sqrt` on [1, 2^32): at most 1 ulp from the correctly rounded
    result (the header's claim; the scores' 1e-5 budget rests on it);
  * the 16-byte LDS operations: offsets that are multiples of 16 inside the dynamic block of a
    kernel without static `__shared__`; `gload_*`: 4-byte aligned offsets, unsigned 32-bit.

Outside these domains nothing is stated and nothing is tested.
"""
import ctypes as C
import fcntl
import os
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
SRC = PROBE / "wave_probe.hip"
SIM_SO = PROBE / "libwave_probe_sim.so"
HIP_SO = PROBE / "libwave_probe_hip.so"
HIP_ASM = PROBE / "wave_probe_gfx950.s"
CSRC = ROOT / "iresearch_amd" / "csrc"

M32 = np.uint64(0xFFFFFFFF)
BORDERS = (0, 15, 16, 31, 32, 47, 48, 63)   # every lane a row_shr / row_bcast step crosses
LANES_K = (0, 31, 32, 63)
NONE = 0xFFFFFFFF


# ------------------------------------------------------------------ builds --

def _stale(target: Path, deps) -> bool:
    return not target.exists() or any(d.stat().st_mtime > target.stat().st_mtime for d in deps)


def _locked():
    lock = open(PROBE / ".build.lock", "w")
    fcntl.flock(lock, fcntl.LOCK_EX)   # (pytest-xdist workers: one builds, the others wait)
    return lock


def build_sim() -> Path:
    """The g++ line of tests/sim/build_sim.sh with the probe in place of the product source."""
    with _locked():
        deps = [SRC, CSRC / "types.h", ROOT / "tests" / "sim" / "sim_switch.S"] + \
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


def bind(path: Path):
    P = C.CDLL(str(path))
    u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
    for name, args in (("wp_arch", [C.c_char_p, C.c_size_t]),
                       ("wp_crosslane", [vp, vp, vp, u32, u32, u32, u32, u32, vp]),
                       ("wp_integer", [vp, u32, vp]), ("wp_float", [vp, u32, vp]),
                       ("wp_lds", [C.c_int, u32, vp, vp, vp, vp, vp]), ("wp_sync", [vp, u32, vp]),
                       ("wp_sload_size", [C.c_int]), ("wp_sload_align", [C.c_int]),
                       ("wp_sload", [C.c_int, vp, u64, u32, vp]), ("wp_gload", [vp, u64, vp, u32, vp]),
                       ("wp_gload_far", [vp, u32, vp, vp, vp]), ("wp_unaligned", [vp, vp])):
        fn = getattr(P, name)
        fn.argtypes, fn.restype = args, C.c_int
    return P


@pytest.fixture(scope="module")
def probe_sim():
    """The probe against tests/sim: the twin header on the CPU fiber emulator."""
    P = bind(build_sim())
    buf = C.create_string_buffer(64)
    assert P.wp_arch(buf, 64) == 0 and buf.value == b"gfx950-sim"
    return P


@pytest.fixture(scope="module")
def probe_gpu():
    """The probe against iresearch_amd/csrc/hip on a real GPU; fails (does not skip) without one."""
    # One HIP runtime per process (as iresearch_amd/_lib.py does it): torch bundles its own
    # libamdhip64 of the same SONAME; loaded first, the probe and the product library share it
    # with the tests that hand torch tensors to the library later in the same process.
    import torch  # noqa: F401
    P = bind(build_hip())
    buf = C.create_string_buffer(64)
    assert P.wp_arch(buf, 64) == 0, "no usable HIP device"
    assert buf.value.decode().startswith("gfx950"), buf.value
    return P


def ptr(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def measured(line: str):
    """A measurement (not an assertion): printed, and appended to the file IRS_WAVE_PROFILE names."""
    print(line)
    path = os.environ.get("IRS_WAVE_PROFILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# -------------------------------------------------------------- cross-lane --

def state_crosslane(a, b, salt, k, x, diverge):
    """All 64 lanes active.  Lane l of a wavefront w holds a[w][l], b[w][l]."""
    a0, b0 = a.reshape(-1, 64), b.reshape(-1, 64)
    a, b = a.astype(np.uint64), b.astype(np.uint64)
    if diverge:   # what the branch in front of the primitives did to the operands
        odd = (np.arange(a.size) & 1) == 1
        a = np.where(odd, a ^ salt, a)
        b = np.where(odd, b, (b + salt) & M32)
    A, B = a.reshape(-1, 64), b.reshape(-1, 64)
    n_w = A.shape[0]
    col = lambda v: np.repeat(np.asarray(v, np.uint64).reshape(n_w, 1), 64, axis=1)
    out = np.zeros((n_w, 64, 16), np.uint64)
    out[:, :, 0] = np.cumsum(A, axis=1) & M32                      # inclusive_scan
    out[:, :, 1] = out[:, :, 0]                                    # inclusive_scan2: first chain
    out[:, :, 2] = np.cumsum(B, axis=1) & M32                      # ... and the second
    out[:, :, 3] = col(A.sum(axis=1) & M32)                        # reduce_add
    out[:, :, 4] = col(A.max(axis=1))                              # reduce_max
    out[:, :, 5] = col(A[:, k])                                    # bcast
    ballot = ((B & np.uint64(1)) << np.arange(64, dtype=np.uint64)).sum(axis=1)
    out[:, :, 6] = col(ballot & M32)                               # ballot: bit l = lane l's predicate
    out[:, :, 7] = col(ballot >> np.uint64(32))
    out[:, :, 8] = col(A[:, k])                                    # read_lane
    out[:, :, 9] = col(B[:, k])                                    # read_lane_f: the same 32 bits
    W = A.copy()
    W[:, k] = x
    out[:, :, 10] = W                                              # write_lane: lane k alone changes
    u = a0[:, 0].astype(np.uint64) ^ b0[:, 63].astype(np.uint64)
    out[:, :, 11] = col(u)                                         # uniform
    out[:, :, 12] = col(a0[:, 63])                                 # uniform64, low word
    out[:, :, 13] = col(b0[:, 0])                                  # ... high word
    out[:, :, 14] = col(u)                                         # uniform_f: the same 32 bits
    out[:, :, 15] = np.arange(64, dtype=np.uint64)[None, :]        # lane_id
    return out.reshape(-1, 16).astype(np.uint32)


def crosslane_cases():
    """(name, a, b) for 16 wavefronts with different data each."""
    rng = np.random.default_rng(64)
    n = 1024
    rnd = lambda: rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    lane = np.arange(n, dtype=np.uint32) & 63
    wavef = np.arange(n, dtype=np.uint32) >> 6
    yield "random (sums wrap 2^32)", rnd() | np.uint32(0x80000000), rnd()
    yield "all ones | ballot all", np.ones(n, np.uint32), np.ones(n, np.uint32) | (rnd() << 1)
    yield "all 0xFFFFFFFF | ballot none", np.full(n, 0xFFFFFFFF, np.uint32), rnd() & np.uint32(0xFFFFFFFE)
    yield "random | ballot alternating", rnd(), (lane + wavef) & 1
    for l in BORDERS:
        a = np.where(lane == l, rnd() | np.uint32(1), 0).astype(np.uint32)
        b = np.where(lane == 63 - l, rnd() | np.uint32(1), 0).astype(np.uint32)   # l = 0: bit 63 alone
        yield "single non-zero at lane %d" % l, a, b


NANS = (0x7FA00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF)   # signalling / quiet, payloads kept bit for bit


def check_crosslane(P):
    rng = np.random.default_rng(7)
    runs = 0
    for ci, (name, a, b) in enumerate(crosslane_cases()):
        for block in (64, 1024):
            for diverge in (0, 1):
                ks = LANES_K if ci == 0 else (LANES_K[(ci + runs) % 4],)
                for k in ks:
                    b = b.copy()
                    if ci == 0:
                        b[k::64] = np.resize(np.array(NANS, np.uint32), 16)
                    salt = rng.integers(0, 2**32, a.size, dtype=np.uint64).astype(np.uint32)
                    x = int(rng.integers(0, 2**32))
                    out = np.zeros((a.size, 16), np.uint32)
                    rc = P.wp_crosslane(ptr(a), ptr(b), ptr(salt), a.size, block, k, x, diverge, ptr(out))
                    assert rc == 0, (name, rc)
                    want = state_crosslane(a, b, salt, k, x, diverge)
                    bad = np.argwhere(out != want)
                    assert bad.size == 0, (name, "block", block, "diverge", diverge, "k", k,
                                           "thread, output:", bad[0], hex(out[tuple(bad[0])]),
                                           hex(want[tuple(bad[0])]))
                    runs += 1
    assert runs == (16 + 11 * 4)


def test_crosslane_twin(probe_sim):
    check_crosslane(probe_sim)


@pytest.mark.gpu
def test_crosslane_gpu(probe_gpu):
    check_crosslane(probe_gpu)


# ----------------------------------------------------------------- integer --

def state_integer(x):
    x = x.astype(np.uint64)
    lo16, hi16 = lambda v: v & np.uint64(0xFFFF), lambda v: (v >> np.uint64(16)) & np.uint64(0xFFFF)
    pack = lambda h, l: ((h & np.uint64(0xFFFF)) << np.uint64(16)) | (l & np.uint64(0xFFFF))
    nz = lambda v: (v != 0).astype(np.uint64)
    r = np.zeros((10, x.shape[1]), np.uint64)
    r[0] = (x[0] * x[1]) & M32                                           # mul24: low 32 bits of the product
    r[1] = (x[2] * x[3]) >> np.uint64(32)                                # mul_hi
    r[2] = (((x[2] << np.uint64(32)) | x[3]) >> x[4]) & M32              # funnel(hi, lo, s)
    r[3] = x[2] & ((np.uint64(1) << x[5]) - np.uint64(1))                # bfe: the low `bits` bits
    r[4] = pack(np.minimum(hi16(x[2]), hi16(x[3])), np.minimum(lo16(x[2]), lo16(x[3])))
    r[5] = pack(np.maximum(hi16(x[2]), hi16(x[3])), np.maximum(lo16(x[2]), lo16(x[3])))
    r[6] = pack(hi16(x[2]) + hi16(x[3]), lo16(x[2]) + lo16(x[3]))        # each half wraps by itself
    r[7] = (x[6] + nz(x[2]) + nz(x[3]) + nz(x[0]) + nz(x[1])) & M32      # count_nonzero4, 32-bit values
    r[8] = (x[6] + nz(x[2] | x[3]) + nz(x[0] | x[1]) + nz(x[3]) + nz(x[1])) & M32   # ... 64-bit values
    r[9] = pack(hi16(x[7]) + nz(hi16(x[2])) + nz(hi16(x[3])) + nz(hi16(x[0])) + nz(hi16(x[1])),
                lo16(x[7]) + nz(lo16(x[2])) + nz(lo16(x[3])) + nz(lo16(x[0])) + nz(lo16(x[1])))
    return r.astype(np.uint32)


EDGE32 = (0, 1, 0xFFFF, 0x10000, 0xFFFF0000, 0xFFFFFFFF, 0x8000, 0x80000000, 0x7FFF7FFF, 0x0001FFFF,
          0xFFFF0001, 0x80008000)
EDGE24 = (0, 1, 0xFFFF, 0x10000, 0xFF0000, 0xFFFFFF, 0x800000, 0xFFF001)
EDGE_ACC = (0, 0xFFFBFFFB, 0xFFFB0000, 0x0000FFFB, 0xFFFCFFFF, 0xFFFFFFFC, 0x12345678)


def integer_cases():
    rng = np.random.default_rng(24)
    rows = []
    i = 0
    for e2 in EDGE32:                  # every edge pair at every shift; every edge at every width
        for j3, e3 in enumerate(EDGE32):
            for s in range(32):
                rows.append((EDGE24[i % 8], EDGE24[(i // 8) % 8], e2, e3, s, 1 + (j3 * 32 + s) % 31,
                             EDGE_ACC[i % 7], EDGE_ACC[(i // 3) % 7]))
                i += 1
    for a in EDGE24:                   # mul24 at its operands' ends: products beyond 2^32
        for b in EDGE24:
            rows.append((a, b, 0, 0, 0, 1, 0, 0))
    x = np.array(rows, np.uint64).T
    n = 8192
    r = rng.integers(0, 2**32, (8, n), dtype=np.uint64)
    r[0] &= np.uint64(0xFFFFFF)
    r[1] &= np.uint64(0xFFFFFF)
    r[0, ::5] |= np.uint64(0xFF0000)   # (large operands: the product passes 2^32)
    r[1, ::5] |= np.uint64(0xFF0000)
    r[4] = np.arange(n) % 32
    r[5] = 1 + (np.arange(n) // 32) % 31
    # halves that are zero in some of the counted values, accumulator halves close to wrapping
    r[2, 1::4] &= np.uint64(0xFFFF)
    r[3, 2::4] &= np.uint64(0xFFFF0000)
    r[0, 3::8] = 0
    r[7, ::3] |= np.uint64(0xFFF8FFF8)
    x = np.concatenate([x, r], axis=1)
    assert int((x[0] * x[1]).max()) > 2**32 and int(x[0].max()) == 2**24 - 1
    assert set(np.unique(x[4])) == set(range(32)) and set(np.unique(x[5])) == set(range(1, 32))
    return np.ascontiguousarray(x.astype(np.uint32))


INT_NAMES = ("mul24", "mul_hi", "funnel", "bfe", "pk_min_u16", "pk_max_u16", "pk_add_u16",
             "count_nonzero4 (u32)", "count_nonzero4 (u64)", "count_nonzero_halves4")


def check_integer(P):
    x = integer_cases()
    n = x.shape[1]
    out = np.zeros((10, n), np.uint32)
    assert P.wp_integer(ptr(x), n, ptr(out)) == 0
    want = state_integer(x)
    for j, name in enumerate(INT_NAMES):
        bad = np.flatnonzero(out[j] != want[j])
        assert bad.size == 0, (name, "operands", [hex(int(v)) for v in x[:, bad[0]]],
                               "got", hex(int(out[j, bad[0]])), "want", hex(int(want[j, bad[0]])))


def test_integer_twin(probe_sim):
    check_integer(probe_sim)


@pytest.mark.gpu
def test_integer_gpu(probe_gpu):
    check_integer(probe_gpu)


# ------------------------------------------------------------------- float --

def _pow2_neighbours(lo_exp, hi_exp, lo, hi):
    p = np.float32(2.0) ** np.arange(lo_exp, hi_exp + 1, dtype=np.float32)
    v = np.concatenate([p, np.nextafter(p, np.float32(0)), np.nextafter(p, np.float32(np.inf))])
    return v[(v >= lo) & (v <= hi)].astype(np.float32)


def float_cases():
    """rcp operands in [1, 2^25] (1 + tf * inv), sqrt operands in [1, 2^32) (tf): 2^20 random values
    each (half of them uniform in the exponent, half uniform in the value), every power of two of
    the range and its two neighbours; fma operands whose product needs more than 24 bits and
    cancels against c."""
    rng = np.random.default_rng(1)
    half = 1 << 19

    def sample(top):
        a = np.exp2(rng.uniform(0, top, half))
        b = rng.uniform(1.0, 2.0 ** top, half)
        v = np.concatenate([a, b]).astype(np.float32)
        return np.clip(v, np.float32(1), np.nextafter(np.float32(2.0 ** top), np.float32(0)))

    rcp = np.concatenate([sample(25), _pow2_neighbours(0, 25, 1.0, 2.0 ** 25)])
    sq = np.concatenate([sample(32), _pow2_neighbours(0, 32, 1.0, np.nextafter(np.float32(2.0 ** 32), np.float32(0)))])
    n = max(rcp.size, sq.size)
    rcp, sq = np.resize(rcp, n), np.resize(sq, n)
    fa = rng.uniform(1.0, 2.0, n).astype(np.float32)
    fb = rng.uniform(1.0, 2.0, n).astype(np.float32)
    fa[0], fb[0] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)
    fc = -(fa * fb)            # the float32 product: the fused result is its rounding error, exactly
    r = rng.uniform(-4.0, 4.0, fc[1::2].size).astype(np.float32)
    fc[1::2] = np.where(np.abs(r) < 2.0 ** -20, np.float32(1.5), r)
    return np.ascontiguousarray(np.stack([rcp, sq, fa, fb, fc]).astype(np.float32))


def ulps(got, want):
    """Distance in units of the last place between positive finite float32 values."""
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


def check_float(P, tag):
    x = float_cases()
    n = x.shape[1]
    out = np.zeros((3, n), np.float32)
    assert P.wp_float(ptr(x), n, ptr(out)) == 0
    x64 = x.astype(np.float64)
    for j, name, want in ((0, "fast_rcp", (1.0 / x64[0]).astype(np.float32)),
                          (1, "fast_sqrt", np.sqrt(x64[1]).astype(np.float32))):
        e = ulps(out[j], want)
        w = int(np.argmax(e))
        measured("%s %s: largest error %d ulp at operand %r (0x%08x) over %d operands; %d of them off by one"
                 % (tag, name, int(e[w]), float(x[j, w]), int(x[j, w:w + 1].view(np.uint32)[0]), n,
                    int((e == 1).sum())))
        assert int(e[w]) <= 1, (name, float(x[j, w]), float(out[j, w]), float(want[w]))
    # a * b is exact in float64 (48 bits below 4), and so is the sum with c (|c| in [2^-20, 4): at
    # most 53 bits from 2^2 down): float64 -> float32 is the ONE rounding of a fused multiply-add
    want = (x64[2] * x64[3] + x64[4]).astype(np.float32)
    unfused = (x[2] * x[3]) + x[4]
    differ = unfused.view(np.uint32) != want.view(np.uint32)
    assert differ.sum() > n // 8, "the cases must tell a fused from an unfused multiply-add"
    bad = np.flatnonzero(out[2].view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, ("fma", [float(v) for v in x[2:5, bad[0]]], float(out[2, bad[0]]), float(want[bad[0]]))
    assert out[2, 0] == np.float32(2.0 ** -24)


def test_float_twin(probe_sim):
    check_float(probe_sim, "emulator")


@pytest.mark.gpu
def test_float_gpu(probe_gpu):
    check_float(probe_gpu, "gfx950")


# --------------------------------------------------------------------- LDS --

LDS_U8, LDS_F32, LDS_ADD32, LDS_ADD64, LDS_READ4, LDS_ZERO4, LDS_TAKE4, LDS_TAKE4X2, LDS_TAKE4X3 = range(9)
LDS_WIDTH = {LDS_U8: 1, LDS_F32: 4, LDS_READ4: 16, LDS_ZERO4: 16, LDS_TAKE4: 16}


def _constants():
    """constexpr uint32_t NAME = <integer expression>; of the kernel headers."""
    env = {}
    for h in ("types.h", "kernels.h", "score.h", "join.h"):
        for name, expr in re.findall(r"constexpr\s+uint32_t\s+(\w+)\s*=\s*([^;]+);", (CSRC / h).read_text()):
            env.setdefault(name, expr)
    return env


def _record_sizes():
    sizes = {}
    for h in ("types.h", "lead.h", "phrase.h", "join.h"):
        for name, n in re.findall(r"static_assert\(sizeof\((\w+)\)\s*==\s*(\d+)", (CSRC / h).read_text()):
            sizes[name] = int(n)
    # (no static_assert in types.h for these: what the probe compiled, test_probe_records_... compares)
    sizes.update(BlkDir=16, DevQTerm=32, DevTail=40)
    return sizes


def join_score_lds_bytes() -> int:
    """JoinOff::end of join.h: the dynamic LDS block launch_join_score asks for (the largest
    block addressed absolutely), evaluated from the source."""
    text = (CSRC / "join.h").read_text()
    body = re.search(r"struct JoinOff \{(.*?)\n\};", text, flags=re.S).group(1)
    env, sizes = _constants(), _record_sizes()
    assert "JoinOff::end" in (CSRC / "plan_join.h").read_text()

    def value(expr, scope):
        expr = re.sub(r"uint32_t\(sizeof\((\w+)\)\)", lambda m: str(sizes[m.group(1)]), expr)
        expr = re.sub(r"\b(\d+)u\b", r"\1", expr)
        names = set(re.findall(r"[A-Za-z_]\w*", expr))
        return int(eval(expr, {"__builtins__": {}},
                        {k: (scope[k] if k in scope else value(env[k], {})) for k in names}))

    scope = {}
    for name, expr in re.findall(r"static constexpr uint32_t (\w+)\s*=\s*([^;]+);", body):
        scope[name] = value(expr, scope)
    return scope["end"]


def state_lds(op, img, par):
    """Every thread's operands name lines of their own (or the operation commutes): the
    operations take effect one thread after the other.  Returns (results [1024][12], image after)."""
    after = img.copy()
    by = after.view(np.uint8)
    res = np.zeros((1024, 12), np.uint32)
    for t in range(1024):
        p = [int(v) for v in par[t]]
        if p[0] == NONE:
            continue
        if op == LDS_U8:
            res[t, 0] = by[p[0]]
        elif op == LDS_F32:
            res[t, 0] = after[p[0] // 4]
        elif op == LDS_ADD32:
            after[p[0] // 4] = (int(after[p[0] // 4]) + p[1]) & 0xFFFFFFFF
        elif op == LDS_ADD64:
            w = after[p[0] // 4:p[0] // 4 + 2].view(np.uint64)
            w[0] = (int(w[0]) + (p[2] << 32 | p[1])) & 0xFFFFFFFFFFFFFFFF
        elif op == LDS_READ4:
            res[t, 0:4] = after[p[0] // 4:p[0] // 4 + 4]
        elif op == LDS_ZERO4:
            after[p[0] // 4:p[0] // 4 + 4] = 0
        else:   # take4 / x2 / x3: the 16 bytes that were there, zeros left behind
            for j in range(op - LDS_TAKE4 + 1):
                res[t, 4 * j:4 * j + 4] = after[p[j] // 4:p[j] // 4 + 4]
                after[p[j] // 4:p[j] // 4 + 4] = 0
    return res, after


def lds_cases(nbytes):
    """(name, op, par [1024][4]); nbytes = the joined score kernel's block, 48 KB = its accumulator tile."""
    rng = np.random.default_rng(3)
    t = np.arange(1024, dtype=np.uint64)
    tile_last, last = 48 * 1024 - 16, nbytes - 16
    lines = nbytes // 16

    def par(p0, p1=None, p2=None, p3=None):
        cols = [np.asarray(c if c is not None else np.zeros(1024), np.uint64) for c in (p0, p1, p2, p3)]
        return np.ascontiguousarray(np.stack(cols, axis=1).astype(np.uint32))

    def sparse(*offsets):   # a few lanes of different wavefronts, everyone else idle
        p = np.full((1024, 4), NONE, np.uint32)
        for lane, offs in zip((0, 64, 1, 1023, 65, 512), offsets):
            p[lane, :len(offs)] = offs
        return p

    r32 = lambda: rng.integers(0, 2**32, 1024, dtype=np.uint64)
    o = (t * 37 + 5) % nbytes
    o[-1] = nbytes - 1
    yield "lds_u8", LDS_U8, par(o)
    o = ((t * 101 + 3) % (nbytes // 4)) * 4
    o[-1] = nbytes - 4
    yield "lds_f32", LDS_F32, par(o)
    yield "lds_add u32, one address", LDS_ADD32, par(np.full(1024, 64), r32())
    yield "lds_add u32, one bank", LDS_ADD32, par((t % 8) * 256 + 1024, r32())
    yield "lds_add u64, one address", LDS_ADD64, par(np.full(1024, last + 8), r32(), r32())
    yield "lds_add u64, one bank", LDS_ADD64, par((t % 8) * 256 + 2048, r32(), r32())
    perm = rng.permutation(lines)[:1024].astype(np.uint64)
    perm[:4] = (0, 1, tile_last // 16, last // 16)
    yield "lds_read4", LDS_READ4, par(perm * 16)
    yield "lds_zero4, corners", LDS_ZERO4, sparse((0,), (16,), (tile_last,), (last,))
    yield "lds_zero4, every other line", LDS_ZERO4, par(t * 32)
    yield "lds_take4, corners", LDS_TAKE4, sparse((0,), (16,), (tile_last,), (last,))
    yield "lds_take4, 1024 scattered lines", LDS_TAKE4, par((rng.permutation(lines // 3)[:1024].astype(np.uint64) * 3 + 1) * 16)
    yield "lds_take4x2, corners", LDS_TAKE4X2, sparse((0, 16), (tile_last, last), (last - 16, 32))
    yield "lds_take4x2, adjacent", LDS_TAKE4X2, par(t * 48, t * 48 + 16)
    g = (t // 16) * 512 + (t % 16) * 16
    yield "lds_take4x2, equal banks", LDS_TAKE4X2, par(g, g + 256)
    yield "lds_take4x3, corners", LDS_TAKE4X3, sparse((0, 16, 32), (tile_last, last, tile_last - 16), (last - 16, last - 32, 48))
    yield "lds_take4x3, adjacent", LDS_TAKE4X3, par(t * 64, t * 64 + 16, t * 64 + 32)
    g = (t // 16) * 768 + (t % 16) * 16
    yield "lds_take4x3, equal banks", LDS_TAKE4X3, par(g, g + 256, g + 512)


def check_lds(P, tag):
    nbytes = join_score_lds_bytes()
    assert 48 * 1024 < nbytes <= 160 * 1024 and nbytes % 16 == 0, nbytes
    img = np.random.default_rng(5).integers(1, 2**32, nbytes // 4, dtype=np.uint64).astype(np.uint32)
    for name, op, par in lds_cases(nbytes):
        if op >= LDS_ZERO4:   # the statement is sequential: the lines must be distinct
            offs = par[:, :max(1, op - LDS_TAKE4 + 1)]
            offs = offs[par[:, 0] != NONE].ravel()
            assert np.unique(offs).size == offs.size and int(offs.max()) <= nbytes - 16, name
        res = np.zeros((1024, 12), np.uint32)
        after = np.zeros_like(img)
        flags = np.zeros(2, np.uint32)
        rc = P.wp_lds(op, nbytes, ptr(img), ptr(par), ptr(res), ptr(after), ptr(flags))
        assert rc != -4, "lds_is_at_zero() does not hold in a kernel without static __shared__"
        assert rc == 0, (name, rc, "lds_is_at_zero: %d, operands out of the block: %d" % tuple(flags))
        want_res, want_after = state_lds(op, img, par)
        bad = np.argwhere(res != want_res)
        assert bad.size == 0, (name, "thread, word", bad[0], hex(res[tuple(bad[0])]), hex(want_res[tuple(bad[0])]))
        bad = np.flatnonzero(after != want_after)
        assert bad.size == 0, (name, "LDS byte offset", int(bad[0]) * 4, hex(after[bad[0]]), hex(want_after[bad[0]]))
    measured("%s lds_is_at_zero (kernel without static __shared__, %d bytes of dynamic LDS): %d"
             % (tag, nbytes, int(flags[0])))


def test_lds_twin(probe_sim):
    check_lds(probe_sim, "emulator")


@pytest.mark.gpu
def test_lds_gpu(probe_gpu):
    check_lds(probe_gpu, "gfx950")


def test_join_score_lds_bytes_is_read_from_the_code():
    assert join_score_lds_bytes() == 4 * 12288 + 256 + 2 * 32 * 16 + 4 * 65 * 16 + 4 * 64 * 16 + 128 + 4096 + 64 + 16384


# -------------------------------------------------------------- wave::sync --

def check_sync(P):
    rng = np.random.default_rng(9)
    for threads in (64, 1024):
        x = rng.integers(0, 2**32, (8, threads), dtype=np.uint64).astype(np.uint32)
        out = np.zeros_like(x)
        assert P.wp_sync(ptr(x), threads, ptr(out)) == 0
        want = x.reshape(8, -1, 64)[:, :, ::-1].reshape(8, threads)   # slot 63 - lane of the SAME round
        assert np.array_equal(out, want), np.argwhere(out != want)[0]


def test_sync_twin(probe_sim):
    check_sync(probe_sim)


@pytest.mark.gpu
def test_sync_gpu(probe_gpu):
    check_sync(probe_gpu)


# ------------------------------------------------------------------- loads --

SLOAD_TYPES = ("BlkDir", "ConjItem", "DevQuery", "DevQTerm", "DevTail", "StreamRec", "JoinWg")


def test_probe_records_have_the_kernels_shapes(probe_sim):
    """sload<T> sees T's size and alignment only; ConjItem / StreamRec / JoinWg are stand-ins in
    the probe (their headers carry kernels): both numbers against the declarations."""
    sizes = _record_sizes()
    text = "".join((CSRC / h).read_text() for h in ("types.h", "lead.h", "phrase.h", "join.h"))
    for i, name in enumerate(SLOAD_TYPES):
        assert probe_sim.wp_sload_size(i) == sizes[name], name
        assert re.search(r"struct (alignas\(\d+\) )?%s \{" % name, text), name
        m = re.search(r"struct alignas\((\d+)\) %s \{" % name, text)
        if m:
            assert probe_sim.wp_sload_align(i) == int(m.group(1)), name
        else:
            assert name in ("DevQuery", "DevQTerm", "DevTail")   # the probe compiles types.h itself
    assert sorted(sizes[n] for n in SLOAD_TYPES) == [16, 32, 32, 40, 64, 64, 128]


def check_loads(P):
    rng = np.random.default_rng(12)
    n_recs = 50_000
    for ti, name in enumerate(SLOAD_TYPES):
        size = P.wp_sload_size(ti)
        recs = rng.integers(0, 256, (n_recs, size), dtype=np.uint8)
        for index in (0, 1, n_recs - 1):
            out = np.zeros(size, np.uint8)
            assert P.wp_sload(ti, ptr(recs), n_recs, index, ptr(out)) == 0, name
            assert np.array_equal(out, recs[index]), (name, index, np.flatnonzero(out != recs[index]))
    # gload_*: offsets 0, 4, 8, 12 (4-byte aligned, not 16), the last 16 bytes, scattered per lane
    nbytes = 1 << 20
    buf = rng.integers(0, 256, nbytes, dtype=np.uint8)
    offs = (rng.integers(0, (nbytes - 16) // 4, 1024, dtype=np.uint64) * 4).astype(np.uint32)
    offs[:5] = (0, 4, 8, 12, nbytes - 16)
    out = np.zeros((1024, 11), np.uint32)
    assert P.wp_gload(ptr(buf), nbytes, ptr(offs), 1024, ptr(out)) == 0
    check_gload(out, state_gload(lambda o: buf[o:o + 16], offs), offs)
    # load_u64 / load_u32 at every byte alignment, global memory and LDS
    line = rng.integers(0, 256, 32, dtype=np.uint8)
    out = np.zeros((16, 6), np.uint32)
    assert P.wp_unaligned(ptr(line), ptr(out)) == 0
    for a in range(16):
        w = [int.from_bytes(line[a + 4 * j:a + 4 * j + 4].tobytes(), "little") for j in (0, 1)]
        assert [int(v) for v in out[a]] == [w[0], w[1], w[0]] * 2, a


def state_gload(read16, offs):
    """gload_u32 | gload_u64 | gload_u32x4 | gload_u32x4_at: the 4 / 8 / 16 / 16 bytes at base + off,
    off an UNSIGNED 32-bit number, little-endian words."""
    want = np.zeros((offs.size, 11), np.uint32)
    for i, o in enumerate(offs):
        w = np.frombuffer(bytes(read16(int(o))), np.uint32)
        want[i] = np.concatenate([w[:1], w[:2], w, w])
    return want


GLOAD_WORDS = ("gload_u32",) + ("gload_u64",) * 2 + ("gload_u32x4",) * 4 + ("gload_u32x4_at",) * 4


def check_gload(out, want, offs):
    bad = np.argwhere(out != want)
    assert bad.size == 0, (GLOAD_WORDS[bad[0][1]], "lane", int(bad[0][0]), "offset", hex(int(offs[bad[0][0]])),
                           hex(int(out[tuple(bad[0])])), hex(int(want[tuple(bad[0])])))


def test_loads_twin(probe_sim):
    check_loads(probe_sim)


@pytest.mark.gpu
def test_loads_gpu(probe_gpu):
    check_loads(probe_gpu)


@pytest.mark.gpu
def test_gload_offsets_with_bit_31_gpu(probe_gpu):
    """Lane offsets 0x7FFFFFF0, 0x80000000, 0x80000010 on a buffer of 2 GiB + 64 KiB: the offset is
    not sign-extended (the probe keeps mapped memory with other words where a signed offset would
    land, so a wrong address is a wrong value)."""
    rng = np.random.default_rng(31)
    offs = (np.arange(64, dtype=np.uint64) * 48).astype(np.uint32)
    offs[[0, 31, 63]] = (0x7FFFFFF0, 0x80000000, 0x80000010)
    offs[[5, 40]] = (0x8000FFF0, 0x7FFFFFE0 - 16)
    patches = rng.integers(0, 2**32, (64, 4), dtype=np.uint64).astype(np.uint32)
    decoys = ~patches
    out = np.zeros((64, 11), np.uint32)
    assert probe_gpu.wp_gload_far(ptr(offs), 64, ptr(patches), ptr(decoys), ptr(out)) == 0
    where = {int(o): i for i, o in enumerate(offs)}
    check_gload(out, state_gload(lambda o: patches[where[o]].tobytes(), offs), offs)


# ------------------------------------------- the GPU build, checked without a GPU --

def _kernels(asm: str):
    """{mangled kernel name: its instructions}, comment lines dropped."""
    out = {}
    for m in re.finditer(r"^(_ZN5probe\w+):.*?\n(.*?)s_endpgm", asm, flags=re.S | re.M):
        out[m.group(1)] = "\n".join(l for l in m.group(2).splitlines() if not l.lstrip().startswith(";"))
    return out


def test_probe_cross_compiles_for_gfx950_in_the_promised_forms():
    """Compile only (no GPU): the GPU build of the probe cannot rot between GPU visits, and the
    generated ISA has the forms hip/wave.h promises and the kernels' timing depends on."""
    so = build_hip()
    data = so.read_bytes()
    assert b"gfx950" in data
    for other in (b"gfx90a", b"gfx942", b"gfx1100", b"sm_"):
        assert other not in data, other
    K = _kernels(HIP_ASM.read_text())
    one = lambda key: [v for k, v in K.items() if key in k]
    sizes = dict(zip(SLOAD_TYPES, (16, 32, 64, 32, 40, 64, 128)))
    shapes = {"ConjItem": "ConjItemShape", "StreamRec": "StreamRecShape", "JoinWg": "JoinWgShape"}
    for name, size in sizes.items():
        (body,) = [v for k, v in K.items() if "k_sloadI" in k and shapes.get(name, name) + "E" in k]
        # sload<T>: the record arrives in SGPRs through s_load_dword*: its bytes on top of the
        # kernel's 20 argument bytes
        got = sum(4 * int(w or 1) for w in re.findall(r"s_load_dword(?:x(\d+))?\s", body))
        assert got >= size + 20, (name, got)
    (g,) = one("k_gloadILb0")
    # gload_u32 / _u64 / _u32x4: (SGPR base) + (32-bit VGPR offset), the saddr form
    assert re.search(r"global_load_dword\s+v\d+, v\d+, s\[\d+:\d+\]", g)
    assert re.search(r"global_load_dwordx2\s+v\[\d+:\d+\], v\d+, s\[\d+:\d+\]", g)
    assert re.search(r"global_load_dwordx4\s+v\[\d+:\d+\], v\d+, s\[\d+:\d+\]", g)
    (at,) = one("k_gloadILb1")
    assert re.search(r"global_load_dwordx4\s", at)
    assert "flat_load" not in g and "flat_load" not in at
    for op, count in ((LDS_TAKE4, 1), (LDS_TAKE4X2, 2), (LDS_TAKE4X3, 3)):
        (body,) = one("k_ldsILi%dE" % op)
        assert body.count("ds_wrxchg2_rtn_b64") == count, op   # ONE pass of the LDS pipeline per 16 bytes
    (i,) = one("k_integer")
    for ins in ("v_alignbit_b32", "v_bfe_u32", "v_mul_u32_u24", "v_mul_hi_u32", "v_pk_min_u16", "v_pk_max_u16",
                "v_pk_add_u16", "v_add3_u32"):
        assert ins in i, ins
    (x,) = one("k_crosslane")
    for ins in ("row_shr:1 ", "row_shr:8 ", "row_bcast:15", "row_bcast:31", "v_readlane_b32", "v_writelane_b32",
                "v_readfirstlane_b32"):
        assert ins in x, ins
    (f,) = one("k_float")
    assert "v_rcp_f32" in f and "v_sqrt_f32" in f and re.search(r"v_fmac?_f32", f)
