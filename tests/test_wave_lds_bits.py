"""irs_hip::lds_bits32 (csrc/lds_bits.h) — the 32 bits at an LDS offset as an integer, read with
wave::lds_f32 and a bit cast — against one plain statement, on both builds.

In the manner of tests/test_wave_primitives.py: `tests/probe/lds_bits_probe.hip` calls it on
the caller's operands and is built twice — against `tests/sim` (the CPU emulator's wave.h) and against
`iresearch_amd/csrc/hip` (hipcc, gfx950) — so the two headers are pinned to one meaning, inside the
domain the header documents: offsets that are multiples of 4 inside the dynamic LDS block of a kernel
without static `__shared__`.

  * read:  res[i] == the image's 32-bit word at offs[i] (little-endian, as numpy views it), for every
           bit pattern: zeros, denormals, infinities, quiet and signalling NaNs with any payload;
  * mask:  what clauses.h relies on — pass 1 adds 32-bit values to the low words of 64-bit
           accumulators, a barrier, then every thread reads a low word while all threads add
           multiples of 2^16 (64-bit adds) to the accumulators: the low 16 bits read are those pass 1
           left whatever pass 2 has added so far, and the accumulators end as the plain sums.
"""
import ctypes as C
import fcntl
import shlex
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
PROBE = ROOT / "tests" / "probe"
SRC = PROBE / "lds_bits_probe.hip"
SIM_SO = PROBE / "liblds_bits_probe_sim.so"
HIP_SO = PROBE / "liblds_bits_probe_hip.so"
CSRC = ROOT / "iresearch_amd" / "csrc"
THREADS = 1024


def _stale(target: Path, deps) -> bool:
    return not target.exists() or any(d.stat().st_mtime > target.stat().st_mtime for d in deps)


def _locked():
    lock = open(PROBE / ".build.lock", "w")
    fcntl.flock(lock, fcntl.LOCK_EX)   # (pytest-xdist workers: one builds, the others wait)
    return lock


def build_sim() -> Path:
    """The g++ line of tests/sim/build_sim.sh with the probe in place of the product source."""
    with _locked():
        deps = [SRC, CSRC / "lds_bits.h", ROOT / "tests" / "sim" / "sim_switch.S"] + list((ROOT / "tests" / "sim").glob("*.h"))
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
    """hipcc for gfx950 with the flags of iresearch_amd/_build.py (cross-compiles without a GPU)."""
    from iresearch_amd import _build
    with _locked():
        deps = [SRC, CSRC / "lds_bits.h"] + list((CSRC / "hip").glob("*.h"))
        if _stale(HIP_SO, deps):
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


def bind(path: Path):
    P = C.CDLL(str(path))
    u32, vp = C.c_uint32, C.c_void_p
    for name, args in (("lp_arch", [C.c_char_p, C.c_size_t]), ("lp_read", [u32, vp, vp, u32, vp, vp]),
                       ("lp_mask", [u32, vp, vp, vp, vp, vp, vp, vp])):
        fn = getattr(P, name)
        fn.argtypes, fn.restype = args, C.c_int
    return P


@pytest.fixture(scope="module")
def probe_sim():
    P = bind(build_sim())
    buf = C.create_string_buffer(64)
    assert P.lp_arch(buf, 64) == 0 and buf.value == b"gfx950-sim"
    return P


@pytest.fixture(scope="module")
def probe_gpu():
    """The probe on a real GPU; fails (does not skip) without one."""
    import torch  # noqa: F401  (one HIP runtime per process: tests/test_wave_primitives.py)
    P = bind(build_hip())
    buf = C.create_string_buffer(64)
    assert P.lp_arch(buf, 64) == 0, "no usable HIP device"
    assert buf.value.decode().startswith("gfx950"), buf.value
    return P


def ptr(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


# ------------------------------------------------------------------- cases --

def case_read(P):
    """res[i] == img32[offs[i] / 4]: the first and the last word, both halves of 8-byte words, one
    offset many times (a broadcast), a permutation (no two lanes alike), strides that collide on a
    bank."""
    rng = np.random.default_rng(5)
    for nbytes in (4, 64, 4096, 64 * 1024):
        words = nbytes // 4
        img = rng.integers(0, 1 << 32, words, dtype=np.uint64).astype(np.uint32)
        # (patterns a floating-point operation would change: signalling / quiet NaNs, denormals, -0)
        odd = np.array([0x7FA00001, 0xFFA12345, 0x7FC00000, 0x7F800001, 0x00000001, 0x807FFFFF, 0x80000000,
                        0x7F800000], np.uint32)
        img[:min(words, odd.size)] = odd[:words]
        img[0], img[-1] = 0xFFFFFFFF, 0x80000001
        sets = [np.array([0, nbytes - 4], np.uint32), np.full(130, (words // 2) * 4, np.uint32),
                (rng.permutation(words)[:3000] * 4).astype(np.uint32),
                ((np.arange(2048) * 64) % words * 4).astype(np.uint32),
                ((np.arange(2048) * 2 + 1) % words * 4).astype(np.uint32)]
        for offs in sets:
            offs = np.ascontiguousarray(offs)
            res = np.zeros(len(offs), np.uint32)
            flags = np.zeros(2, np.uint32)
            assert P.lp_read(nbytes, ptr(img), ptr(offs), len(offs), ptr(res), ptr(flags)) == 0
            assert flags.tolist() == [1, 0], flags
            assert np.array_equal(res, img[offs // 4]), (nbytes, offs[:8])
    # (outside the domain nothing is read: the probe skips and counts)
    img = np.arange(16, dtype=np.uint32)
    offs = np.array([0, 2, 64, 60], np.uint32)
    res = np.zeros(4, np.uint32)
    flags = np.zeros(2, np.uint32)
    assert P.lp_read(64, ptr(img), ptr(offs), 4, ptr(res), ptr(flags)) == 0
    assert int(flags[1]) == 2 and res[0] == 0 and res[3] == 15


def case_mask(P):
    """The low 16 bits a thread reads in pass 2 are the sum pass 1 left there, whatever the other
    threads have added to the high 48 bits meanwhile; the accumulators end as the plain sums."""
    rng = np.random.default_rng(9)
    for words, spread in ((1, 1), (7, 7), (1024, 1024), (8192, 8192), (8192, 3)):
        # pass 1: 1 << j for 16 `entries` j, at most one per (accumulator, j): no carry out of 16 bits
        a1 = rng.integers(0, spread, THREADS).astype(np.uint32)
        seen = {}
        lo = np.zeros(THREADS, np.uint32)
        for t in range(THREADS):
            n = seen.get(int(a1[t]), 0)
            if n < 16:
                lo[t] = 1 << n
                seen[int(a1[t])] = n + 1
        a2 = rng.integers(0, spread, THREADS).astype(np.uint32)
        hi = rng.integers(0, 1 << 32, THREADS, dtype=np.uint64).astype(np.uint32)
        res = np.zeros(THREADS, np.uint32)
        acc = np.zeros(words, np.uint64)
        flags = np.zeros(2, np.uint32)
        assert P.lp_mask(words, ptr(a1), ptr(lo), ptr(a2), ptr(hi), ptr(res), ptr(acc), ptr(flags)) == 0
        assert flags.tolist() == [1, 0], flags
        low = np.zeros(words, np.uint64)
        np.add.at(low, a1, lo.astype(np.uint64))
        assert int(low.max()) <= 0xFFFF
        assert np.array_equal(res & 0xFFFF, low[a2].astype(np.uint32)), (words, spread)
        want = low.copy()
        np.add.at(want, a2, hi.astype(np.uint64) << np.uint64(16))
        assert np.array_equal(acc, want), (words, spread)


def test_lds_bits_read_emulated(probe_sim):
    case_read(probe_sim)


def test_lds_bits_mask_emulated(probe_sim):
    case_mask(probe_sim)


@pytest.mark.gpu
def test_lds_bits_read_gpu(probe_gpu):
    case_read(probe_gpu)


@pytest.mark.gpu
def test_lds_bits_mask_gpu(probe_gpu):
    case_mask(probe_gpu)
