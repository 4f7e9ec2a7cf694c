"""The C++ host layer's QueryBatch::nested_sets / nested_topk (irs_hip_batch_nested_*):
tests/cpp/test_nested.cpp, built against the emulator build of the product sources (CPU tier) and
against libirs_hip.so on the GPU — driven as tests/test_score_docs_cpp.py drives its C++ test."""
import subprocess
from pathlib import Path

import pytest

import oracle
from iresearch_amd import _build

ROOT = Path(__file__).resolve().parents[1]


def _cpp(L, tmp_path, extra=()):
    synth_lib = _build.build_synth()
    exe = tmp_path / "test_nested"
    lib = Path(L._name)
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall",
           "-I", str(ROOT / "include"), "-I", str(ROOT / "iresearch_amd" / "cpp"),
           "-I", str(ROOT / "iresearch_amd" / "index"), "-I", str(ROOT / "oracle"),
           str(ROOT / "tests" / "cpp" / "test_nested.cpp"), "-o", str(exe), str(lib), str(synth_lib),
           str(oracle.build()), "-pthread", "-Wl,-rpath," + str(lib.parent),
           "-Wl,-rpath," + str(Path(synth_lib).parent), "-Wl,-rpath," + str(ROOT / "oracle"), *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0 and "test_nested OK" in run.stdout, (run.stdout + run.stderr)[-3000:]


def test_cpp_nested_emulated(simlib, tmp_path):
    _cpp(simlib, tmp_path)


@pytest.mark.gpu
def test_cpp_nested_gpu(gpulib, tmp_path):
    rocm = "/opt/rocm/lib"
    _cpp(gpulib, tmp_path, ["-Wl,-rpath," + rocm, "-Wl,-rpath-link," + rocm, "-Wl,--allow-shlib-undefined"])
