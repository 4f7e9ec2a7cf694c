"""Generates tests/golden/codec_live_golden.npz with the REFERENCE's own compiled codec
(oracle/_ref, see make_golden.py): the random vectors of test_oracle.py's
test_codec_against_live_reference (default_rng(5), four per bit width, drawn in the test's
order) and the words the reference packs them into, so that the test checks them where
oracle/_ref cannot be built.  Run in the build container only:
python tests/golden/make_live_codec_golden.py

Contents (all little-endian uint32):
  values_b{bits}                 [4][128] random values < 2^bits
  scalar_b{bits}, simd4_b{bits}  [4][4 * bits] the reference's packed words of them
The text of no reference source file is stored — only inputs and outputs.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import oracle  # noqa: E402


def main():
    R = oracle.ref()
    assert R is not None, "oracle/_ref is not built (needs /root/reference)"
    rng = np.random.default_rng(5)
    out = {}
    for bits in range(1, 33):
        vals = np.stack([rng.integers(0, 1 << bits, 128, dtype=np.uint64).astype(np.uint32)
                         for _ in range(4)])
        out["values_b%d" % bits] = vals
        for lay, fn in (("scalar", R.ref_pack_scalar), ("simd4", R.ref_pack_simd4)):
            packed = np.zeros((len(vals), 4 * bits), np.uint32)
            for v, p in zip(vals, packed):
                fn(np.ascontiguousarray(v).ctypes.data, bits, p.ctypes.data)
            out["%s_b%d" % (lay, bits)] = packed
    np.savez_compressed(Path(__file__).with_name("codec_live_golden.npz"), **out)
    print("wrote", len(out), "arrays")


if __name__ == "__main__":
    main()
