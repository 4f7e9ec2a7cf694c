// lds_bits.h — the 32 bits at a 4-byte aligned LDS offset as an integer, through a primitive that
// hip/wave.h and its emulator twin both have: wave::lds_f32 (ds_read_b32) and a bit cast — a load
// followed by a bit cast is no floating-point operation, every pattern (NaNs with any payload
// included) comes back as it lies there; tests/test_wave_lds_bits.py pins that on both builds.
// What clauses.h reads a doc's presence mask with: the low half of a 64-bit sum whose other bits
// other wavefronts are adding to between the same two barriers — the aligned 4-byte read is one
// LDS access, the bits nobody changes come back as they are.
#pragma once
#include "wave.h"

namespace irs_hip {

__device__ __forceinline__ uint32_t lds_bits32(const unsigned char* lds, uint32_t off) {
  return __float_as_uint(wave::lds_f32(lds, off));
}

}  // namespace irs_hip
