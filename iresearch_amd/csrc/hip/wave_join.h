// wave_join.h — two more wavefront primitives, for k_join_score<2>'s requests and epilogue
// (join.h join_load4, join_pairs).  Unlike wave.h this header has no twin: each primitive carries
// its own — the gfx950 form under __HIP_DEVICE_COMPILE__, a plain C++ statement of the same
// meaning otherwise, written with what both wave.h and its twin of the CPU emulator offer — so the
// emulator build includes this very file.
// Include wave.h FIRST (as every kernel header does): a quoted include from here would find the
// wave.h next to this file, never the emulator's.
#pragma once
#include <cstdint>

namespace wave {

// acc (two 16-bit counters) += the non-zero low halves / high halves among a..d, as
// count_nonzero_halves4, while NO HALF OF acc CAN OVERFLOW (both counters stay below 2^16 — the
// caller's to guarantee): every minimum has halves <= 1, so plain 32-bit adds never carry from the
// low counter into the high one and two v_add3_u32 stand for the four packed adds.  Outside that
// domain the low counter's carry lands in the high one, where count_nonzero_halves4 wraps each
// half by itself.  (Four temporaries: every packed result is read two instructions after it is
// written at the earliest — no s_nop.)
__device__ __forceinline__ void count_nonzero_halves4_nc(uint32_t& acc, uint32_t a, uint32_t b,
                                                         uint32_t c, uint32_t d) {
  const uint32_t one = 0x00010001u;
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t t0, t1, t2, t3;
  asm("v_pk_min_u16 %1, %5, %9\n\tv_pk_min_u16 %2, %6, %9\n\tv_pk_min_u16 %3, %7, %9\n\t"
      "v_pk_min_u16 %4, %8, %9\n\tv_add3_u32 %1, %1, %2, %3\n\tv_add3_u32 %0, %0, %1, %4"
      : "+v"(acc), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
      : "v"(a), "v"(b), "v"(c), "v"(d), "s"(one));
#else
  acc += pk_min_u16(a, one) + pk_min_u16(b, one) + pk_min_u16(c, one) + pk_min_u16(d, one);
#endif
}

// 4 bytes at (wave-uniform 64-bit base) + (per-lane 32-bit offset) + IMM, IMM < 4096 a compile-time
// constant: gload_u32's instruction with IMM in its immediate offset field — several loads off one
// (base, offset) pair cost no address arithmetic at all.  The sum is formed in 64 bits on the GPU;
// callers keep off + IMM below 2^32, where the two forms agree.
template<uint32_t IMM>
__device__ __forceinline__ uint32_t gload_u32_imm(uint64_t base, uint32_t off) {
  static_assert(IMM < 4096u && IMM % 4u == 0u, "gload_u32_imm: the instruction's offset field");
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const IRS_GLOBAL uint32_t*)((const IRS_GLOBAL uint8_t*)base + off + IMM);
#else
  return gload_u32(base, off + IMM);
#endif
}

}  // namespace wave
