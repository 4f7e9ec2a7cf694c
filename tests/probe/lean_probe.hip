// tests/probe/lean_probe.hip — TEST INFRASTRUCTURE ONLY, in the manner of wave_probe.hip: the two
// wave:: primitives of iresearch_amd/csrc/hip/wave_join.h (k_join_score<2>'s requests and
// epilogue), each called on the caller's operands and nothing else.  That header carries its own
// plain C++ forms; tests/test_join_score_lean.py builds this file the way the CPU emulator is built
// (g++, tests/sim: the plain forms) and for gfx950 (hipcc: the device forms) and holds both to one
// plain statement per primitive.  The product library never sees this file.
//
// Both kernels are straight-line; every buffer comes with its size and is indexed below it (an
// offset that would reach outside is skipped and reported through the `bad` word).
#include "gpu_rt.h"
#include "types.h"
#include "wave.h"
#include "wave_join.h"

#include <cstdint>

namespace probe {

enum : int { kOk = 0, kEinval = -1, kEdevice = -2, kEbounds = -3 };

// in: [5][n] = acc, a, b, c, d; out: [n] = acc after count_nonzero_halves4_nc(acc, a, b, c, d)
__global__ void __launch_bounds__(256)
k_halves_nc(const uint32_t* in, uint32_t n, uint32_t* out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  uint32_t acc = in[t];
  wave::count_nonzero_halves4_nc(acc, in[size_t(n) + t], in[size_t(2) * n + t], in[size_t(3) * n + t],
                                 in[size_t(4) * n + t]);
  out[t] = acc;
}

// per thread one offset: out[t] = gload_u32_imm<0 | 256 | 512 | 768 | 4092>(base, offs[t])
constexpr uint32_t kImmOut = 5, kImmMax = 4092;
__global__ void __launch_bounds__(256)
k_gload_imm(uint64_t base, uint32_t bytes, const uint32_t* offs, uint32_t n, uint32_t* out, uint32_t* bad) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t off = offs[t];
  if ((off & 3u) || bytes < kImmMax + 4u || off > bytes - kImmMax - 4u) {
    atomicAdd(bad, 1u);
    return;
  }
  uint32_t* o = out + size_t(t) * kImmOut;
  o[0] = wave::gload_u32_imm<0u>(base, off);
  o[1] = wave::gload_u32_imm<256u>(base, off);
  o[2] = wave::gload_u32_imm<512u>(base, off);
  o[3] = wave::gload_u32_imm<768u>(base, off);
  o[4] = wave::gload_u32_imm<kImmMax>(base, off);
}

struct Dev {   // a device buffer that frees itself
  void* p = nullptr;
  explicit Dev(size_t n) : p(rt::dmalloc(n)) {}
  ~Dev() { rt::dfree(p); }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  template<typename T> T* as() const { return static_cast<T*>(p); }
};
inline bool up(const Dev& d, const void* h, size_t n) { return rt::h2d(d.p, h, n, nullptr) && rt::sync(nullptr); }
inline bool down(void* h, const Dev& d, size_t n) { return rt::d2h(h, d.p, n, nullptr) && rt::sync(nullptr); }
inline int finish() { return rt::sync(nullptr) && rt::last_error_ok() ? kOk : kEdevice; }

}  // namespace probe

using namespace probe;

extern "C" {

int lp_arch(char* buf, size_t cap) {
  return buf && cap && rt::device_count() > 0 && rt::set_device(0) && rt::device_arch(0, buf, cap) ? kOk : kEdevice;
}

// in: [5][n], out: [n]
int lp_halves_nc(const uint32_t* in, uint32_t n, uint32_t* out) {
  if (!in || !out || !n) return kEinval;
  const size_t in_b = size_t(n) * 5u * 4u, out_b = size_t(n) * 4u;
  Dev din(in_b), dout(out_b);
  if (!din.p || !dout.p) return kEdevice;
  if (!up(din, in, in_b) || !rt::dmemset(dout.p, 0xEE, out_b, nullptr)) return kEdevice;
  RT_LAUNCH(k_halves_nc, (n + 255u) / 256u, 256, 0, nullptr, din.as<uint32_t>(), n, dout.as<uint32_t>());
  const int rc = finish();
  if (rc != kOk) return rc;
  return down(out, dout, out_b) ? kOk : kEdevice;
}

// buf: `bytes` bytes; offs: [n] byte offsets, multiples of 4, at most bytes - 4096; out: [n][5]
int lp_gload_imm(const void* buf, uint64_t bytes, const uint32_t* offs, uint32_t n, uint32_t* out) {
  if (!buf || !offs || !out || !n || bytes < 4096u || bytes >> 32) return kEinval;
  const size_t out_b = size_t(n) * kImmOut * 4u;
  Dev dbuf(bytes), doffs(size_t(n) * 4u), dout(out_b), dbad(4);
  if (!dbuf.p || !doffs.p || !dout.p || !dbad.p) return kEdevice;
  if (!up(dbuf, buf, bytes) || !up(doffs, offs, size_t(n) * 4u) || !rt::dmemset(dout.p, 0xEE, out_b, nullptr) ||
      !rt::dmemset(dbad.p, 0, 4, nullptr))
    return kEdevice;
  RT_LAUNCH(k_gload_imm, (n + 255u) / 256u, 256, 0, nullptr, uint64_t(reinterpret_cast<uintptr_t>(dbuf.p)),
            uint32_t(bytes), doffs.as<uint32_t>(), n, dout.as<uint32_t>(), dbad.as<uint32_t>());
  const int rc = finish();
  if (rc != kOk) return rc;
  uint32_t bad = 0;
  if (!down(out, dout, out_b) || !down(&bad, dbad, 4)) return kEdevice;
  return bad ? kEbounds : kOk;
}

}  // extern "C"
