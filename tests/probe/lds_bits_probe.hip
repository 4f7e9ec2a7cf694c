// tests/probe/lds_bits_probe.hip — TEST INFRASTRUCTURE ONLY: irs_hip::lds_bits32 (csrc/lds_bits.h: the
// 32 bits at an LDS offset as an integer, wave::lds_f32 and a bit cast) on the caller's operands,
// alone and the way clauses.h uses it — the low word of a 64-bit
// accumulator read while other threads add multiples of 2^16 to the same accumulator.
// tests/test_wave_lds_bits.py builds this file twice, as tests/test_wave_primitives.py builds
// wave_probe.hip — against tests/sim (the emulator's wave.h) and against iresearch_amd/csrc/hip
// (hipcc, gfx950) — and holds both to one plain statement.  The product library never sees it.
//
// Every buffer comes with its size and is indexed below it: an offset that is not a multiple of 4
// inside the image is skipped and counted in flags[1]; no kernel waits on another.
#include "gpu_rt.h"
#include "lds_bits.h"
#include "wave.h"

#include <cstdint>

namespace probe {

enum : int { kOk = 0, kEinval = -1, kEdevice = -2 };
constexpr uint32_t kThreads = 1024;
constexpr uint32_t kMaxBytes = 64u * 1024u;

// res[i] = the 4 bytes at offs[i] of an LDS image of `bytes` bytes
__global__ void __launch_bounds__(kThreads)
k_read(const uint32_t* img, uint32_t bytes, const uint32_t* offs, uint32_t n, uint32_t* res, uint32_t* flags) {
  RT_DYN_SMEM(smem);
  uint32_t* sm32 = reinterpret_cast<uint32_t*>(smem);
  if (threadIdx.x == 0) flags[0] = wave::lds_is_at_zero(smem) ? 1u : 0u;
  for (uint32_t i = threadIdx.x; i < bytes / 4u; i += blockDim.x) sm32[i] = img[i];
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
    const uint32_t off = offs[i];
    if (off % 4u || off >= bytes) {
      atomicAdd(&flags[1], 1u);
      continue;
    }
    res[i] = irs_hip::lds_bits32(smem, off);
  }
}

// `words` 64-bit accumulators, zero.  Pass 1: thread t adds lo[t] (32 bits) to the low word of
// accumulator a1[t].  Barrier.  Pass 2: thread t reads the low word of accumulator a2[t] into res[t]
// and adds hi[t] << 16 (64 bits: the low 16 bits of the add are zero) to the same accumulator.
// Barrier; the accumulators come back in acc_out.
__global__ void __launch_bounds__(kThreads)
k_mask(uint32_t words, const uint32_t* a1, const uint32_t* lo, const uint32_t* a2, const uint32_t* hi,
       uint32_t* res, unsigned long long* acc_out, uint32_t* flags) {
  RT_DYN_SMEM(smem);
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(smem);
  const uint32_t t = threadIdx.x;
  if (t == 0) flags[0] = wave::lds_is_at_zero(smem) ? 1u : 0u;
  for (uint32_t i = t; i < words; i += blockDim.x) acc[i] = 0ull;
  __syncthreads();
  if (a1[t] < words) wave::lds_add(smem, 8u * a1[t], lo[t]);
  else atomicAdd(&flags[1], 1u);
  __syncthreads();
  if (a2[t] < words) {
    res[t] = irs_hip::lds_bits32(smem, 8u * a2[t]);
    wave::lds_add(smem, 8u * a2[t], static_cast<unsigned long long>(hi[t]) << 16);
  } else {
    atomicAdd(&flags[1], 1u);
  }
  __syncthreads();
  for (uint32_t i = t; i < words; i += blockDim.x) acc_out[i] = acc[i];
}

struct Dev {   // a device buffer that frees itself
  void* p = nullptr;
  explicit Dev(size_t n) : p(rt::dmalloc(n ? n : 4)) {}
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

int lp_read(uint32_t bytes, const uint32_t* img, const uint32_t* offs, uint32_t n, uint32_t* res, uint32_t* flags) {
  if (!bytes || bytes % 4u || bytes > kMaxBytes || !img || !offs || !n || !res || !flags) return kEinval;
  if (!rt::set_device(0)) return kEdevice;
  Dev dimg(bytes), doffs(size_t(n) * 4u), dres(size_t(n) * 4u), dflags(8);
  if (!dimg.p || !doffs.p || !dres.p || !dflags.p) return kEdevice;
  if (!up(dimg, img, bytes) || !up(doffs, offs, size_t(n) * 4u) || !rt::dmemset(dres.p, 0xEE, size_t(n) * 4u, nullptr) ||
      !rt::dmemset(dflags.p, 0, 8, nullptr))
    return kEdevice;
  if (!rt::allow_dynamic_smem(reinterpret_cast<const void*>(k_read), bytes)) return kEdevice;
  RT_LAUNCH(k_read, 1, kThreads, bytes, nullptr, dimg.as<uint32_t>(), bytes, doffs.as<uint32_t>(), n,
            dres.as<uint32_t>(), dflags.as<uint32_t>());
  const int rc = finish();
  if (rc != kOk) return rc;
  return down(res, dres, size_t(n) * 4u) && down(flags, dflags, 8) ? kOk : kEdevice;
}

int lp_mask(uint32_t words, const uint32_t* a1, const uint32_t* lo, const uint32_t* a2, const uint32_t* hi,
            uint32_t* res, uint64_t* acc_out, uint32_t* flags) {
  if (!words || words * 8u > kMaxBytes || !a1 || !lo || !a2 || !hi || !res || !acc_out || !flags) return kEinval;
  if (!rt::set_device(0)) return kEdevice;
  const size_t tb = size_t(kThreads) * 4u;
  Dev d1(tb), dlo(tb), d2(tb), dhi(tb), dres(tb), dacc(size_t(words) * 8u), dflags(8);
  if (!d1.p || !dlo.p || !d2.p || !dhi.p || !dres.p || !dacc.p || !dflags.p) return kEdevice;
  if (!up(d1, a1, tb) || !up(dlo, lo, tb) || !up(d2, a2, tb) || !up(dhi, hi, tb) ||
      !rt::dmemset(dres.p, 0xEE, tb, nullptr) || !rt::dmemset(dflags.p, 0, 8, nullptr))
    return kEdevice;
  if (!rt::allow_dynamic_smem(reinterpret_cast<const void*>(k_mask), size_t(words) * 8u)) return kEdevice;
  RT_LAUNCH(k_mask, 1, kThreads, size_t(words) * 8u, nullptr, words, d1.as<uint32_t>(), dlo.as<uint32_t>(),
            d2.as<uint32_t>(), dhi.as<uint32_t>(), dres.as<uint32_t>(), dacc.as<unsigned long long>(),
            dflags.as<uint32_t>());
  const int rc = finish();
  if (rc != kOk) return rc;
  return down(res, dres, tb) && down(acc_out, dacc, size_t(words) * 8u) && down(flags, dflags, 8) ? kOk : kEdevice;
}

}  // extern "C"
