// tests/probe/wave_probe.hip — TEST INFRASTRUCTURE ONLY: one kernel per family of wave::
// primitives, each doing nothing but calling the primitive on the caller's operands and
// storing what it returned.  tests/test_wave_primitives.py builds this file twice, like the
// product sources are built — against tests/sim (g++, the CPU fiber emulator's wave.h / gpu_rt.h)
// and against iresearch_amd/csrc/hip (hipcc, gfx950) — and holds both to one plain statement
// per primitive.  The product library never sees this file.
//
// Every kernel is straight-line or loops over a compile-time count; every buffer comes with
// its size and is indexed below it (an operand that would reach outside is skipped and
// reported through the `bad` word); no kernel waits on another.
#include "gpu_rt.h"
#include "types.h"
#include "wave.h"

#include <cstdint>
#include <cstring>

namespace probe {

using irs_hip::BlkDir;
using irs_hip::DevQTerm;
using irs_hip::DevQuery;
using irs_hip::DevTail;

// The records the block-driven and joined kernels read with sload<T> live in headers that
// carry those kernels (lead.h: ConjItem; join.h: StreamRec, JoinWg).  sload<T> depends on T
// through its size and alignment only: same-shaped stand-ins here, and the test module
// compares both numbers with the declarations in those headers.
struct alignas(32) ConjItemShape { uint32_t w[8]; };
struct alignas(16) StreamRecShape { uint64_t a[4]; uint32_t w[8]; };
struct alignas(16) JoinWgShape { uint64_t a[8]; uint32_t w[10]; uint32_t pad[2]; uint64_t b[2]; };
static_assert(sizeof(ConjItemShape) == 32 && sizeof(StreamRecShape) == 64 && sizeof(JoinWgShape) == 128, "");

enum : int { kOk = 0, kEinval = -1, kEdevice = -2, kEbounds = -3, kEldsBase = -4 };

constexpr uint32_t kNone = 0xFFFFFFFFu;   // an operand slot that asks for nothing

__device__ __forceinline__ uint32_t f2u(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
__device__ __forceinline__ float u2f(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// ---- cross-lane ------------------------------------------------------------------------
// One thread per input word, whole wavefronts only.  `diverge`: odd and even lanes first take
// different sides of a branch that loads (so that it stays a branch), reconverge, and the
// primitives follow directly — the statement is applied to the values behind the branch.
constexpr uint32_t kXlOut = 16;
__global__ void __launch_bounds__(1024)
k_crosslane(const uint32_t* a_in, const uint32_t* b_in, const uint32_t* salt, uint32_t n,
            uint32_t k, uint32_t x, uint32_t diverge, uint32_t* out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;   // (n is a multiple of 64: whole wavefronts leave)
  uint32_t a = a_in[t], b = b_in[t];
  if (diverge) {
    if (t & 1u) a ^= salt[t]; else b += salt[t];
  }
  const uint32_t wbase = t & ~63u;
  const uint32_t u = a_in[wbase] ^ b_in[wbase + 63u];   // identical in the wavefront's lanes
  const uint64_t u64 = (uint64_t(b_in[wbase]) << 32) | a_in[wbase + 63u];
  uint32_t* o = out + size_t(t) * kXlOut;
  o[0] = wave::inclusive_scan(a);
  uint32_t s0 = a, s1 = b;
  wave::inclusive_scan2(s0, s1);
  o[1] = s0;
  o[2] = s1;
  o[3] = wave::reduce_add(a);
  o[4] = wave::reduce_max(a);
  o[5] = wave::bcast(a, int(k));
  const uint64_t m = wave::ballot((b & 1u) != 0u);
  o[6] = uint32_t(m);
  o[7] = uint32_t(m >> 32);
  o[8] = wave::read_lane(a, k);
  o[9] = f2u(wave::read_lane_f(u2f(b), k));
  o[10] = wave::write_lane(a, x, k);
  o[11] = wave::uniform(u);
  const uint64_t v64 = wave::uniform64(u64);
  o[12] = uint32_t(v64);
  o[13] = uint32_t(v64 >> 32);
  o[14] = f2u(wave::uniform_f(u2f(u)));
  o[15] = wave::lane_id();
}

// ---- integer ---------------------------------------------------------------------------
constexpr uint32_t kIntIn = 8, kIntOut = 10;
__global__ void __launch_bounds__(256)
k_integer(const uint32_t* in, uint32_t n, uint32_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t x[kIntIn];
#pragma unroll
  for (uint32_t j = 0; j < kIntIn; ++j) x[j] = in[size_t(j) * n + i];
  uint32_t r[kIntOut];
  r[0] = wave::mul24(x[0], x[1]);
  r[1] = wave::mul_hi(x[2], x[3]);
  r[2] = wave::funnel(x[2], x[3], x[4]);
  r[3] = wave::bfe(x[2], x[5]);
  r[4] = wave::pk_min_u16(x[2], x[3]);
  r[5] = wave::pk_max_u16(x[2], x[3]);
  r[6] = wave::pk_add_u16(x[2], x[3]);
  uint32_t acc = x[6];
  wave::count_nonzero4(acc, x[2], x[3], x[0], x[1]);
  r[7] = acc;
  acc = x[6];
  wave::count_nonzero4(acc, (unsigned long long)((uint64_t(x[2]) << 32) | x[3]),
                       (unsigned long long)((uint64_t(x[0]) << 32) | x[1]),
                       (unsigned long long)(uint64_t(x[3]) << 32), (unsigned long long)(x[1]));
  r[8] = acc;
  acc = x[7];
  wave::count_nonzero_halves4(acc, x[2], x[3], x[0], x[1]);
  r[9] = acc;
#pragma unroll
  for (uint32_t j = 0; j < kIntOut; ++j) out[size_t(j) * n + i] = r[j];
}

// ---- float -----------------------------------------------------------------------------
constexpr uint32_t kFltIn = 5, kFltOut = 3;
__global__ void __launch_bounds__(256)
k_float(const float* in, uint32_t n, float* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = wave::fast_rcp(in[i]);
  out[size_t(n) + i] = wave::fast_sqrt(in[size_t(n) + i]);
  out[size_t(2) * n + i] = wave::fma(in[size_t(2) * n + i], in[size_t(3) * n + i], in[size_t(4) * n + i]);
}

// ---- LDS by absolute address -----------------------------------------------------------
// No static __shared__ here: the dynamic block is the kernel's only LDS.  The workgroup
// copies `img` into it through ordinary pointers, every thread performs ONE operation of
// kind OP on its own operands par[4 * t ..] (kNone in the first: none), and the block is
// copied out again, so that the caller sees what the operation returned AND every byte it
// left behind.  flags[0] = lds_is_at_zero (nothing is addressed absolutely unless it holds),
// flags[1] = operands that would have reached beyond `bytes` (skipped).
enum LdsOp : int { kLdsU8, kLdsF32, kLdsAdd32, kLdsAdd64, kLdsRead4, kLdsZero4, kLdsTake4, kLdsTake4x2, kLdsTake4x3, kLdsOps };
constexpr uint32_t kLdsMax = 160u * 1024u, kLdsThreads = 1024, kLdsRes = 12;
constexpr uint32_t kLdsWordsPerThread = kLdsMax / 4u / kLdsThreads;   // 40

__device__ __forceinline__ bool lds_fits(uint32_t off, uint32_t width, uint32_t bytes, uint32_t* flags) {
  if (off <= bytes && width <= bytes - off && off % (width < 16u ? width : 16u) == 0u) return true;
  atomicAdd(&flags[1], 1u);
  return false;
}

template<int OP>
__global__ void __launch_bounds__(kLdsThreads)
k_lds(const uint32_t* img, uint32_t bytes, const uint32_t* par, uint32_t* res, uint32_t* img_out,
      uint32_t* flags) {
  RT_DYN_SMEM(smem);
  const uint32_t t = threadIdx.x, words = bytes / 4u;
  uint32_t* sm32 = reinterpret_cast<uint32_t*>(smem);
  const bool at_zero = wave::lds_is_at_zero(smem);
  if (t == 0) flags[0] = at_zero ? 1u : 0u;
#pragma unroll 4
  for (uint32_t j = 0; j < kLdsWordsPerThread; ++j) {
    const uint32_t w = j * kLdsThreads + t;
    if (w < words) sm32[w] = img[w];
  }
  __syncthreads();
  uint32_t p[4];
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) p[j] = par[size_t(t) * 4u + j];
  uint32_t r[kLdsRes];
#pragma unroll
  for (uint32_t j = 0; j < kLdsRes; ++j) r[j] = 0;
  if (at_zero && p[0] != kNone) {
    uint32_t a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0}, c[4] = {0, 0, 0, 0};
    if (OP == kLdsU8) {
      if (lds_fits(p[0], 1, bytes, flags)) r[0] = wave::lds_u8(smem, p[0]);
    } else if (OP == kLdsF32) {
      if (lds_fits(p[0], 4, bytes, flags)) r[0] = f2u(wave::lds_f32(smem, p[0]));
    } else if (OP == kLdsAdd32) {
      if (lds_fits(p[0], 4, bytes, flags)) wave::lds_add(smem, p[0], p[1]);
    } else if (OP == kLdsAdd64) {
      if (lds_fits(p[0], 8, bytes, flags))
        wave::lds_add(smem, p[0], (unsigned long long)((uint64_t(p[2]) << 32) | p[1]));
    } else if (OP == kLdsRead4) {
      if (lds_fits(p[0], 16, bytes, flags)) wave::lds_read4(smem, p[0], a);
    } else if (OP == kLdsZero4) {
      if (lds_fits(p[0], 16, bytes, flags)) wave::lds_zero4(smem, p[0]);
    } else if (OP == kLdsTake4) {
      if (lds_fits(p[0], 16, bytes, flags)) wave::lds_take4(smem, p[0], a);
    } else if (OP == kLdsTake4x2) {
      if (lds_fits(p[0], 16, bytes, flags) && lds_fits(p[1], 16, bytes, flags))
        wave::lds_take4x2(smem, p[0], p[1], a, b);
    } else if (OP == kLdsTake4x3) {
      if (lds_fits(p[0], 16, bytes, flags) && lds_fits(p[1], 16, bytes, flags) &&
          lds_fits(p[2], 16, bytes, flags))
        wave::lds_take4x3(smem, p[0], p[1], p[2], a, b, c);
    }
    if (OP >= kLdsRead4) {
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        r[j] = a[j];
        r[4 + j] = b[j];
        r[8 + j] = c[j];
      }
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < kLdsRes; ++j) res[size_t(t) * kLdsRes + j] = r[j];
  __syncthreads();
#pragma unroll 4
  for (uint32_t j = 0; j < kLdsWordsPerThread; ++j) {
    const uint32_t w = j * kLdsThreads + t;
    if (w < words) img_out[w] = sm32[w];
  }
}

// ---- wave::sync ------------------------------------------------------------------------
// Eight rounds: lane l of every wavefront writes its wavefront's slot l, sync, reads slot
// 63 - l.  (A second sync closes the round: the next round's write must not overtake this
// round's read of the same slot — in hardware order holds by itself, the emulator's lanes
// are fibers.)
constexpr uint32_t kSyncRounds = 8;
__global__ void __launch_bounds__(1024)
k_sync(const uint32_t* in, uint32_t n, uint32_t* out) {
  RT_DYN_SMEM(smem);
  uint32_t* slot = reinterpret_cast<uint32_t*>(smem);
  const uint32_t t = threadIdx.x;
  if (t >= n) return;
  const uint32_t base = t & ~63u, lane = t & 63u;
#pragma unroll
  for (uint32_t r = 0; r < kSyncRounds; ++r) {
    slot[base + lane] = in[size_t(r) * n + t];
    wave::sync();
    out[size_t(r) * n + t] = slot[base + 63u - lane];
    wave::sync();
  }
}

// ---- loads that are not flat -----------------------------------------------------------
template<typename T>
__global__ void __launch_bounds__(64)
k_sload(uint64_t base, uint32_t index, T* out) {
  const T v = wave::sload<T>(base + uint64_t(index) * sizeof(T));
  if (threadIdx.x == 0) *out = v;
}

// per thread: one offset; gload_u32 | gload_u64 | gload_u32x4 -> words 0..6 (AT = false), or
// gload_u32x4_at of the same address -> words 7..10 (AT = true: a kernel of its own, so that the
// 64-bit per-lane address it needs is not shared with the base + offset forms)
constexpr uint32_t kGlOut = 11;
template<bool AT>
__global__ void __launch_bounds__(256)
k_gload(uint64_t base, uint32_t bytes, const uint32_t* offs, uint32_t n, uint32_t* out, uint32_t* bad) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t off = offs[t];
  uint32_t* o = out + size_t(t) * kGlOut;
  if (bytes < 16u || off > bytes - 16u || (off & 3u)) {   // (32-bit: the buffer is below 4 GiB)
    atomicAdd(bad, 1u);
    return;
  }
  uint32_t q[4];
  if (AT) {
    wave::gload_u32x4_at(base + off, q);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) o[7 + j] = q[j];
  } else {
    o[0] = wave::gload_u32(base, off);
    const uint64_t v = wave::gload_u64(base, off);
    o[1] = uint32_t(v);
    o[2] = uint32_t(v >> 32);
    wave::gload_u32x4(base, off, q);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) o[3 + j] = q[j];
  }
}

// load_u64 / load_u32 at byte offsets 0..15 of a 32-byte line, from global memory and from LDS
__global__ void __launch_bounds__(64)
k_unaligned(const uint8_t* line /*[32]*/, uint32_t* out /*[16][6]*/) {
  RT_DYN_SMEM(smem);
  const uint32_t t = threadIdx.x;
  if (t < 32u) smem[t] = line[t];
  __syncthreads();
  if (t >= 16u) return;
  const uint64_t g = wave::load_u64(line + t), l = wave::load_u64(smem + t);
  uint32_t* o = out + t * 6u;
  o[0] = uint32_t(g);
  o[1] = uint32_t(g >> 32);
  o[2] = wave::load_u32(line + t);
  o[3] = uint32_t(l);
  o[4] = uint32_t(l >> 32);
  o[5] = wave::load_u32(smem + t);
}

// ---- host side: the same code on both builds (rt:: only) -------------------------------
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

template<int OP>
int run_lds(uint32_t bytes, const Dev& img, const Dev& par, const Dev& res,
            const Dev& out, const Dev& flags) {
  if (!rt::allow_dynamic_smem(reinterpret_cast<const void*>(k_lds<OP>), bytes)) return kEdevice;
  RT_LAUNCH(k_lds<OP>, 1, kLdsThreads, bytes, nullptr, img.as<uint32_t>(), bytes, par.as<uint32_t>(),
            res.as<uint32_t>(), out.as<uint32_t>(), flags.as<uint32_t>());
  return finish();
}

template<typename T>
int run_sload(const void* recs, size_t n_recs, uint32_t index, void* out) {
  Dev d(n_recs * sizeof(T)), o(sizeof(T));
  if (!d.p || !o.p) return kEdevice;
  if (!up(d, recs, n_recs * sizeof(T)) || !rt::dmemset(o.p, 0xEE, sizeof(T), nullptr)) return kEdevice;
  RT_LAUNCH(k_sload<T>, 1, 64, 0, nullptr, uint64_t(reinterpret_cast<uintptr_t>(d.p)), index, o.as<T>());
  const int rc = finish();
  if (rc != kOk) return rc;
  return down(out, o, sizeof(T)) ? kOk : kEdevice;
}

}  // namespace probe

using namespace probe;

extern "C" {

int wp_arch(char* buf, size_t cap) {
  return buf && cap && rt::device_count() > 0 && rt::set_device(0) && rt::device_arch(0, buf, cap) ? kOk : kEdevice;
}

// n threads (a multiple of 64) in workgroups of `block`; out: [n][16]
int wp_crosslane(const uint32_t* a, const uint32_t* b, const uint32_t* salt, uint32_t n, uint32_t block,
                 uint32_t k, uint32_t x, uint32_t diverge, uint32_t* out) {
  if (!a || !b || !salt || !out || !n || n % 64u || !block || block % 64u || block > 1024u || n % block ||
      k > 63u)
    return kEinval;
  const size_t in_b = size_t(n) * 4u, out_b = size_t(n) * kXlOut * 4u;
  Dev da(in_b), db(in_b), ds(in_b), dout(out_b);
  if (!da.p || !db.p || !ds.p || !dout.p) return kEdevice;
  if (!up(da, a, in_b) || !up(db, b, in_b) || !up(ds, salt, in_b) || !rt::dmemset(dout.p, 0xEE, out_b, nullptr))
    return kEdevice;
  RT_LAUNCH(k_crosslane, n / block, block, 0, nullptr, da.as<uint32_t>(), db.as<uint32_t>(),
            ds.as<uint32_t>(), n, k, x, diverge, dout.as<uint32_t>());
  const int rc = finish();
  if (rc != kOk) return rc;
  return down(out, dout, out_b) ? kOk : kEdevice;
}

// in: [8][n], out: [10][n]
int wp_integer(const uint32_t* in, uint32_t n, uint32_t* out) {
  if (!in || !out || !n) return kEinval;
  const size_t in_b = size_t(n) * kIntIn * 4u, out_b = size_t(n) * kIntOut * 4u;
  Dev din(in_b), dout(out_b);
  if (!din.p || !dout.p) return kEdevice;
  if (!up(din, in, in_b) || !rt::dmemset(dout.p, 0xEE, out_b, nullptr)) return kEdevice;
  RT_LAUNCH(k_integer, (n + 255u) / 256u, 256, 0, nullptr, din.as<uint32_t>(), n, dout.as<uint32_t>());
  const int rc = finish();
  if (rc != kOk) return rc;
  return down(out, dout, out_b) ? kOk : kEdevice;
}

// in: [5][n] (rcp operand, sqrt operand, fma a, b, c), out: [3][n]
int wp_float(const float* in, uint32_t n, float* out) {
  if (!in || !out || !n) return kEinval;
  const size_t in_b = size_t(n) * kFltIn * 4u, out_b = size_t(n) * kFltOut * 4u;
  Dev din(in_b), dout(out_b);
  if (!din.p || !dout.p) return kEdevice;
  if (!up(din, in, in_b) || !rt::dmemset(dout.p, 0xEE, out_b, nullptr)) return kEdevice;
  RT_LAUNCH(k_float, (n + 255u) / 256u, 256, 0, nullptr, din.as<float>(), n, dout.as<float>());
  const int rc = finish();
  if (rc != kOk) return rc;
  return down(out, dout, out_b) ? kOk : kEdevice;
}

// One workgroup of 1024 threads (16 wavefronts) on a dynamic LDS block of `bytes` (a multiple
// of 16) holding img; par: [1024][4], res: [1024][12], img_out: [bytes], flags: [2]
int wp_lds(int op, uint32_t bytes, const uint32_t* img, const uint32_t* par,
           uint32_t* res, uint32_t* img_out, uint32_t* flags) {
  const uint32_t threads = kLdsThreads;
  if (op < 0 || op >= kLdsOps || !bytes || bytes % 16u || bytes > kLdsMax || !img || !par || !res || !img_out || !flags)
    return kEinval;
  const size_t par_b = size_t(threads) * 16u, res_b = size_t(threads) * kLdsRes * 4u;
  Dev dimg(bytes), dpar(par_b), dres(res_b), dout(bytes), dfl(8);
  if (!dimg.p || !dpar.p || !dres.p || !dout.p || !dfl.p) return kEdevice;
  if (!up(dimg, img, bytes) || !up(dpar, par, par_b) || !rt::dmemset(dres.p, 0xEE, res_b, nullptr) ||
      !rt::dmemset(dout.p, 0xEE, bytes, nullptr) || !rt::dmemset(dfl.p, 0, 8, nullptr))
    return kEdevice;
  int rc = kEinval;
  switch (op) {
    case kLdsU8: rc = run_lds<kLdsU8>(bytes, dimg, dpar, dres, dout, dfl); break;
    case kLdsF32: rc = run_lds<kLdsF32>(bytes, dimg, dpar, dres, dout, dfl); break;
    case kLdsAdd32: rc = run_lds<kLdsAdd32>(bytes, dimg, dpar, dres, dout, dfl); break;
    case kLdsAdd64: rc = run_lds<kLdsAdd64>(bytes, dimg, dpar, dres, dout, dfl); break;
    case kLdsRead4: rc = run_lds<kLdsRead4>(bytes, dimg, dpar, dres, dout, dfl); break;
    case kLdsZero4: rc = run_lds<kLdsZero4>(bytes, dimg, dpar, dres, dout, dfl); break;
    case kLdsTake4: rc = run_lds<kLdsTake4>(bytes, dimg, dpar, dres, dout, dfl); break;
    case kLdsTake4x2: rc = run_lds<kLdsTake4x2>(bytes, dimg, dpar, dres, dout, dfl); break;
    case kLdsTake4x3: rc = run_lds<kLdsTake4x3>(bytes, dimg, dpar, dres, dout, dfl); break;
  }
  if (rc != kOk) return rc;
  if (!down(res, dres, res_b) || !down(img_out, dout, bytes) || !down(flags, dfl, 8)) return kEdevice;
  if (!flags[0]) return kEldsBase;
  return flags[1] ? kEbounds : kOk;
}

// in, out: [8][threads]; one workgroup
int wp_sync(const uint32_t* in, uint32_t threads, uint32_t* out) {
  if (!in || !out || !threads || threads % 64u || threads > 1024u) return kEinval;
  const size_t b = size_t(threads) * kSyncRounds * 4u;
  Dev din(b), dout(b);
  if (!din.p || !dout.p) return kEdevice;
  if (!up(din, in, b) || !rt::dmemset(dout.p, 0xEE, b, nullptr)) return kEdevice;
  RT_LAUNCH(k_sync, 1, threads, size_t(threads) * 4u, nullptr, din.as<uint32_t>(), threads, dout.as<uint32_t>());
  const int rc = finish();
  if (rc != kOk) return rc;
  return down(out, dout, b) ? kOk : kEdevice;
}

// type: 0 BlkDir, 1 ConjItem, 2 DevQuery, 3 DevQTerm, 4 DevTail, 5 StreamRec, 6 JoinWg
int wp_sload_size(int type) {
  switch (type) {
    case 0: return int(sizeof(BlkDir));
    case 1: return int(sizeof(ConjItemShape));
    case 2: return int(sizeof(DevQuery));
    case 3: return int(sizeof(DevQTerm));
    case 4: return int(sizeof(DevTail));
    case 5: return int(sizeof(StreamRecShape));
    case 6: return int(sizeof(JoinWgShape));
  }
  return kEinval;
}
int wp_sload_align(int type) {
  switch (type) {
    case 0: return int(alignof(BlkDir));
    case 1: return int(alignof(ConjItemShape));
    case 2: return int(alignof(DevQuery));
    case 3: return int(alignof(DevQTerm));
    case 4: return int(alignof(DevTail));
    case 5: return int(alignof(StreamRecShape));
    case 6: return int(alignof(JoinWgShape));
  }
  return kEinval;
}
// recs: n_recs records of the type; out: one record = record `index`
int wp_sload(int type, const void* recs, uint64_t n_recs, uint32_t index, void* out) {
  if (!recs || !out || index >= n_recs) return kEinval;
  switch (type) {
    case 0: return run_sload<BlkDir>(recs, n_recs, index, out);
    case 1: return run_sload<ConjItemShape>(recs, n_recs, index, out);
    case 2: return run_sload<DevQuery>(recs, n_recs, index, out);
    case 3: return run_sload<DevQTerm>(recs, n_recs, index, out);
    case 4: return run_sload<DevTail>(recs, n_recs, index, out);
    case 5: return run_sload<StreamRecShape>(recs, n_recs, index, out);
    case 6: return run_sload<JoinWgShape>(recs, n_recs, index, out);
  }
  return kEinval;
}

// buf: `bytes` bytes; offs: n per-thread offsets (4-byte aligned, offs + 16 <= bytes); out: [n][11]
int wp_gload(const void* buf, uint64_t bytes, const uint32_t* offs, uint32_t n, uint32_t* out) {
  if (!buf || !offs || !out || !n || bytes < 16u || bytes >> 32) return kEinval;
  const size_t out_b = size_t(n) * kGlOut * 4u;
  Dev dbuf(bytes), doffs(size_t(n) * 4u), dout(out_b), dbad(4);
  if (!dbuf.p || !doffs.p || !dout.p || !dbad.p) return kEdevice;
  if (!up(dbuf, buf, bytes) || !up(doffs, offs, size_t(n) * 4u) || !rt::dmemset(dout.p, 0xEE, out_b, nullptr) ||
      !rt::dmemset(dbad.p, 0, 4, nullptr))
    return kEdevice;
  RT_LAUNCH(k_gload<false>, (n + 255u) / 256u, 256, 0, nullptr, uint64_t(reinterpret_cast<uintptr_t>(dbuf.p)),
            uint32_t(bytes), doffs.as<uint32_t>(), n, dout.as<uint32_t>(), dbad.as<uint32_t>());
  RT_LAUNCH(k_gload<true>, (n + 255u) / 256u, 256, 0, nullptr, uint64_t(reinterpret_cast<uintptr_t>(dbuf.p)),
            uint32_t(bytes), doffs.as<uint32_t>(), n, dout.as<uint32_t>(), dbad.as<uint32_t>());
  int rc = finish();
  if (rc != kOk) return rc;
  uint32_t bad = 0;
  if (!down(out, dout, out_b) || !down(&bad, dbad, 4)) return kEdevice;
  return bad ? kEbounds : kOk;
}

// Lane offsets with bit 31 set, on a buffer of 2 GiB + 64 KiB (one allocation, freed before
// returning).  The allocation has 2 GiB more in FRONT of the buffer, so that an offset taken
// as a signed number would still read mapped memory — there, where the `decoy` words were
// put — and shows up as a wrong value.  patches: [n][4] words stored at buffer + offs[i];
// decoys: [n][4] words stored 4 GiB below that (only where offs[i] has bit 31 set).
int wp_gload_far(const uint32_t* offs, uint32_t n, const uint32_t* patches, const uint32_t* decoys,
                 uint32_t* out) {
  if (!offs || !patches || !decoys || !out || !n || n > 256u) return kEinval;
  const uint64_t half = (uint64_t(1) << 31) + (uint64_t(64) << 10), front = uint64_t(1) << 31, wrap = uint64_t(1) << 32;
  for (uint32_t i = 0; i < n; ++i)
    if (uint64_t(offs[i]) + 16u > half || (offs[i] & 3u)) return kEinval;
  const size_t out_b = size_t(n) * kGlOut * 4u;
  Dev all(front + half), doffs(size_t(n) * 4u), dout(out_b), dbad(4);
  if (!all.p || !doffs.p || !dout.p || !dbad.p) return kEdevice;
  uint8_t* buf = all.as<uint8_t>() + front;
  for (uint32_t i = 0; i < n; ++i) {
    if ((offs[i] >> 31) && !rt::h2d(buf + offs[i] - wrap, decoys + 4u * i, 16, nullptr)) return kEdevice;
    if (!rt::h2d(buf + offs[i], patches + 4u * i, 16, nullptr)) return kEdevice;
  }
  if (!up(doffs, offs, size_t(n) * 4u) || !rt::dmemset(dout.p, 0xEE, out_b, nullptr) ||
      !rt::dmemset(dbad.p, 0, 4, nullptr) || !rt::sync(nullptr))
    return kEdevice;
  RT_LAUNCH(k_gload<false>, (n + 255u) / 256u, 256, 0, nullptr, uint64_t(reinterpret_cast<uintptr_t>(buf)), uint32_t(half),
            doffs.as<uint32_t>(), n, dout.as<uint32_t>(), dbad.as<uint32_t>());
  RT_LAUNCH(k_gload<true>, (n + 255u) / 256u, 256, 0, nullptr, uint64_t(reinterpret_cast<uintptr_t>(buf)), uint32_t(half),
            doffs.as<uint32_t>(), n, dout.as<uint32_t>(), dbad.as<uint32_t>());
  int rc = finish();
  if (rc != kOk) return rc;
  uint32_t bad = 0;
  if (!down(out, dout, out_b) || !down(&bad, dbad, 4)) return kEdevice;
  return bad ? kEbounds : kOk;
}

// line: 32 bytes; out: [16][6] = load_u64 lo, hi, load_u32 from global | the same from LDS
int wp_unaligned(const uint8_t* line, uint32_t* out) {
  if (!line || !out) return kEinval;
  Dev dl(32), dout(16 * 6 * 4);
  if (!dl.p || !dout.p) return kEdevice;
  if (!up(dl, line, 32) || !rt::dmemset(dout.p, 0xEE, 16 * 6 * 4, nullptr)) return kEdevice;
  RT_LAUNCH(k_unaligned, 1, 64, 64, nullptr, dl.as<uint8_t>(), dout.as<uint32_t>());
  const int rc = finish();
  if (rc != kOk) return rc;
  return down(out, dout, 16 * 6 * 4) ? kOk : kEdevice;
}

}  // extern "C"
