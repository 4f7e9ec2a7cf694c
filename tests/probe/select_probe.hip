// tests/probe/select_probe.hip — TEST INFRASTRUCTURE ONLY, in the manner of lean_probe.hip: the
// kernels every execution path ends in ("the selection layer"), each launched UNMODIFIED on the
// caller's operands — k_select (kernels.h), k_union_topk (phrase.h), k_conj_threshold and
// k_conj_hits (conj.h), k_group_threshold, k_group_sums and k_group_verdict (join.h) — and the
// three device functions of the integer pre-filter (score.h from_fixed, score_bin, bin_threshold)
// through the only kernel this file defines.  tests/test_select_layer.py builds this file the way
// the CPU emulator is built (g++, tests/sim) and for gfx950 (hipcc) and holds both to one plain
// statement per kernel.  The product library never sees this file.
//
// Every buffer comes with its size; an index a kernel would follow outside one (a unit, a member,
// an item range, a k beyond k_max, caps the dynamic LDS cannot hold) is refused here with kEinval
// before anything is launched.  Outputs are pre-filled with 0xEE bytes.
#include "gpu_rt.h"
#include "types.h"
#include "kernels.h"
#include "score.h"
#include "phrase.h"
#include "conj.h"
#include "join.h"

#include <cstdint>
#include <vector>

namespace probe {

using namespace irs_hip;

enum : int { kOk = 0, kEinval = -1, kEdevice = -2 };
constexpr size_t kLdsMax = 160u * 1024u;
constexpr uint32_t kNone = 0xFFFFFFFFu;

// out: val = from_fixed<ACC>(acc), bin = score_bin(val, bin_scale), thr = bin_threshold<ACC>(bs)
template<typename ACC>
__global__ void __launch_bounds__(256)
k_bins(const unsigned long long* acc, const uint32_t* bs, const float* bin_scale, const float* fx_inv,
       uint32_t n, float* val, uint32_t* bin, unsigned long long* thr) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  DevQuery qd{};
  qd.bin_scale = bin_scale[t];
  qd.fx_inv = fx_inv[t];
  const float v = from_fixed<ACC>(static_cast<ACC>(acc[t]), qd.fx_inv);
  val[t] = v;
  bin[t] = score_bin(v, qd.bin_scale);
  thr[t] = bin_threshold<ACC>(bs[t], qd);
}

struct Dev {   // a device buffer that frees itself
  void* p = nullptr;
  size_t n = 0;
  explicit Dev(size_t bytes) : p(rt::dmalloc(bytes)), n(bytes) {}
  ~Dev() { rt::dfree(p); }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  template<typename T> T* as() const { return static_cast<T*>(p); }
  // the caller's bytes (null: the buffer stays what a kernel's null argument is)
  bool up(const void* h) const { return p && rt::h2d(p, h, n, nullptr) && rt::sync(nullptr); }
  bool fill() const { return p && rt::dmemset(p, 0xEE, n, nullptr) && rt::sync(nullptr); }
  bool down(void* h) const { return p && rt::d2h(h, p, n, nullptr) && rt::sync(nullptr); }
};
inline int finish() { return rt::sync(nullptr) && rt::last_error_ok() ? kOk : kEdevice; }

// an optional per-unit array: uploaded if the caller gave one, else the kernel gets null
template<typename T>
struct Opt {
  Dev d;
  const bool on;
  Opt(const T* h, size_t count) : d(h ? count * sizeof(T) : 1), on(h != nullptr) { ok = !on || d.up(h); }
  const T* ptr() const { return on ? d.as<T>() : nullptr; }
  bool ok;
};

// DevQuery records of which only k is set
inline std::vector<DevQuery> queries_of(const uint32_t* k, uint32_t nq) {
  std::vector<DevQuery> v(nq, DevQuery{});
  for (uint32_t q = 0; q < nq; ++q) v[q].k = k[q];
  return v;
}

}  // namespace probe

using namespace probe;

extern "C" {

int sp_arch(char* buf, size_t cap) {
  return buf && cap && rt::device_count() > 0 && rt::set_device(0) && rt::device_arch(0, buf, cap) ? kOk : kEdevice;
}

// cands: [nq][cand_cap]; cand_count, hits, k, bstar, pruned: [nq]; min_bin, min_score, group_of: [nq]
// or null; out: [nq][k_max]; out_count: [nq]; status: one word, in (the bits so far) and out
int sp_select(const uint64_t* cands, uint32_t nq, uint32_t cand_cap, const uint32_t* cand_count,
              const unsigned long long* hits, const uint32_t* k, uint32_t k_max, uint32_t stage_cap,
              uint32_t sort_cap, const uint32_t* bstar, const uint32_t* min_bin, const uint32_t* pruned,
              const float* min_score, const uint32_t* group_of, Hit* out, uint32_t* out_count,
              uint32_t* status) {
  if (!cands || !cand_count || !hits || !k || !bstar || !pruned || !out || !out_count || !status) return kEinval;
  if (!nq || !cand_cap || !k_max || !stage_cap || sort_cap < 2u || (sort_cap & (sort_cap - 1u))) return kEinval;
  if (k_max > sort_cap || k_max > kMaxK || stage_cap > cand_cap) return kEinval;
  for (uint32_t q = 0; q < nq; ++q)
    if (k[q] > k_max) return kEinval;
  const size_t smem = (size_t(sort_cap) + stage_cap) * sizeof(uint64_t);
  if (smem > kLdsMax) return kEinval;
  const std::vector<DevQuery> qs = queries_of(k, nq);
  const size_t out_b = size_t(nq) * k_max * sizeof(Hit);
  Dev dq(size_t(nq) * sizeof(DevQuery)), dc(size_t(nq) * cand_cap * 8u), dn(size_t(nq) * 4u), dh(size_t(nq) * 8u),
      db(size_t(nq) * 4u), dp(size_t(nq) * 4u), dout(out_b), doc(size_t(nq) * 4u), dst(4);
  Opt<uint32_t> dmb(min_bin, nq), dgo(group_of, nq);
  Opt<float> dms(min_score, nq);
  if (!dq.up(qs.data()) || !dc.up(cands) || !dn.up(cand_count) || !dh.up(hits) || !db.up(bstar) ||
      !dp.up(pruned) || !dmb.ok || !dgo.ok || !dms.ok || !dout.fill() || !doc.fill() || !dst.up(status))
    return kEdevice;
  if (!rt::allow_dynamic_smem(reinterpret_cast<const void*>(k_select), smem)) return kEdevice;
  RT_LAUNCH(k_select, nq, kThreads, smem, nullptr, dq.as<DevQuery>(), dc.as<uint64_t>(), cand_cap,
            dn.as<uint32_t>(), dh.as<unsigned long long>(), dout.as<Hit>(), k_max, doc.as<uint32_t>(),
            dst.as<uint32_t>(), stage_cap, sort_cap, db.as<uint32_t>(), dmb.ptr(), dp.as<uint32_t>(),
            dms.ptr(), dgo.ptr());
  const int rc = finish();
  if (rc != kOk) return rc;
  return dout.down(out) && doc.down(out_count) && dst.down(status) ? kOk : kEdevice;
}

// a, b, out: [nq][k_max]; ca, cb, ta, tb, k, out_count, out_total: [nq]
int sp_union(const uint32_t* k, uint32_t nq, uint32_t k_max, const Hit* a, const uint32_t* ca,
             const unsigned long long* ta, const Hit* b, const uint32_t* cb, const unsigned long long* tb,
             Hit* out, uint32_t* out_count, unsigned long long* out_total) {
  if (!k || !a || !ca || !ta || !b || !cb || !tb || !out || !out_count || !out_total || !nq || !k_max) return kEinval;
  const std::vector<DevQuery> qs = queries_of(k, nq);
  const size_t list_b = size_t(nq) * k_max * sizeof(Hit);
  Dev dq(size_t(nq) * sizeof(DevQuery)), da(list_b), dca(size_t(nq) * 4u), dta(size_t(nq) * 8u), dbb(list_b),
      dcb(size_t(nq) * 4u), dtb(size_t(nq) * 8u), dout(list_b), doc(size_t(nq) * 4u), dot(size_t(nq) * 8u);
  if (!dq.up(qs.data()) || !da.up(a) || !dca.up(ca) || !dta.up(ta) || !dbb.up(b) || !dcb.up(cb) || !dtb.up(tb) ||
      !dout.fill() || !doc.fill() || !dot.fill())
    return kEdevice;
  RT_LAUNCH(k_union_topk, nq, kThreads, 0, nullptr, dq.as<DevQuery>(), k_max, da.as<Hit>(), dca.as<uint32_t>(),
            dta.as<unsigned long long>(), dbb.as<Hit>(), dcb.as<uint32_t>(), dtb.as<unsigned long long>(),
            dout.as<Hit>(), doc.as<uint32_t>(), dot.as<unsigned long long>());
  const int rc = finish();
  if (rc != kOk) return rc;
  return dout.down(out) && doc.down(out_count) && dot.down(out_total) ? kOk : kEdevice;
}

// k, bstar, min_bin (or null): [nq]; hist: [nq][kBins]; conj_units, n_items: [nc]
int sp_conj_threshold(const uint32_t* k, uint32_t nq, const uint32_t* conj_units, const uint32_t* n_items,
                      uint32_t nc, const uint32_t* hist, uint32_t stride, uint32_t margin,
                      const uint32_t* min_bin, uint32_t* bstar) {
  if (!k || !conj_units || !n_items || !hist || !bstar || !nq || !nc || !stride) return kEinval;
  for (uint32_t c = 0; c < nc; ++c)
    if (conj_units[c] >= nq) return kEinval;
  const std::vector<DevQuery> qs = queries_of(k, nq);
  Dev dq(size_t(nq) * sizeof(DevQuery)), du(size_t(nc) * 4u), dn(size_t(nc) * 4u), dh(size_t(nq) * kBins * 4u),
      db(size_t(nq) * 4u);
  Opt<uint32_t> dmb(min_bin, nq);
  if (!dq.up(qs.data()) || !du.up(conj_units) || !dn.up(n_items) || !dh.up(hist) || !dmb.ok || !db.fill())
    return kEdevice;
  RT_LAUNCH(k_conj_threshold, nc, 64, 0, nullptr, dq.as<DevQuery>(), du.as<uint32_t>(), dn.as<uint32_t>(),
            dh.as<uint32_t>(), stride, margin, db.as<uint32_t>(), dmb.ptr());
  const int rc = finish();
  if (rc != kOk) return rc;
  return db.down(bstar) ? kOk : kEdevice;
}

// k, bstar, min_bin (or null): [nq]; members: [ng][n_segs], a unit or 0xFFFFFFFF; group_hist:
// [ng][kBins + 2] = bins, sampled tiles, tiles
int sp_group_threshold(const uint32_t* k, uint32_t nq, const uint32_t* members, uint32_t n_segs, uint32_t ng,
                       const uint32_t* group_hist, uint32_t margin, const uint32_t* min_bin, uint32_t* bstar) {
  if (!k || !members || !group_hist || !bstar || !nq || !ng || !n_segs || n_segs > 64u) return kEinval;
  for (size_t i = 0; i < size_t(ng) * n_segs; ++i)
    if (members[i] != kNone && members[i] >= nq) return kEinval;
  const std::vector<DevQuery> qs = queries_of(k, nq);
  Dev dq(size_t(nq) * sizeof(DevQuery)), dm(size_t(ng) * n_segs * 4u), dh(size_t(ng) * (kBins + 2u) * 4u),
      db(size_t(nq) * 4u);
  Opt<uint32_t> dmb(min_bin, nq);
  if (!dq.up(qs.data()) || !dm.up(members) || !dh.up(group_hist) || !dmb.ok || !db.fill()) return kEdevice;
  RT_LAUNCH(k_group_threshold, ng, 64, 0, nullptr, dq.as<DevQuery>(), dm.as<uint32_t>(), n_segs, dh.as<uint32_t>(),
            margin, dmb.ptr(), db.as<uint32_t>());
  const int rc = finish();
  if (rc != kOk) return rc;
  return db.down(bstar) ? kOk : kEdevice;
}

// k_group_sums, then k_group_verdict on the sums (one rank: nothing is added in between).
// k, out_count, hits, bstar, min_bin (or null): [nq]; members: [ng][n_segs]; sums: [ng * 3 + 2];
// status: one word, in and out
int sp_group_verdict(const uint32_t* k, uint32_t nq, const uint32_t* members, uint32_t n_segs, uint32_t ng,
                     const uint32_t* out_count, const unsigned long long* hits, const uint32_t* bstar,
                     const uint32_t* min_bin, uint32_t* status, uint32_t* sums) {
  if (!k || !members || !out_count || !hits || !bstar || !status || !sums || !nq || !ng || !n_segs || ng > nq)
    return kEinval;
  for (size_t i = 0; i < size_t(ng) * n_segs; ++i)
    if (members[i] != kNone && members[i] >= nq) return kEinval;
  const std::vector<DevQuery> qs = queries_of(k, nq);
  const size_t sums_b = (size_t(ng) * kGroupSumWords + 2u) * 4u;
  Dev dq(size_t(nq) * sizeof(DevQuery)), dm(size_t(ng) * n_segs * 4u), doc(size_t(nq) * 4u), dh(size_t(nq) * 8u),
      db(size_t(nq) * 4u), dst(4), ds(sums_b);
  Opt<uint32_t> dmb(min_bin, nq);
  if (!dq.up(qs.data()) || !dm.up(members) || !doc.up(out_count) || !dh.up(hits) || !db.up(bstar) || !dmb.ok ||
      !dst.up(status) || !ds.fill())
    return kEdevice;
  RT_LAUNCH(k_group_sums, (ng + 63u) / 64u, 64, 0, nullptr, dq.as<DevQuery>(), dm.as<uint32_t>(), n_segs, ng,
            doc.as<uint32_t>(), dh.as<unsigned long long>(), db.as<uint32_t>(), dmb.ptr(), dst.as<uint32_t>(),
            ds.as<uint32_t>());
  if (!rt::last_error_ok()) return kEdevice;
  RT_LAUNCH(k_group_verdict, (ng + 63u) / 64u, 64, 0, nullptr, dq.as<DevQuery>(), ng, ds.as<uint32_t>(),
            dst.as<uint32_t>());
  const int rc = finish();
  if (rc != kOk) return rc;
  return ds.down(sums) && dst.down(status) ? kOk : kEdevice;
}

// conj_units: [nc]; item_base: [nc + 1], ascending, at most n_items; item_hits: [n_items]; hits: [nq]
int sp_conj_hits(const uint32_t* conj_units, const uint32_t* item_base, const uint32_t* item_hits, uint32_t nc,
                 uint32_t n_items, uint32_t nq, unsigned long long* hits) {
  if (!conj_units || !item_base || !item_hits || !hits || !nc || !nq) return kEinval;
  for (uint32_t c = 0; c < nc; ++c)
    if (conj_units[c] >= nq || item_base[c] > item_base[c + 1u] || item_base[c + 1u] > n_items) return kEinval;
  Dev du(size_t(nc) * 4u), dbase(size_t(nc + 1u) * 4u), di(size_t(n_items) * 4u), dh(size_t(nq) * 8u);
  if (!du.up(conj_units) || !dbase.up(item_base) || !di.up(item_hits) || !dh.fill()) return kEdevice;
  RT_LAUNCH(k_conj_hits, nc, 64, 0, nullptr, du.as<uint32_t>(), dbase.as<uint32_t>(), di.as<uint32_t>(),
            dh.as<unsigned long long>());
  const int rc = finish();
  if (rc != kOk) return rc;
  return dh.down(hits) ? kOk : kEdevice;
}

// acc, bs, bin_scale, fx_inv, val, bin, thr: [n]; wide: ACC = unsigned long long, else uint32_t
// (acc below 2^32)
int sp_bins(const unsigned long long* acc, const uint32_t* bs, const float* bin_scale, const float* fx_inv,
            uint32_t n, int wide, float* val, uint32_t* bin, unsigned long long* thr) {
  if (!acc || !bs || !bin_scale || !fx_inv || !val || !bin || !thr || !n) return kEinval;
  if (!wide)
    for (uint32_t i = 0; i < n; ++i)
      if (acc[i] >> 32) return kEinval;
  Dev da(size_t(n) * 8u), dbs(size_t(n) * 4u), dsc(size_t(n) * 4u), dfx(size_t(n) * 4u), dv(size_t(n) * 4u),
      dbin(size_t(n) * 4u), dt(size_t(n) * 8u);
  if (!da.up(acc) || !dbs.up(bs) || !dsc.up(bin_scale) || !dfx.up(fx_inv) || !dv.fill() || !dbin.fill() || !dt.fill())
    return kEdevice;
  if (wide)
    RT_LAUNCH(k_bins<unsigned long long>, (n + 255u) / 256u, 256, 0, nullptr, da.as<unsigned long long>(),
              dbs.as<uint32_t>(), dsc.as<float>(), dfx.as<float>(), n, dv.as<float>(), dbin.as<uint32_t>(),
              dt.as<unsigned long long>());
  else
    RT_LAUNCH(k_bins<uint32_t>, (n + 255u) / 256u, 256, 0, nullptr, da.as<unsigned long long>(),
              dbs.as<uint32_t>(), dsc.as<float>(), dfx.as<float>(), n, dv.as<float>(), dbin.as<uint32_t>(),
              dt.as<unsigned long long>());
  const int rc = finish();
  if (rc != kOk) return rc;
  return dv.down(val) && dbin.down(bin) && dt.down(thr) ? kOk : kEdevice;
}

}  // extern "C"
