// tests/probe/tree_probe.hip — TEST INFRASTRUCTURE ONLY, in the manner of select_probe.hip: the
// device copy of the node-table walk (tree.h tree_table + tree_scoring_mask), UNMODIFIED, on the
// table tree_compile (tree_shape.h, unmodified) makes of the caller's query record and entries —
// once per presence mask p < 2^n_leaves — and beside it the host's tree_eval of the same table for
// the same masks.  tests/test_tree_layer.py builds this file the way the CPU emulator is built (g++,
// tests/sim) and for gfx950 (hipcc) and holds both results to one plain statement over the filter
// objects.  The product library never sees this file.
//
// The kernel runs as k_tree_pilot / k_tree_score do: kWideThreads threads, TreeOff::end bytes of
// dynamic LDS obtained as plan_tree.h obtains them, the table at TreeOff::nodes, a barrier behind
// tree_table.  Sizes are checked before anything is launched; the output is pre-filled with 0xEE.
#include "gpu_rt.h"
#include "types.h"
#include "tree.h"

#include <cstdint>
#include <cstring>
#include <vector>

namespace probe {

using namespace irs_hip;

enum : int { kOk = 0, kEinval = -1, kEdevice = -2 };
constexpr uint32_t kMaskBlocks = 64;   // 2^16 masks: one per thread

// out[p] = tree_scoring_mask(p) for p < n_masks; every workgroup holds the table in its own LDS
__global__ void __launch_bounds__(kWideThreads)
k_tree_masks(const TreeNode* nodes, uint32_t n_nodes, uint32_t n_masks, uint32_t* out) {
  RT_DYN_SMEM(smem);
  tree_table(smem, nodes, n_nodes);
  __syncthreads();
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_masks; p += gridDim.x * blockDim.x)
    out[p] = tree_scoring_mask(smem, n_nodes, p);
}

struct Dev {   // a device buffer that frees itself
  void* p = nullptr;
  size_t n = 0;
  explicit Dev(size_t bytes) : p(rt::dmalloc(bytes)), n(bytes) {}
  ~Dev() { rt::dfree(p); }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  template<typename T> T* as() const { return static_cast<T*>(p); }
  bool up(const void* h) const { return p && rt::h2d(p, h, n, nullptr) && rt::sync(nullptr); }
  bool fill() const { return p && rt::dmemset(p, 0xEE, n, nullptr) && rt::sync(nullptr); }
  bool down(void* h) const { return p && rt::d2h(h, p, n, nullptr) && rt::sync(nullptr); }
};

}  // namespace probe

using namespace probe;

extern "C" {

int tp_arch(char* buf, size_t cap) {
  return buf && cap && rt::device_count() > 0 && rt::set_device(0) && rt::device_arch(0, buf, cap) ? kOk : kEdevice;
}

// sizeof(TreeTable), TreeOff::nodes, TreeOff::end, kWideThreads: what the module pins
void tp_layout(uint32_t* out4) {
  out4[0] = uint32_t(sizeof(TreeTable));
  out4[1] = TreeOff::nodes;
  out4[2] = TreeOff::end;
  out4[3] = kWideThreads;
}

// query: the record, n_terms entries at ents (first_term is not followed); *status: tree_compile's;
// table: sizeof(TreeTable) bytes; dev, host: [n_masks] — written only when *status is IRS_HIP_OK, and
// then n_masks must be 2^n_leaves
int tp_tree(const irs_hip_query* query, const irs_hip_term_scorer* ents, uint32_t n_ents, int* status,
            void* table, uint32_t table_bytes, uint32_t* dev, uint32_t* host, uint32_t n_masks) {
  if (!query || !ents || !status || !table || !dev || !host) return kEinval;
  if (table_bytes != sizeof(TreeTable) || query->n_terms != n_ents) return kEinval;
  TreeTable T;
  *status = tree_compile(*query, ents, T);
  std::memcpy(table, &T, sizeof(TreeTable));
  if (*status != IRS_HIP_OK) return kOk;
  if (T.n_nodes == 0 || T.n_nodes > kTreeMaxNodes || T.n_leaves == 0 || T.n_leaves > kTreeMaxLeaves) return kEinval;
  if (n_masks != 1u << T.n_leaves) return kEinval;
  for (uint32_t p = 0; p < n_masks; ++p) host[p] = tree_eval(T.node, T.n_nodes, p);
  Dev dn(sizeof(TreeNode) * kTreeMaxNodes), dout(size_t(n_masks) * 4u);
  if (!dn.up(T.node) || !dout.fill()) return kEdevice;
  const size_t smem = TreeOff::end;
  if (!rt::allow_dynamic_smem(reinterpret_cast<const void*>(k_tree_masks), smem)) return kEdevice;
  const uint32_t grid = (n_masks + kWideThreads - 1u) / kWideThreads;
  RT_LAUNCH(k_tree_masks, grid < kMaskBlocks ? grid : kMaskBlocks, kWideThreads, smem, nullptr,
            dn.as<TreeNode>(), T.n_nodes, n_masks, dout.as<uint32_t>());
  if (!rt::sync(nullptr) || !rt::last_error_ok()) return kEdevice;
  return dout.down(dev) ? kOk : kEdevice;
}

}  // extern "C"
