// tree_shape.h — what create checks of a tree query (entries with IRS_HIP_TREE_NODE), and the node
// table of its unit (tree.h).  Plain host code over the API's records, nothing of the batch: it also
// builds on its own (tests/cpp/tree_shape_check.cpp runs it under the host sanitizers).
//
// The prefix form — the root's children in order, a node entry followed by the `span` entries of its
// subtree — is compiled to at most 16 node records in children-before-parents order, the root last.
// A record's masks are over the query's LEAVES (bit l = the l-th leaf entry in prefix order, positive
// and negated alike: the presence mask k_tree_score keeps per doc) and over the RECORDS before it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "irs_hip.h"

namespace irs_hip {

constexpr uint32_t kTreeMaxLeaves = 16;   // the low 16 bits of a doc's sum
constexpr uint32_t kTreeMaxNodes = 16;    // the root and up to 15 node entries
enum : uint8_t { kTreeOr = 0, kTreeAnd = 1 };

// One node: it matches a doc iff at least `min_match` of its positive children do — an And: all of
// them (min_match = their number), an Or: 1, a min-match Or: its min_match, 255 where the entry
// asks for more than that — and none of its negated children does.
struct TreeNode {
  uint16_t pos_leaves, neg_leaves;   // over the leaves
  uint16_t pos_nodes, neg_nodes;     // over the records before this one
  uint8_t type;                      // kTreeOr / kTreeAnd
  uint8_t min_match;
  uint16_t pad0;
  uint32_t pad1;
};
static_assert(sizeof(TreeNode) == 16, "TreeNode: 16 bytes");

struct TreeTable {
  TreeNode node[kTreeMaxNodes];
  uint32_t n_nodes = 0;    // records, the root last (counted on past kTreeMaxNodes)
  uint32_t n_leaves = 0;   // leaf entries (counted on past kTreeMaxLeaves)
  uint32_t n_entries = 0;  // node entries
  uint32_t leaf_at[kTreeMaxLeaves];   // the entry of leaf l, relative to the query's first
  uint16_t negated = 0;    // bit l: leaf l is an IRS_HIP_EXCLUDE entry
  bool unsupported = false;
};

constexpr int32_t kTreeShapeFlags = 0x200 | 0x400 | 0x800 | IRS_HIP_CLAUSE_AND | 0x2000 | 0x4000;

// Does any entry of the query carry IRS_HIP_TREE_NODE
inline bool tree_flagged(const irs_hip_term_scorer* ents, uint32_t n) {
  for (uint32_t j = 0; j < n; ++j)
    if (ents[j].kind & IRS_HIP_TREE_NODE) return true;
  return false;
}

inline bool tree_op_ok(int32_t op) {
  return op == IRS_HIP_OP_OR || op == IRS_HIP_OP_AND || op == IRS_HIP_OP_MINMATCH;
}

// The children [lo, hi) of one node (`root`: the query's) into a record; returns IRS_HIP_EINVAL or
// IRS_HIP_OK and the record's index in *at.  What is only unsupported is noted in T and the walk
// goes on: an illegal entry further on still answers IRS_HIP_EINVAL.
inline int tree_node(const irs_hip_term_scorer* ents, uint32_t lo, uint32_t hi, int32_t op, uint32_t min_match,
                     bool root, uint32_t depth, TreeTable& T, uint32_t* at) {
  TreeNode nd{};
  uint32_t n_pos = 0;
  for (uint32_t j = lo; j < hi;) {
    const int32_t kind = ents[j].kind;
    const bool node = (kind & IRS_HIP_TREE_NODE) != 0;
    const bool neg = node ? (kind & IRS_HIP_EXCLUDE) != 0 : kind == IRS_HIP_EXCLUDE;
    if (kind & kTreeShapeFlags) return IRS_HIP_EINVAL;
    if (neg && op != IRS_HIP_OP_AND) {   // an Or's Not child: all docs but some, not a posting-list query
      if (!root) return IRS_HIP_EINVAL;
      T.unsupported = true;
    }
    if (!node) {
      const uint32_t l = T.n_leaves++;
      if (l < kTreeMaxLeaves) {
        T.leaf_at[l] = j;
        (neg ? nd.neg_leaves : nd.pos_leaves) |= uint16_t(1u << l);
        if (neg) T.negated |= uint16_t(1u << l);
      }
      n_pos += neg ? 0u : 1u;
      ++j;
      continue;
    }
    const int32_t nop = kind & 0xFF;
    const uint32_t span = ents[j].phrase_offset & 0xFFFFu, mm = ents[j].phrase_offset >> 16;
    if ((kind & ~(IRS_HIP_TREE_NODE | IRS_HIP_EXCLUDE | 0xFF)) || !tree_op_ok(nop)) return IRS_HIP_EINVAL;
    if (span == 0 || span > hi - (j + 1u)) return IRS_HIP_EINVAL;
    if (nop != IRS_HIP_OP_MINMATCH && mm != 0) return IRS_HIP_EINVAL;
    if (nop == IRS_HIP_OP_MINMATCH && mm == 0) T.unsupported = true;   // (the all-docs filter, as for every MINMATCH)
    ++T.n_entries;
    if (depth + 1u >= kTreeMaxNodes) {   // (deeper than 15 node entries can nest: too many of them)
      T.unsupported = true;
      T.n_entries = kTreeMaxNodes;
      j += 1u + span;
      continue;
    }
    uint32_t child = 0;
    if (const int rc = tree_node(ents, j + 1u, j + 1u + span, nop, mm, false, depth + 1u, T, &child)) return rc;
    if (child < kTreeMaxNodes) (neg ? nd.neg_nodes : nd.pos_nodes) |= uint16_t(1u << child);
    n_pos += neg ? 0u : 1u;
    j += 1u + span;
  }
  if (op == IRS_HIP_OP_AND && n_pos == 0) T.unsupported = true;   // (an And of Nots: all docs but some)
  nd.type = op == IRS_HIP_OP_AND ? kTreeAnd : kTreeOr;
  const uint32_t need = op == IRS_HIP_OP_AND ? n_pos : op == IRS_HIP_OP_OR ? 1u : min_match;
  nd.min_match = uint8_t(need < 255u ? need : 255u);
  *at = T.n_nodes++;
  if (*at < kTreeMaxNodes) T.node[*at] = nd;
  return IRS_HIP_OK;
}

// A query with node entries `ents[0, in.n_terms)`: checked and compiled.  IRS_HIP_EINVAL /
// IRS_HIP_EUNSUPPORTED as include/irs_hip.h lists them under IRS_HIP_TREE_NODE; the per-term rules
// are wide_terms_ok's.
inline int tree_compile(const irs_hip_query& in, const irs_hip_term_scorer* ents, TreeTable& T) {
  T = TreeTable{};
  if (!tree_op_ok(in.op) || in.n_terms == 0) return IRS_HIP_EINVAL;   // (PHRASE, MULTITERM, unknown ops)
  uint32_t root = 0;
  if (const int rc = tree_node(ents, 0, in.n_terms, in.op, in.min_match, true, 0, T, &root)) return rc;
  if (in.op == IRS_HIP_OP_MINMATCH && in.min_match == 0) T.unsupported = true;
  if (T.n_leaves > kTreeMaxLeaves || T.n_entries >= kTreeMaxNodes || in.merge != IRS_HIP_MERGE_SUM)
    T.unsupported = true;
  return T.unsupported ? IRS_HIP_EUNSUPPORTED : IRS_HIP_OK;
}

// What the kernels compute per doc, stated once on the host (the tests' stand-alone program checks
// the compiled table with it): `present` = the leaves that hold the doc.  Returns the scoring mask:
// the positive leaves present under active nodes — a node is active when it matches and every
// ancestor up to the root does — or 0 when the root does not match.
inline uint32_t tree_eval(const TreeNode* node, uint32_t n_nodes, uint32_t present) {
  uint32_t sat = 0;
  for (uint32_t i = 0; i < n_nodes; ++i) {
    const TreeNode& nd = node[i];
    const uint32_t cnt = uint32_t(__builtin_popcount(present & nd.pos_leaves)) + uint32_t(__builtin_popcount(sat & nd.pos_nodes));
    const bool ok = cnt >= nd.min_match && !(present & nd.neg_leaves) && !(sat & nd.neg_nodes);
    sat |= uint32_t(ok) << i;
  }
  if (n_nodes == 0 || !((sat >> (n_nodes - 1u)) & 1u)) return 0u;
  uint32_t active = 1u << (n_nodes - 1u), score = 0;
  for (uint32_t i = n_nodes; i-- > 0;) {
    if (!((active >> i) & 1u)) continue;
    score |= present & node[i].pos_leaves;
    active |= sat & node[i].pos_nodes;
  }
  return score;
}

}  // namespace irs_hip
