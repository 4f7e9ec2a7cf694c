// tests/cpp/tree_shape_check.cpp — TEST: csrc/tree_shape.h on its own (tree_compile: what create
// checks of a query with IRS_HIP_TREE_NODE entries, and its node table; tree_eval: what the kernels
// compute per doc) over the shapes tests/test_boolean_trees.py sends through batch create, as a
// stand-alone program: built with -fsanitize=address,undefined by tests/test_boolean_trees_cpp.py
// (host code only; nothing here touches a device).  The table is held against a recursive walk of
// the prefix form written out here, for every presence mask of the tree's leaves.
#include <cstdio>
#include <vector>

#include "tree_shape.h"

using namespace irs_hip;

#define REQUIRE(c)                                                          \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #c); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

namespace {

constexpr int32_t TN = IRS_HIP_TREE_NODE, EX = IRS_HIP_EXCLUDE;
constexpr int32_t OR = IRS_HIP_OP_OR, AND = IRS_HIP_OP_AND, MM = IRS_HIP_OP_MINMATCH;

irs_hip_term_scorer leaf(bool neg = false) {
  irs_hip_term_scorer e{};
  e.term = 1;
  e.kind = neg ? EX : IRS_HIP_SCORE_BM25;
  e.c0 = 1.f;
  return e;
}

irs_hip_term_scorer node(int32_t op, uint32_t span, uint32_t mm = 0, bool neg = false) {
  irs_hip_term_scorer e{};
  e.term = IRS_HIP_NO_TERM;
  e.kind = TN | op | (neg ? EX : 0);
  e.phrase_offset = span | (mm << 16);
  return e;
}

irs_hip_query query(int32_t op, size_t n, uint32_t min_match = 0, uint32_t merge = IRS_HIP_MERGE_SUM) {
  irs_hip_query q{};
  q.op = op;
  q.n_terms = uint32_t(n);
  q.k = 10;
  q.min_match = min_match;
  q.merge = merge;
  return q;
}

using Entries = std::vector<irs_hip_term_scorer>;

int compile(int32_t op, const Entries& e, TreeTable& T, uint32_t min_match = 0, uint32_t merge = IRS_HIP_MERGE_SUM) {
  // (an exact-size copy: a read past the entries is the sanitizer's to see)
  Entries copy(e);
  copy.shrink_to_fit();
  return tree_compile(query(op, copy.size(), min_match, merge), copy.data(), T);
}

// The prefix form walked directly: does the node with children [lo, hi) match, and which positive
// leaves score under it.  `leaf_no` counts the leaves in prefix order as the walk passes them.
struct Walk {
  const Entries& e;
  uint32_t present;
  uint32_t leaf_no = 0;
  bool node_matches(uint32_t lo, uint32_t hi, int32_t op, uint32_t mm, uint32_t* scoring) {
    uint32_t n_pos = 0, n_match = 0, mine = 0;
    bool barred = false;
    for (uint32_t j = lo; j < hi;) {
      const int32_t kind = e[j].kind;
      bool m;
      uint32_t sub = 0, next = j + 1;
      bool neg;
      if (kind & TN) {
        const uint32_t span = e[j].phrase_offset & 0xFFFFu;
        neg = (kind & EX) != 0;
        m = node_matches(j + 1, j + 1 + span, kind & 0xFF, e[j].phrase_offset >> 16, &sub);
        next = j + 1 + span;
      } else {
        neg = kind == EX;
        const uint32_t bit = 1u << leaf_no++;
        m = (present & bit) != 0;
        sub = m ? bit : 0u;
      }
      if (neg) {
        barred = barred || m;
      } else {
        ++n_pos;
        n_match += m ? 1u : 0u;
        if (m) mine |= sub;
      }
      j = next;
    }
    const uint32_t need = op == AND ? n_pos : op == OR ? 1u : mm;
    const bool ok = n_match >= need && !barred;
    *scoring = ok ? mine : 0u;
    return ok;
  }
};

// every presence mask of the tree's leaves: tree_eval on the compiled table == the direct walk
bool same_everywhere(int32_t op, const Entries& e, uint32_t min_match = 0) {
  TreeTable T;
  if (compile(op, e, T, min_match) != IRS_HIP_OK) return false;
  for (uint32_t present = 0; present < (1u << T.n_leaves); ++present) {
    Walk w{e, present};
    uint32_t want = 0;
    const bool m = w.node_matches(0, uint32_t(e.size()), op, min_match, &want);
    const uint32_t got = tree_eval(T.node, T.n_nodes, present);
    if (got != (m ? want : 0u) || (m && want == 0u)) return false;   // (a hit always has a scoring leaf)
    if (got & T.negated) return false;
  }
  return true;
}

// a left-deep chain alternating And / Or over n leaves, the root being the last operator
Entries chain(uint32_t n, int32_t* root_op) {
  Entries e{leaf(), leaf()};   // t0 AND t1
  int32_t op = AND;
  for (uint32_t i = 2; i < n; ++i) {
    Entries up{node(op, uint32_t(e.size()))};
    up.insert(up.end(), e.begin(), e.end());
    up.push_back(leaf());
    e.swap(up);
    op = i % 2 == 0 ? OR : AND;
  }
  *root_op = op;
  return e;
}

}  // namespace

int main() {
  TreeTable T;
  // a AND (b OR (c AND d))
  const Entries nest{leaf(), node(OR, 4), leaf(), node(AND, 2), leaf(), leaf()};
  REQUIRE(compile(AND, nest, T) == IRS_HIP_OK);
  REQUIRE(T.n_nodes == 3 && T.n_leaves == 4 && T.n_entries == 2 && T.negated == 0);
  REQUIRE(T.leaf_at[0] == 0 && T.leaf_at[1] == 2 && T.leaf_at[2] == 4 && T.leaf_at[3] == 5);
  // children before parents, the root last
  REQUIRE(T.node[0].type == kTreeAnd && T.node[0].pos_leaves == 0xC && T.node[0].min_match == 2);
  REQUIRE(T.node[1].type == kTreeOr && T.node[1].pos_leaves == 0x2 && T.node[1].pos_nodes == 0x1 && T.node[1].min_match == 1);
  REQUIRE(T.node[2].type == kTreeAnd && T.node[2].pos_leaves == 0x1 && T.node[2].pos_nodes == 0x2 && T.node[2].min_match == 2);
  REQUIRE(tree_eval(T.node, T.n_nodes, 0x1) == 0 && tree_eval(T.node, T.n_nodes, 0x3) == 0x3);
  REQUIRE(tree_eval(T.node, T.n_nodes, 0x5) == 0 && tree_eval(T.node, T.n_nodes, 0xD) == 0xD);
  REQUIRE(tree_eval(T.node, T.n_nodes, 0x7) == 0x3);   // c without d: c does not score
  REQUIRE(same_everywhere(AND, nest));
  // (a AND NOT b) OR c; a AND NOT (b AND c); +a +(b c d)~2; Or([And(a, b), c, Or(d, e)], 2)
  const Entries andnot{node(AND, 2), leaf(), leaf(true), leaf()};
  REQUIRE(compile(OR, andnot, T) == IRS_HIP_OK && T.negated == 0x2 && T.node[0].neg_leaves == 0x2);
  REQUIRE(tree_eval(T.node, T.n_nodes, 0x7) == 0x4 && tree_eval(T.node, T.n_nodes, 0x1) == 0x1);
  REQUIRE(same_everywhere(OR, andnot));
  const Entries notand{leaf(), node(AND, 2, 0, true), leaf(), leaf()};
  REQUIRE(compile(AND, notand, T) == IRS_HIP_OK && T.node[1].neg_nodes == 0x1);
  REQUIRE(same_everywhere(AND, notand));
  const Entries mmgroup{leaf(), node(MM, 3, 2), leaf(), leaf(), leaf()};
  REQUIRE(same_everywhere(AND, mmgroup));
  const Entries mixed{node(AND, 2), leaf(), leaf(), leaf(), node(OR, 2), leaf(), leaf()};
  REQUIRE(same_everywhere(MM, mixed, 2));
  REQUIRE(same_everywhere(MM, mixed, 3) && same_everywhere(MM, mixed, 4));   // (4: above its children, never)
  const Entries above{leaf(), node(MM, 2, 0xFFFF), leaf(), leaf()};
  REQUIRE(compile(AND, above, T) == IRS_HIP_OK && T.node[0].min_match == 255);
  REQUIRE(same_everywhere(AND, above));
  REQUIRE(compile(MM, nest, T, 0xFFFFFFFFu) == IRS_HIP_OK && T.node[2].min_match == 255);

  // IRS_HIP_EINVAL: spans, node ops, min_match on the wrong node, Nots under an Or node, the flag
  // under other ops and next to other flags
  Entries bad = nest;
  bad[3].phrase_offset = 3;
  REQUIRE(compile(AND, bad, T) == IRS_HIP_EINVAL);
  bad = nest;
  bad[1].phrase_offset = 5;
  REQUIRE(compile(AND, bad, T) == IRS_HIP_EINVAL);
  bad = nest;
  bad[3].phrase_offset = 0;
  REQUIRE(compile(AND, bad, T) == IRS_HIP_EINVAL);
  bad = nest;
  bad.back() = node(AND, 1);   // a node entry at the very end: its span runs past the query
  REQUIRE(compile(AND, bad, T) == IRS_HIP_EINVAL);
  for (int32_t op : {int32_t(IRS_HIP_OP_PHRASE), int32_t(IRS_HIP_OP_MULTITERM), 5, 0xFF}) {
    bad = nest;
    bad[3].kind = TN | op;
    REQUIRE(compile(AND, bad, T) == IRS_HIP_EINVAL);
    REQUIRE(compile(op, nest, T) == IRS_HIP_EINVAL);
  }
  bad = nest;
  bad[1].phrase_offset = 4 | (1u << 16);
  REQUIRE(compile(AND, bad, T) == IRS_HIP_EINVAL);
  bad = nest;
  bad[2] = leaf(true);
  REQUIRE(compile(AND, bad, T) == IRS_HIP_EINVAL);
  bad = nest;
  bad[3].kind |= EX;
  REQUIRE(compile(AND, bad, T) == IRS_HIP_EINVAL);
  for (int32_t flag : {0x200, 0x400, 0x800, 0x1000, 0x2000, 0x4000}) {
    bad = nest;
    bad[3].kind |= flag;
    REQUIRE(compile(AND, bad, T) == IRS_HIP_EINVAL);
    bad = nest;
    bad[4].kind |= flag;
    REQUIRE(compile(AND, bad, T) == IRS_HIP_EINVAL);
  }
  REQUIRE(tree_compile(query(AND, 0), nest.data(), T) == IRS_HIP_EINVAL);
  // ... also behind something that is only unsupported
  bad = nest;
  bad[0] = leaf(true);
  bad[3].phrase_offset = 0;
  REQUIRE(compile(OR, bad, T) == IRS_HIP_EINVAL);

  // IRS_HIP_EUNSUPPORTED
  REQUIRE(compile(AND, nest, T, 0, IRS_HIP_MERGE_MAX) == IRS_HIP_EUNSUPPORTED);
  REQUIRE(compile(AND, nest, T, 0, IRS_HIP_MERGE_MIN) == IRS_HIP_EUNSUPPORTED);
  bad = nest;
  bad[4] = bad[5] = leaf(true);
  REQUIRE(compile(AND, bad, T) == IRS_HIP_EUNSUPPORTED);            // an And node of only Nots
  const Entries nots{leaf(true), node(OR, 2, 0, true), leaf(), leaf()};
  REQUIRE(compile(AND, nots, T) == IRS_HIP_EUNSUPPORTED);           // ... the root
  bad = nest;
  bad[0] = leaf(true);
  REQUIRE(compile(OR, bad, T) == IRS_HIP_EUNSUPPORTED);             // a Not under the root Or
  REQUIRE(compile(MM, bad, T, 1) == IRS_HIP_EUNSUPPORTED);
  REQUIRE(compile(AND, bad, T) == IRS_HIP_OK);
  bad = nest;
  bad[1] = node(MM, 4, 0);
  REQUIRE(compile(AND, bad, T) == IRS_HIP_EUNSUPPORTED);            // a MINMATCH node with min_match 0
  REQUIRE(compile(MM, nest, T, 0) == IRS_HIP_EUNSUPPORTED);
  REQUIRE(compile(MM, nest, T, 1) == IRS_HIP_OK);

  // the limits: 16 leaves, 15 node entries; chains of every length against the walk
  int32_t op = 0;
  for (uint32_t n = 2; n <= 16; ++n) {
    const Entries c = chain(n, &op);
    REQUIRE(same_everywhere(op, c));
  }
  const Entries c16 = chain(16, &op);
  REQUIRE(compile(op, c16, T) == IRS_HIP_OK && T.n_leaves == 16 && T.n_entries == 14 && T.n_nodes == 15);
  REQUIRE(tree_eval(T.node, T.n_nodes, 0xFFFF) != 0);
  const Entries c17 = chain(17, &op);
  REQUIRE(compile(op, c17, T) == IRS_HIP_EUNSUPPORTED);
  Entries c14 = chain(14, &op);   // 13 operators: 12 node entries
  Entries full{node(op, uint32_t(c14.size()))};
  full.insert(full.end(), c14.begin(), c14.end());
  full.push_back(node(OR, 1));
  full.push_back(leaf());
  full.push_back(node(OR, 1));
  full.push_back(leaf());
  REQUIRE(compile(OR, full, T) == IRS_HIP_OK && T.n_leaves == 16 && T.n_entries == 15 && T.n_nodes == 16);
  REQUIRE(same_everywhere(OR, full));
  Entries over = full;
  over.back() = node(OR, 1);
  over.push_back(leaf());
  over[over.size() - 3].phrase_offset = 2;
  REQUIRE(compile(OR, over, T) == IRS_HIP_EUNSUPPORTED);           // 16 node entries
  Entries deep{leaf()};
  for (int i = 0; i < 100; ++i) deep.insert(deep.begin(), node(OR, uint32_t(deep.size())));
  REQUIRE(compile(OR, deep, T) == IRS_HIP_EUNSUPPORTED);           // 100 nested node entries
  Entries many(40, leaf());
  many[0] = node(AND, 39);
  REQUIRE(compile(OR, many, T) == IRS_HIP_EUNSUPPORTED);           // 39 leaves
  REQUIRE(!tree_flagged(many.data() + 1, 39) && tree_flagged(many.data(), 40) && !tree_flagged(many.data(), 0));
  std::printf("tree_shape_check OK\n");
  return 0;
}
