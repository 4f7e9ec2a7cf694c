// tests/cpp/clause_shape_check.cpp — TEST: csrc/clause_shape.h on its own (clause_shape_ok, the
// clause of every entry, the need-masks of a unit's rows) over the shapes tests/test_or_clauses.py
// sends through batch create, as a stand-alone program: built with -fsanitize=address,undefined by
// tests/test_or_clauses_cpp.py (host code only; nothing here touches a device).
#include <cstdio>
#include <vector>

#include "clause_shape.h"

using namespace irs_hip;

#define REQUIRE(c)                                                          \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #c); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

namespace {

constexpr int32_t CL = IRS_HIP_CLAUSE_AND;

// entries of kind BM25, `flags[j]` OR-ed in
std::vector<irs_hip_term_scorer> entries(const std::vector<int32_t>& flags) {
  std::vector<irs_hip_term_scorer> e(flags.size());
  for (size_t j = 0; j < flags.size(); ++j) {
    e[j] = irs_hip_term_scorer{};
    e[j].term = uint32_t(j);
    e[j].kind = IRS_HIP_SCORE_BM25 | flags[j];
    e[j].c0 = 1.f;
  }
  return e;
}

irs_hip_query query(int32_t op, uint32_t n, uint32_t min_match = 1, uint32_t merge = IRS_HIP_MERGE_SUM) {
  irs_hip_query q{};
  q.op = op;
  q.n_terms = n;
  q.k = 10;
  q.min_match = min_match;
  q.merge = merge;
  return q;
}

}  // namespace

int main() {
  // (a AND b) OR c
  auto abc = entries({0, CL, 0});
  REQUIRE(clause_shape_ok(query(IRS_HIP_OP_OR, 3), abc.data(), 3, 0) == IRS_HIP_OK);
  REQUIRE(clause_shape_ok(query(IRS_HIP_OP_MINMATCH, 3, 2), abc.data(), 3, 0) == IRS_HIP_OK);
  REQUIRE(clause_shape_ok(query(IRS_HIP_OP_MINMATCH, 3, 3), abc.data(), 3, 0) == IRS_HIP_OK);
  // the flag on the first entry, on an excluded kind, under AND / PHRASE / MULTITERM
  auto first = entries({CL, CL, 0});
  REQUIRE(clause_shape_ok(query(IRS_HIP_OP_OR, 3), first.data(), 3, 0) == IRS_HIP_EINVAL);
  auto excl = entries({0, 0, 0});
  excl[2].kind = IRS_HIP_EXCLUDE | CL;
  REQUIRE(clause_shape_ok(query(IRS_HIP_OP_OR, 3), excl.data(), 3, 0) == IRS_HIP_EINVAL);
  for (int32_t op : {IRS_HIP_OP_AND, IRS_HIP_OP_PHRASE, IRS_HIP_OP_MULTITERM})
    REQUIRE(clause_shape_ok(query(op, 3), abc.data(), 3, 0) == IRS_HIP_EINVAL);
  REQUIRE(clause_shape_ok(query(IRS_HIP_OP_OR, 0), abc.data(), 0, 0) == IRS_HIP_EINVAL);
  // 16 entries taken, 17 refused; MAX / MIN; an excluded entry behind
  std::vector<int32_t> f16(16, 0), f17(17, 0);
  f16[1] = f17[1] = CL;
  auto e16 = entries(f16), e17 = entries(f17);
  REQUIRE(clause_shape_ok(query(IRS_HIP_OP_OR, 16), e16.data(), 16, 0) == IRS_HIP_OK);
  REQUIRE(clause_shape_ok(query(IRS_HIP_OP_OR, 17), e17.data(), 17, 0) == IRS_HIP_EUNSUPPORTED);
  REQUIRE(clause_shape_ok(query(IRS_HIP_OP_OR, 3, 1, IRS_HIP_MERGE_MAX), abc.data(), 3, 0) == IRS_HIP_EUNSUPPORTED);
  REQUIRE(clause_shape_ok(query(IRS_HIP_OP_OR, 3, 1, IRS_HIP_MERGE_MIN), abc.data(), 3, 0) == IRS_HIP_EUNSUPPORTED);
  REQUIRE(clause_shape_ok(query(IRS_HIP_OP_OR, 4), abc.data(), 3, 1) == IRS_HIP_EUNSUPPORTED);

  // the clause of every entry: a clause of 16, 8 of 2, 1 of 2 plus 14 single terms
  uint32_t of[16];
  std::vector<int32_t> conj(16, CL), pairs(16, 0), tail(16, 0);
  conj[0] = 0;
  for (int j = 1; j < 16; j += 2) pairs[size_t(j)] = CL;
  tail[1] = CL;
  auto e = entries(conj);
  REQUIRE(clause_of_entries(e.data(), 16, of) == 1 && of[0] == 0 && of[15] == 0);
  e = entries(pairs);
  REQUIRE(clause_of_entries(e.data(), 16, of) == 8 && of[0] == 0 && of[1] == 0 && of[14] == 7 && of[15] == 7);
  e = entries(tail);
  REQUIRE(clause_of_entries(e.data(), 16, of) == 15 && of[1] == 0 && of[2] == 1 && of[15] == 14);
  REQUIRE(clause_of_entries(e.data(), 0, of) == 0);

  // need-masks: every row's mask holds its own bit; the rows of one clause share one mask; a
  // clause whose middle rows are gone (a dead clause between two live ones) keeps the numbering
  uint32_t mask[16];
  const uint32_t rows16[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  clause_masks(rows16, 16, mask);
  for (int r = 0; r < 16; ++r) REQUIRE(mask[r] == 0xFFFFu);
  const uint32_t rows8[16] = {0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7};
  clause_masks(rows8, 16, mask);
  for (uint32_t r = 0; r < 16; ++r) REQUIRE(mask[r] == (3u << (r & ~1u)));
  const uint32_t gaps[5] = {0, 0, 2, 5, 5};   // clauses 1, 3 and 4 are empty here
  clause_masks(gaps, 5, mask);
  REQUIRE(mask[0] == 3u && mask[1] == 3u && mask[2] == 4u && mask[3] == 24u && mask[4] == 24u);
  const uint32_t shared[4] = {0, 1, 0, 1};    // (members of one clause need not be neighbours)
  clause_masks(shared, 4, mask);
  REQUIRE(mask[0] == 5u && mask[1] == 10u && mask[2] == 5u && mask[3] == 10u);
  clause_masks(gaps, 0, mask);
  std::printf("clause_shape_check OK\n");
  return 0;
}
