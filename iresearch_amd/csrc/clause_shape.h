// clause_shape.h — what create checks of a query with IRS_HIP_CLAUSE_AND entries, and the clause
// table of its unit (clauses.h).  Plain host code over the API's records, nothing of the batch: it
// also builds on its own (tests/cpp/clause_shape_check.cpp runs it under the host sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>

#include "irs_hip.h"

namespace irs_hip {

// An Or / min-match Or whose included entries `ents` (n_incl of them, n_excl IRS_HIP_EXCLUDE entries
// behind) carry IRS_HIP_CLAUSE_AND somewhere: an entry without the flag opens a clause, one with it
// is one more required member.  IRS_HIP_EINVAL: the flag under another op, on the first entry, on
// an IRS_HIP_EXCLUDE kind.  IRS_HIP_EUNSUPPORTED: more entries than the 16 bits of a doc's presence
// mask, a merge other than SUM, excluded terms (a mask of the unit's own cannot ride on the streams
// every unit shares).  The per-term rules are wide_terms_ok's.
inline int clause_shape_ok(const irs_hip_query& in, const irs_hip_term_scorer* ents, uint32_t n_incl,
                           uint32_t n_excl) {
  if (in.op != IRS_HIP_OP_OR && in.op != IRS_HIP_OP_MINMATCH) return IRS_HIP_EINVAL;
  if (n_incl == 0 || (ents[0].kind & IRS_HIP_CLAUSE_AND)) return IRS_HIP_EINVAL;
  for (uint32_t j = 0; j < n_incl; ++j)
    if ((ents[j].kind & IRS_HIP_CLAUSE_AND) && (ents[j].kind & IRS_HIP_EXCLUDE)) return IRS_HIP_EINVAL;
  if (n_incl > IRS_HIP_MAX_TERMS || n_excl || in.merge != IRS_HIP_MERGE_SUM) return IRS_HIP_EUNSUPPORTED;
  return IRS_HIP_OK;
}

// The clause of every included entry: clause_of[j] for j < n_incl.  Returns the clauses.
inline uint32_t clause_of_entries(const irs_hip_term_scorer* ents, uint32_t n_incl, uint32_t* clause_of) {
  uint32_t n = 0;
  for (uint32_t j = 0; j < n_incl; ++j) {
    if (!(ents[j].kind & IRS_HIP_CLAUSE_AND) || n == 0) ++n;
    clause_of[j] = n - 1u;
  }
  return n;
}

// The need-masks of a unit's rows (at most 16: lane j = row j of k_clause_score): mask[r] = the rows
// of r's clause, bit r among them.  A row that is the lowest bit of its mask opens its clause — the
// kernels build their clause table from that.
inline void clause_masks(const uint32_t* row_clause, size_t n_rows, uint32_t* mask) {
  for (size_t r = 0; r < n_rows; ++r) {
    uint32_t m = 0;
    for (size_t x = 0; x < n_rows; ++x)
      if (row_clause[x] == row_clause[r]) m |= 1u << x;
    mask[r] = m;
  }
}

}  // namespace irs_hip
