// score_docs_shape.h — what irs_hip_batch_score_docs checks of a caller's doc lists, and how they are
// cut into the chunks k_score_docs (score_docs.h) takes a wavefront each.  Plain host code over
// plain arrays, nothing of the batch: it also builds on its own (tests/cpp/score_docs_shape_check.cpp
// runs it under the host sanitizers).
//
// Unit u's docs are docs[offsets[u] .. offsets[u + 1]): strictly ascending, each in 1..num_docs of
// the unit's segment (unit = segment * n_queries + query).  A chunk is at most kScoreDocsChunk
// consecutive docs of ONE unit's list: lists are cut at unit borders and every kScoreDocsChunk docs.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "irs_hip.h"

namespace irs_hip {

constexpr uint32_t kScoreDocsChunk = 128;            // docs of one chunk: a lane's two
constexpr uint64_t kScoreDocsMax = uint64_t(1) << 31;   // docs of one call, all units together

// One chunk as the host form hands it to the kernel
struct ScoreDocsChunk {
  uint32_t unit;
  uint32_t first;   // index of the chunk's first doc in `docs`
  uint32_t n;       // 1..kScoreDocsChunk
  uint32_t pad;
};
static_assert(sizeof(ScoreDocsChunk) == 16, "ScoreDocsChunk: 16 bytes");

// offsets[0 .. units]: starts at 0, never decreases; *total = offsets[units].  IRS_HIP_EINVAL, or
// IRS_HIP_EUNSUPPORTED for more than kScoreDocsMax docs in all (checked entry by entry: an offset
// near 2^64 never takes part in arithmetic).
inline int score_docs_offsets(const uint64_t* offsets, uint32_t units, uint64_t* total) {
  *total = 0;
  if (!offsets || offsets[0] != 0) return IRS_HIP_EINVAL;
  for (uint32_t u = 0; u < units; ++u)
    if (offsets[u + 1] < offsets[u]) return IRS_HIP_EINVAL;
  if (offsets[units] > kScoreDocsMax) return IRS_HIP_EUNSUPPORTED;
  *total = offsets[units];
  return IRS_HIP_OK;
}

// Every list strictly ascending and inside its segment: seg_docs[u / n_queries] = num_docs of unit
// u's segment.  (Offsets as score_docs_offsets left them.)
inline int score_docs_lists(const uint32_t* docs, const uint64_t* offsets, uint32_t units, uint32_t n_queries,
                            const uint32_t* seg_docs) {
  if (!docs || !n_queries) return IRS_HIP_EINVAL;
  for (uint32_t u = 0; u < units; ++u) {
    const uint32_t last = seg_docs[u / n_queries];
    uint32_t prev = 0;   // (a doc of 0 is not above it)
    for (uint64_t i = offsets[u]; i < offsets[u + 1]; ++i) {
      const uint32_t d = docs[i];
      if (d <= prev || d > last) return IRS_HIP_EINVAL;
      prev = d;
    }
  }
  return IRS_HIP_OK;
}

// The chunks of every list, unit after unit (an empty list has none)
inline void score_docs_cut(const uint64_t* offsets, uint32_t units, std::vector<ScoreDocsChunk>& out) {
  out.clear();
  for (uint32_t u = 0; u < units; ++u) {
    for (uint64_t at = offsets[u]; at < offsets[u + 1]; at += kScoreDocsChunk) {
      const uint64_t left = offsets[u + 1] - at;
      out.push_back(ScoreDocsChunk{u, uint32_t(at), uint32_t(left < kScoreDocsChunk ? left : kScoreDocsChunk), 0u});
    }
  }
}

// The device form has no chunk records: wavefront w of score_docs_grid(n_docs, units) finds its
// chunk from the offsets alone.  The chunks of unit u take the slots from score_docs_slot(offsets[u],
// u) on; the slots of two units never meet — floor(a / C) + ceil((b - a) / C) <= floor(b / C) + 1 for
// a <= b — and slot(u) grows strictly with u, so "the last unit whose first slot is <= w" is a
// binary search.
constexpr uint64_t score_docs_slot(uint64_t offset, uint32_t unit) { return offset / kScoreDocsChunk + unit; }
constexpr uint64_t score_docs_grid(uint64_t n_docs, uint32_t units) {
  return (n_docs + kScoreDocsChunk - 1u) / kScoreDocsChunk + units;
}

}  // namespace irs_hip
