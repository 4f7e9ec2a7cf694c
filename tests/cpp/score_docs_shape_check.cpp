// tests/cpp/score_docs_shape_check.cpp — TEST: csrc/score_docs_shape.h on its own (host code only,
// no device): what irs_hip_batch_score_docs checks of the caller's offsets and doc lists, the chunks
// the lists are cut into — at 0 / 1 / 128 / 129 docs and at unit borders — offsets that would
// overflow, and the device form's slot rule held against the chunk list for many shapes.  Built with
// -fsanitize=address,undefined by tests/test_score_docs_cpp.py; every array here is sized exactly,
// so a read past an end is reported.
#include <cstdio>
#include <memory>
#include <vector>

#include "score_docs_shape.h"

using namespace irs_hip;

#define REQUIRE(c)                                                          \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #c); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

namespace {

// heap copies of exactly n elements: the sanitizer sees every access past them
template<typename T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(new T[v.size()]);
  for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
  return p;
}

int offsets_rc(const std::vector<uint64_t>& offs, uint64_t* total) {
  const auto p = exact(offs);
  return score_docs_offsets(p.get(), uint32_t(offs.size() - 1), total);
}

int lists_rc(const std::vector<uint32_t>& docs, const std::vector<uint64_t>& offs, uint32_t nq,
             const std::vector<uint32_t>& seg_docs) {
  const auto d = exact(docs), s = exact(seg_docs);
  const auto o = exact(offs);
  return score_docs_lists(d.get(), o.get(), uint32_t(offs.size() - 1), nq, s.get());
}

std::vector<ScoreDocsChunk> cut(const std::vector<uint64_t>& offs) {
  const auto o = exact(offs);
  std::vector<ScoreDocsChunk> out;
  score_docs_cut(o.get(), uint32_t(offs.size() - 1), out);
  return out;
}

}  // namespace

int main() {
  uint64_t total = 99;
  // offsets
  REQUIRE(offsets_rc({0}, &total) == IRS_HIP_OK && total == 0);                  // no unit at all
  REQUIRE(offsets_rc({0, 0, 0}, &total) == IRS_HIP_OK && total == 0);            // every list empty
  REQUIRE(offsets_rc({0, 3, 3, 10}, &total) == IRS_HIP_OK && total == 10);
  REQUIRE(offsets_rc({1, 3, 3, 10}, &total) == IRS_HIP_EINVAL && total == 0);    // offsets[0] != 0
  REQUIRE(offsets_rc({0, 3, 2, 10}, &total) == IRS_HIP_EINVAL);                  // decreasing
  REQUIRE(offsets_rc({0, 5, 4}, &total) == IRS_HIP_EINVAL);
  REQUIRE(score_docs_offsets(nullptr, 3, &total) == IRS_HIP_EINVAL);
  REQUIRE(offsets_rc({0, kScoreDocsMax}, &total) == IRS_HIP_OK && total == kScoreDocsMax);
  REQUIRE(offsets_rc({0, kScoreDocsMax + 1}, &total) == IRS_HIP_EUNSUPPORTED && total == 0);
  // offsets that would overflow any sum or 32-bit index: refused, never added to
  REQUIRE(offsets_rc({0, ~uint64_t(0)}, &total) == IRS_HIP_EUNSUPPORTED);
  REQUIRE(offsets_rc({0, ~uint64_t(0), ~uint64_t(0)}, &total) == IRS_HIP_EUNSUPPORTED);
  REQUIRE(offsets_rc({0, ~uint64_t(0), 5}, &total) == IRS_HIP_EINVAL);           // (and decreasing wins)
  REQUIRE(offsets_rc({0, uint64_t(1) << 32, (uint64_t(1) << 32) + 1}, &total) == IRS_HIP_EUNSUPPORTED);

  // doc lists: two segments of 100 and 50 docs, two queries each
  const std::vector<uint32_t> sd{100, 50};
  REQUIRE(lists_rc({1, 2, 100, 7, 1, 50, 50}, {0, 3, 4, 6, 7}, 2, sd) == IRS_HIP_OK);
  REQUIRE(lists_rc({}, {0, 0, 0, 0, 0}, 2, sd) == IRS_HIP_OK);
  REQUIRE(lists_rc({0, 2, 100, 7, 1, 50, 50}, {0, 3, 4, 6, 7}, 2, sd) == IRS_HIP_EINVAL);    // a doc of 0
  REQUIRE(lists_rc({1, 2, 101, 7, 1, 50, 50}, {0, 3, 4, 6, 7}, 2, sd) == IRS_HIP_EINVAL);    // above num_docs
  REQUIRE(lists_rc({1, 2, 100, 7, 1, 51, 50}, {0, 3, 4, 6, 7}, 2, sd) == IRS_HIP_EINVAL);    // ... of ITS segment
  REQUIRE(lists_rc({1, 2, 100, 7, 1, 50, 51}, {0, 3, 4, 6, 7}, 2, sd) == IRS_HIP_EINVAL);
  REQUIRE(lists_rc({1, 2, 2, 7, 1, 50, 50}, {0, 3, 4, 6, 7}, 2, sd) == IRS_HIP_EINVAL);      // equal docs
  REQUIRE(lists_rc({1, 3, 2, 7, 1, 50, 50}, {0, 3, 4, 6, 7}, 2, sd) == IRS_HIP_EINVAL);      // descending
  REQUIRE(lists_rc({1, 2, 100, 7, 50, 1, 50}, {0, 3, 4, 6, 7}, 2, sd) == IRS_HIP_EINVAL);
  REQUIRE(lists_rc({5, 4}, {0, 1, 2, 2, 2}, 2, sd) == IRS_HIP_OK);      // ascending is per list, not across borders
  REQUIRE(lists_rc({0xFFFFFFFFu}, {0, 1, 1, 1, 1}, 2, sd) == IRS_HIP_EINVAL);
  {
    const std::vector<uint64_t> o{0, 1};
    const auto op = exact(o);
    const auto sp = exact(sd);
    REQUIRE(score_docs_lists(nullptr, op.get(), 1, 1, sp.get()) == IRS_HIP_EINVAL);
  }

  // chunks: 0 / 1 / 128 / 129 docs, unit borders
  REQUIRE(cut({0}).empty() && cut({0, 0, 0}).empty());
  {
    const auto c = cut({0, 1});
    REQUIRE(c.size() == 1 && c[0].unit == 0 && c[0].first == 0 && c[0].n == 1);
  }
  {
    const auto c = cut({0, 128});
    REQUIRE(c.size() == 1 && c[0].n == 128);
  }
  {
    const auto c = cut({0, 129});
    REQUIRE(c.size() == 2 && c[0].n == 128 && c[1].unit == 0 && c[1].first == 128 && c[1].n == 1);
  }
  {
    // 127 | empty | 130 | 1 | 256: a chunk never crosses a unit border
    const auto c = cut({0, 127, 127, 257, 258, 514});
    REQUIRE(c.size() == 6);
    const ScoreDocsChunk want[6] = {{0, 0, 127, 0}, {2, 127, 128, 0}, {2, 255, 2, 0}, {3, 257, 1, 0},
                                    {4, 258, 128, 0}, {4, 386, 128, 0}};
    for (int i = 0; i < 6; ++i)
      REQUIRE(c[i].unit == want[i].unit && c[i].first == want[i].first && c[i].n == want[i].n && c[i].pad == 0);
  }

  // the device form's slots: every chunk of the cut sits in its own slot below the grid, in order,
  // and "the last unit whose first slot is <= w" names its unit
  uint64_t seed = 12345;
  auto rnd = [&](uint64_t m) {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    return (seed >> 33) % m;
  };
  for (int round = 0; round < 2000; ++round) {
    const uint32_t units = 1 + uint32_t(rnd(9));
    std::vector<uint64_t> offs{0};
    for (uint32_t u = 0; u < units; ++u) {
      const uint64_t kind = rnd(6);
      const uint64_t len = kind == 0 ? 0 : kind == 1 ? 128 * rnd(4) : kind == 2 ? 1 + 128 * rnd(3) : rnd(600);
      offs.push_back(offs.back() + len);
    }
    const auto c = cut(offs);
    const uint64_t grid = score_docs_grid(offs.back(), units);
    uint64_t prev = 0;
    bool first = true;
    for (const ScoreDocsChunk& ch : c) {
      const uint64_t slot = score_docs_slot(offs[ch.unit], ch.unit) + (ch.first - offs[ch.unit]) / kScoreDocsChunk;
      REQUIRE(slot < grid && (first || slot > prev));
      uint32_t lo = 0, hi = units;   // the kernel's search
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (score_docs_slot(offs[mid], mid) <= slot) lo = mid; else hi = mid;
      }
      REQUIRE(lo == ch.unit);
      REQUIRE(offs[lo] + (slot - score_docs_slot(offs[lo], lo)) * kScoreDocsChunk == ch.first);
      prev = slot;
      first = false;
    }
    // and a slot no chunk takes resolves to a range behind its unit's end
    std::vector<uint8_t> taken(grid, 0);
    for (const ScoreDocsChunk& ch : c)
      taken[score_docs_slot(offs[ch.unit], ch.unit) + (ch.first - offs[ch.unit]) / kScoreDocsChunk] = 1;
    for (uint64_t w = 0; w < grid; ++w) {
      if (taken[w]) continue;
      uint32_t lo = 0, hi = units;
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (score_docs_slot(offs[mid], mid) <= w) lo = mid; else hi = mid;
      }
      REQUIRE(offs[lo] + (w - score_docs_slot(offs[lo], lo)) * kScoreDocsChunk >= offs[lo + 1]);
    }
  }
  std::printf("score_docs_shape_check OK\n");
  return 0;
}
