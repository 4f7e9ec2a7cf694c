// tests/cpp/test_pending.cpp — Pending (iresearch_amd/csrc/pool.h) against the emulator's rt::
// (tests/sim/gpu_rt.h): what it asks of the runtime, read from the emulator's sync log
// (IRS_SIM_SYNC_LOG), and what it says of itself.  Stand-alone (no library, a main of its own):
// tests/test_run_sync.py builds and runs it; it is also what to build with -fsanitize=address,undefined
// when pool.h changes.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "gpu_rt.h"
#include "pool.h"

using irs_hip::Pending;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

static std::vector<std::string> lines(const char* path) {
  std::vector<std::string> out;
  std::ifstream in(path);
  for (std::string l; std::getline(in, l);) out.push_back(l);
  return out;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const char* log = argv[1];
  std::remove(log);
  setenv("IRS_SIM_SYNC_LOG", log, 1);
  rt::stream_t a = nullptr, b = nullptr;
  CHECK(rt::stream_create(&a) && rt::stream_create(&b) && a && b && a != b);
  const std::string sa = " s" + std::to_string(reinterpret_cast<uintptr_t>(a));
  const std::string sb = " s" + std::to_string(reinterpret_cast<uintptr_t>(b));

  {  // never marked: wait, sync and sync_keep succeed and touch nothing
    Pending p;
    CHECK(!p.pending());
    CHECK(p.wait(a) && p.sync_keep() && p.sync());
    p.settle();
    CHECK(!p.pending() && lines(log).empty());
  }
  {  // mark, then wait: still pending; sync_keep: still pending; sync clears it
    Pending p;
    CHECK(p.mark(a) && p.pending());
    CHECK(p.wait(b) && p.pending());
    CHECK(p.sync_keep() && p.pending());
    CHECK(p.sync() && !p.pending());
    CHECK(p.wait(b) && p.sync());   // (through: nothing more is asked)
    const std::vector<std::string> want = {"record e1" + sa, "wait e1" + sb, "sync e1 s-", "sync e1 s-"};
    CHECK(lines(log) == want);
  }
  {  // settle clears it; a second mark makes it pending again, on the same event
    Pending p;
    CHECK(p.mark(a) && p.wait(b));
    p.settle();
    CHECK(!p.pending() && p.wait(a) && p.sync());
    CHECK(p.mark(b) && p.pending() && p.sync() && !p.pending());
    const std::vector<std::string> got = lines(log);
    const std::vector<std::string> want = {"record e2" + sa, "wait e2" + sb, "record e2" + sb, "sync e2 s-"};
    CHECK(got.size() == 8 && std::equal(want.begin(), want.end(), got.begin() + 4));
  }
  {  // a failed record does not make it pending — and leaves what was pending so
    Pending p;
    rt::fail_records() = true;
    CHECK(!p.mark(a) && !p.pending() && p.wait(b) && p.sync());
    rt::fail_records() = false;
    CHECK(p.mark(a) && p.pending());
    rt::fail_records() = true;
    CHECK(!p.mark(b) && p.pending());
    rt::fail_records() = false;
    CHECK(p.sync() && !p.pending());
    const std::vector<std::string> got = lines(log);
    CHECK(got.size() == 10 && got[8] == "record e3" + sa && got[9] == "sync e3 s-");
  }
  if (failures) return 1;
  std::printf("test_pending OK\n");
  return 0;
}
