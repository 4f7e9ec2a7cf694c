// pool.h — host side: pooled device / page-locked memory, the staging of a batch's uploads, the
// copy streams, host-side stage times.  Included by irs_hip.hip (one translation unit).
#pragma once

// (a named namespace: the segment and batch records, at global scope, hold these buffers)
namespace irs_hip {

// Freed device / page-locked memory is kept per device and handed out again (size classes of
// 1/8 of a power of two): hipMalloc, hipFree and hipHostMalloc cost 0.1 - 1 ms apiece and hipFree
// synchronises the device — a batch that is created, run once and destroyed (the normal life of
// a batch) would spend more time in the allocator than in its kernels.  Whoever returns a block
// has made sure no queued work still touches it (irs_hip_batch_destroy waits for the batch's own
// events).  irs_hip_device_trim() gives everything back to the runtime.
namespace pool {
constexpr int kMaxDevices = 16;
struct Bin {
  std::mutex m;
  std::multimap<size_t, void*> blocks;   // capacity -> block
  size_t cached = 0;
};
inline Bin& bin(int device, bool pinned) {
  static Bin bins[2][kMaxDevices];
  return bins[pinned ? 1 : 0][device >= 0 && device < kMaxDevices ? device : 0];
}
inline size_t size_class(size_t n) {
  size_t step = 4096;
  while (step * 16 <= n) step <<= 1;   // step = 2^floor(log2 n) / 8 for n >= 64 KB
  return (std::max<size_t>(n, 1) + step - 1) / step * step;
}
// What stays with the library per device: device memory up to rt::pool_cap_bytes() — the buffers
// of the batches a pipelined serving loop has alive (a config-5 step holds two batches of ~6 GB, and
// three steps overlap; a cap of 16 GB was tried: blocks then go back to the runtime, hipFree
// synchronises the device and the steps stall — 45 -> 150 ms) —, page-locked HOST memory up to 4 GB:
// a batch pins a few MB of tables and its results (8 MB for 1000 x top-1000), and pinned pages are
// taken from every process on the node (8 ranks x the old 64 GB default was the whole host).
// IRS_HIP_POOL_MB / IRS_HIP_PINNED_POOL_MB override.
inline size_t cap_bytes(bool pinned) {
  if (const char* e = std::getenv(pinned ? "IRS_HIP_PINNED_POOL_MB" : "IRS_HIP_POOL_MB"))
    return size_t(std::atoll(e)) << 20;
  return pinned ? std::min<size_t>(rt::pool_cap_bytes(), size_t(4) << 30) : rt::pool_cap_bytes();
}
// A closing segment's memory goes back to the runtime, not into the pool: it is hundreds of MB in
// sizes no batch asks for (irs_hip_segment_close sets this around its destructor).
inline thread_local bool tl_free_now = false;
inline void release_all(int device, bool pinned) {
  Bin& b = bin(device, pinned);
  std::lock_guard<std::mutex> lock(b.m);
  for (auto& kv : b.blocks) pinned ? rt::hfree(kv.second) : rt::dfree(kv.second);
  b.blocks.clear();
  b.cached = 0;
}
// `*cap` = the block's capacity (what give() wants back)
inline void* take(int device, bool pinned, size_t bytes, size_t* cap) {
  const size_t want = size_class(bytes);
  Bin& b = bin(device, pinned);
  {
    std::lock_guard<std::mutex> lock(b.m);
    auto it = b.blocks.lower_bound(want);
    if (it != b.blocks.end() && it->first <= want + want / 4) {
      void* p = it->second;
      *cap = it->first;
      b.cached -= it->first;
      b.blocks.erase(it);
      rt::poison(p, *cap);
      return p;
    }
  }
  void* p = pinned ? rt::hmalloc(want) : rt::dmalloc(want);
  if (!p) {   // out of memory with blocks of other sizes lying around: give them back first
    release_all(device, pinned);
    p = pinned ? rt::hmalloc(want) : rt::dmalloc(want);
  }
  *cap = p ? want : 0;
  return p;
}
inline void give(int device, bool pinned, void* p, size_t cap) {
  if (!p) return;
  Bin& b = bin(device, pinned);
  if (!tl_free_now) {
    std::lock_guard<std::mutex> lock(b.m);
    if (b.cached + cap <= cap_bytes(pinned)) {
      b.blocks.emplace(cap, p);
      b.cached += cap;
      return;
    }
  }
  pinned ? rt::hfree(p) : rt::dfree(p);
}
}  // namespace pool

template<bool PINNED>
struct PoolBuf {  // owning allocation out of the pool of the device that was current at alloc()
  void* p = nullptr;
  size_t n = 0;     // bytes asked for
  size_t cap = 0;   // the block's capacity
  int device = 0;
  bool owned = true;   // false: a view into another PoolBuf (view())
  PoolBuf() = default;
  PoolBuf(const PoolBuf&) = delete;
  PoolBuf& operator=(const PoolBuf&) = delete;
  PoolBuf(PoolBuf&& o) noexcept : p(o.p), n(o.n), cap(o.cap), device(o.device), owned(o.owned) {
    o.p = nullptr;
    o.n = o.cap = 0;
  }
  ~PoolBuf() { release(); }
  bool alloc(size_t bytes) {
    if (p && owned && bytes <= cap && pool::size_class(bytes) == cap) {   // the same block would come back
      n = bytes;
      return true;
    }
    release();
    device = rt::current_device();
    p = pool::take(device, PINNED, bytes, &cap);
    n = p ? bytes : 0;
    return p != nullptr;
  }
  void release() {
    if (owned) pool::give(device, PINNED, p, cap);
    p = nullptr;
    n = cap = 0;
    owned = true;
  }
  // `bytes` at `ptr` inside a block somebody else owns (and outlives this view)
  void view(void* ptr, size_t bytes) {
    release();
    p = ptr;
    n = bytes;
    owned = false;
  }
  template<typename T>
  T* as() const { return static_cast<T*>(p); }
};
using DevBuf = PoolBuf<false>;
using PinBuf = PoolBuf<true>;

// A HIP event, created on first use and destroyed with its owner (sync / wait fail on one that
// was never created)
struct Event {
  rt::event_t e{};
  bool made = false;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { if (made) rt::event_destroy(e); }
  bool create() { return made || (made = rt::event_create(&e)); }
  bool record(rt::stream_t st) { return create() && rt::event_record(e, st); }
  bool sync() const { return made && rt::event_sync(e); }
  bool wait(rt::stream_t st) const { return made && rt::stream_wait(st, e); }   // st waits for it
};

// An event together with "something recorded on it may still be in flight".  Whoever is about to
// touch what that work reads or writes calls wait() or sync() and names no guard of its own: on a
// Pending that nothing was ever recorded on — or whose work is known to be through — both do
// nothing and succeed.
struct Pending {
  bool mark(rt::stream_t st) {   // recorded on `st`: pending from here on
    if (!e.record(st)) return false;
    on = true;
    return true;
  }
  // `st` gets behind it.  It stays pending: a stream wait proves nothing to the host or to another stream.
  bool wait(rt::stream_t st) const { return !on || e.wait(st); }
  // the host gets behind it: through, no longer pending
  bool sync() {
    if (!sync_keep()) return false;
    on = false;
    return true;
  }
  // ... and it stays pending: for a reader that cannot speak for the later ones (a const owner), or
  // where the mark also says that what the work left is there to be read
  bool sync_keep() const { return !on || e.sync(); }
  bool pending() const { return on; }
  // a stream is behind it AND everything that touches the same memory later is ordered behind that
  // stream's work: the caller says why
  void settle() { on = false; }
 private:
  Event e;
  bool on = false;
};

// Host -> device uploads of a batch: the bytes are built in (or copied into) page-locked memory
// and go out with asynchronous copies on the stream of the batch's next run — no copy from
// pageable memory (the runtime stages those synchronously), no stream synchronisation, so a
// caller's host thread prepares batch i + 1 while the device still executes batch i.
struct Stager {
  struct Piece { void* dst; const void* src; size_t n; };
  std::vector<PinBuf> chunks;
  size_t used = 0;   // of chunks.back()
  std::vector<Piece> pending;
  // n bytes of page-locked memory that will be copied to `dst`: the caller fills them before
  // the next flush()
  void* put(void* dst, size_t n) {
    if (!n) return nullptr;
    const size_t need = (n + 63) & ~size_t(63);
    if (chunks.empty() || used + need > chunks.back().n) {
      PinBuf c;
      if (!c.alloc(std::max<size_t>(need, size_t(1) << 20))) return nullptr;
      chunks.push_back(std::move(c));
      used = 0;
    }
    void* at = chunks.back().as<uint8_t>() + used;
    used += need;
    pending.push_back(Piece{dst, at, n});
    return at;
  }
  bool copy(void* dst, const void* src, size_t n) {
    if (!n) return true;
    void* at = put(dst, n);
    if (!at) return false;
    std::memcpy(at, src, n);
    return true;
  }
  bool flush(rt::stream_t st) {
    bool ok = true;
    for (const Piece& p : pending) ok = ok && rt::h2d(p.dst, p.src, p.n, st);
    pending.clear();
    return ok;
  }
};

// One copy stream per device for the tables of a batch's FIRST run: queued on the caller's stream
// they would start only when the previous batch's kernels are through (0.2 ms of idle compute per
// step for the headline batch's 5 MB); on their own stream they travel while those kernels run,
// and the run waits for them by an event.
// (`made`: whether the stream exists)
inline rt::stream_t copy_stream(int device, int which, bool* made = nullptr) {
  struct Made { rt::stream_t s; bool ok; };
  static std::mutex m;
  static std::map<int, Made> streams;
  std::lock_guard<std::mutex> lock(m);
  const int key = device * 4 + which;
  auto it = streams.find(key);
  if (it == streams.end()) {
    Made s{nullptr, false};
    s.ok = rt::stream_create(&s.s);
    if (!s.ok) s.s = nullptr;   // (null: the caller keeps its own stream)
    it = streams.emplace(key, s).first;
  }
  if (made) *made = it->second.ok;
  return it->second.s;
}
inline rt::stream_t upload_stream(int device) { return copy_stream(device, 0); }
// ... and one for results on their way to page-locked host memory (irs_hip_batch_results_to_host):
// the copy of batch i travels while the kernels of batch i + 1 run
inline rt::stream_t download_stream(int device) { return copy_stream(device, 1); }

// One tail stream per device: behind a batch whose whole score stage is the one paired launch
// (k_join_score<kJKHalf>, which holds every wave slot of the chip), k_join_rescore and k_select
// leave more than half of the slots empty — on a stream of their own they share the chip with
// the k_join_pilot of the NEXT batch the caller has queued (tail_ok / queue_tail, irs_hip.hip).
// `done`: re-recorded behind every tail; the score stage of every later run waits for the record
// made last (a started k_join_score workgroup holds the LDS the previous k_select asks for).
// The worker thread and callers with asynchronous runs off both come here: `m` is held across
// the queuing of a whole tail and around every wait.
struct Tail {
  std::mutex m;
  Pending done;
};
inline Tail& tail_of(int device) {
  static Tail* tails = new Tail[pool::kMaxDevices];   // (never destroyed: the runtime may go first)
  return tails[device >= 0 && device < pool::kMaxDevices ? device : 0];
}
inline rt::stream_t tail_stream(int device, bool* made) { return copy_stream(device, 2, made); }
// `st` gets behind the tail queued last on the device
inline bool wait_for_tail(int device, rt::stream_t st) {
  Tail& t = tail_of(device);
  std::lock_guard<std::mutex> lock(t.m);
  return t.done.wait(st);
}

// IRS_HIP_TRACE=1: host-side stage times on stderr (what a batch costs before its first kernel)
struct HostTrace {
  const char* what;
  std::chrono::steady_clock::time_point t0;
  explicit HostTrace(const char* w) : what(w), t0(std::chrono::steady_clock::now()) {}
  ~HostTrace() {
    static const bool on = std::getenv("IRS_HIP_TRACE") != nullptr;
    if (on)
      std::fprintf(stderr, "[irs_hip] %s: %.1f us\n", what,
                   std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
  }
};

}  // namespace irs_hip
