// stream_cache.h — host side: the decoded posting streams a device keeps across batches.
// k_join's output for a (segment, term) — the 4-byte entries and the tile-boundary table — is a
// pure function of the segment: nothing of the query or the scorer is in it, and a segment never
// changes after irs_hip_segment_open.  So the streams a batch decodes stay on the device, keyed by
// (segment, term), and a later batch that references them queues no k_join for them.
//
// Streams live in SLABS: the streams one batch missed, per segment, packed into one allocation of
// the pool — every stream's entries from a 64-byte line on, kJoinSlack readable entries behind the
// last one (join.h's look-ahead guarantee, once per slab), then the streams' boundary tables.  A
// slab is the unit of pinning, of the fill event and of eviction: a tiny stream costs its entries
// rounded up to 64 bytes, 4 bytes per doc tile of the segment + 4, and a map node on the host.
//
// BOUND IMAGES (join.h k_join_bound) are cached next to them: an image is a function of (segment,
// term, scorer signature), so it has a map of its own with that key, and lives in slabs of the same
// kind — the same pinning, fill event, LRU order and budget; `held` counts both.  An image's entries
// are whole slabs of 64 from a 256-byte-aligned offset, sized by join_image_entries' bound (join.h:
// every (term, tile) piece padded to a slab), and it has two boundary tables (plan_join.h).  The counters
// (hits, misses, evictions) and the size of `map` keep counting exact streams only.
// Included by irs_hip.hip (one translation unit).
#pragma once

namespace irs_hip {
namespace scache {

constexpr uint64_t kSlabEntries = 64ull << 20;   // entries per slab at most (256 MB; a longer stream gets its own)
constexpr uint64_t kAlign = 16;                  // a stream starts on a multiple of 16 entries

struct ImageKey {   // (segment, term, scorer signature: kind and the bits of its two floats)
  uint32_t seg_uid, term;
  int32_t kind;
  uint32_t nc, nl;
  bool operator==(const ImageKey& o) const {
    return seg_uid == o.seg_uid && term == o.term && kind == o.kind && nc == o.nc && nl == o.nl;
  }
};
struct ImageKeyHash {
  size_t operator()(const ImageKey& k) const {
    uint64_t h = (uint64_t(k.seg_uid) << 32) | k.term;
    h = (h ^ (uint64_t(k.nc) << 32 | k.nl)) * 0x9E3779B97F4A7C15ull;
    h = (h ^ uint64_t(uint32_t(k.kind)) ^ (h >> 29)) * 0xBF58476D1CE4E5B9ull;
    return size_t(h ^ (h >> 32));
  }
};
struct Slab {
  DevBuf mem;
  uint64_t bytes = 0;     // mem.cap: what the budget counts
  uint64_t entries = 0;   // entries in front of the slack
  uint32_t seg_uid = 0;
  uint32_t n_streams = 0;
  std::vector<uint32_t> terms;   // the streams the map serves out of this slab
  std::vector<ImageKey> images;   // ... or the bound images the image map serves out of it
  // Filled by ONE batch's k_join, on whatever stream that batch's plan stage was queued on;
  // `filled` is recorded behind that launch.  (cache mutex) `queued` turns true once it is: only
  // then is the slab served to other batches, whose runs make their own stream wait for `filled`.
  Pending filled;
  rt::stream_t fill_stream{};   // where (a run on the same stream is behind the fill anyway)
  bool queued = false;
  std::atomic<bool> settled{false};   // the filling batch has waited for its run: nobody needs `filled`
  uint32_t pins = 0;       // (cache mutex) batches alive that reference it
  uint64_t last_use = 0;   // (cache mutex)
  bool listed = false;     // (cache mutex) in the cache: counted in `held`, its terms in the map
};
using SlabPtr = std::shared_ptr<Slab>;
struct Where {
  Slab* slab;
  uint64_t entries, bounds;   // device addresses
};

struct Cache {
  std::mutex m;   // held for table work only: never across a launch, an allocation or a free
  std::unordered_map<uint64_t, Where> map;   // seg_uid << 32 | term
  std::unordered_map<ImageKey, Where, ImageKeyHash> imap;   // the bound images
  std::vector<SlabPtr> slabs;
  uint64_t held = 0, clock = 0;
  uint64_t hits = 0, misses = 0, evictions = 0;
  std::atomic<int64_t> budget{-1};   // bytes; -1: not asked for yet
};
inline Cache& of(int device) {
  static Cache caches[pool::kMaxDevices];
  return caches[device >= 0 && device < pool::kMaxDevices ? device : 0];
}
inline uint64_t key_of(uint32_t seg_uid, uint32_t term) { return (uint64_t(seg_uid) << 32) | term; }

// IRS_HIP_STREAM_CACHE_MB (process-wide, read once; 0: no cache, every batch decodes its own
// streams), else an eighth of the device's memory; irs_hip_device_set_stream_cache overrides.
inline uint64_t budget_bytes(int device) {
  Cache& c = of(device);
  int64_t v = c.budget.load();
  if (v < 0) {
    static const int64_t env = [] {
      const char* e = std::getenv("IRS_HIP_STREAM_CACHE_MB");
      return e ? int64_t(std::max<long long>(0, std::atoll(e))) << 20 : int64_t(-1);
    }();
#ifdef RT_HAS_DEVICE_TOTAL_MEM
    const int64_t eighth = int64_t(rt::device_total_mem(device) / 8);
#else   // (no device behind the runtime header: half of what the pool may keep)
    const int64_t eighth = int64_t(rt::pool_cap_bytes() / 2);
#endif
    const int64_t def = env >= 0 ? env : eighth;
    c.budget.compare_exchange_strong(v, def);
    v = c.budget.load();
  }
  return uint64_t(v);
}

// (cache mutex held) the slab leaves the cache; `out` keeps it alive until the lock is released —
// a batch that pins it keeps it longer
inline void drop_locked(Cache& c, Slab* s, std::vector<SlabPtr>& out) {
  if (!s->listed) return;
  for (uint32_t term : s->terms) {
    auto it = c.map.find(key_of(s->seg_uid, term));
    if (it != c.map.end() && it->second.slab == s) c.map.erase(it);
  }
  for (const ImageKey& k : s->images) {
    auto it = c.imap.find(k);
    if (it != c.imap.end() && it->second.slab == s) c.imap.erase(it);
  }
  s->listed = false;
  c.held -= s->bytes;
  for (size_t i = 0; i < c.slabs.size(); ++i)
    if (c.slabs[i].get() == s) {
      out.push_back(std::move(c.slabs[i]));
      c.slabs[i] = std::move(c.slabs.back());
      c.slabs.pop_back();
      break;
    }
}
// (cache mutex held) unpinned slabs, least recently used first, until `extra` more bytes fit
inline bool make_room_locked(Cache& c, uint64_t extra, uint64_t budget, std::vector<SlabPtr>& out) {
  while (c.held + extra > budget) {
    Slab* lru = nullptr;
    for (const SlabPtr& s : c.slabs)
      if (!s->pins && (!lru || s->last_use < lru->last_use)) lru = s.get();
    if (!lru) return false;
    c.evictions += lru->terms.size();
    drop_locked(c, lru, out);
  }
  return true;
}
// every unpinned slab (of one segment: `seg_uid` != 0) goes back to the pool; a pinned one of a
// closing segment leaves the cache and goes with its last batch
inline void drop_unpinned(int device, uint32_t seg_uid) {
  Cache& c = of(device);
  std::vector<SlabPtr> out;
  {
    std::lock_guard<std::mutex> lock(c.m);
    for (size_t i = c.slabs.size(); i-- > 0;) {
      Slab* s = c.slabs[i].get();
      if (seg_uid ? s->seg_uid == seg_uid : !s->pins) drop_locked(c, s, out);
    }
  }
}
inline void set_budget(int device, uint64_t bytes) {
  Cache& c = of(device);
  std::vector<SlabPtr> out;
  c.budget.store(int64_t(std::min<uint64_t>(bytes, uint64_t(1) << 62)));
  std::lock_guard<std::mutex> lock(c.m);
  make_room_locked(c, 0, bytes, out);   // (what batches pin stays until they go)
  // (`out` is destroyed after `lock`: declared first)
}

}  // namespace scache
}  // namespace irs_hip
