// graph_table.h — which forward passes of a P3HIP_FLAG_LAUNCH_GRAPH_ANY engine are launched kernel by kernel, captured or
// replayed.  Host only, plain C++, no HIP type: the engine keeps the graphs themselves in an array
// by the slot numbers handed out here (forward.cpp run_pass), p3hip_debug_graph_table and tools/graph_table_check.cpp
// drive the policy alone.
//
// A captured graph bakes in every kernel argument and grid of its pass; the key is what those follow from.  Whatever a
// kernel reads from device memory at run time (features, the slot symmetry table, INT8 scales) is not part of it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <iterator>
#include <list>
#include <unordered_map>
#include <vector>

namespace gt {

struct Key {
  int npos = 0;                  // slots of the pass
  int total = 0;                 // forward rows: npos, npos * k (SYMMETRY_AVG), or the staged table's sum (SYMMETRY_SLOT)
  const void* feats = nullptr;   // the feature buffer the pass reads
  const void* res = nullptr;     // the dense result target (null: not written)
  bool operator==(const Key& o) const { return npos == o.npos && total == o.total && feats == o.feats && res == o.res; }
};

struct KeyHash {
  size_t operator()(const Key& k) const {
    uint64_t h = 14695981039346656037ull;
    for (uint64_t v : {(uint64_t)(uint32_t)k.npos, (uint64_t)(uint32_t)k.total, (uint64_t)(uintptr_t)k.feats, (uint64_t)(uintptr_t)k.res})
      h = (h ^ v) * 1099511628211ull;
    return (size_t)(h ^ (h >> 32));
  }
};

enum Action { kLaunch = 0, kCapture = 1, kReplay = 2 };

// What the pass does.  kCapture: the new graph goes into `slot`; with evicted_tag >= 0 that slot still holds the graph of
// the entry captured at the step of that tag, which the caller destroys first.  kReplay: the graph in `slot`.
struct Step {
  Action action = kLaunch;
  int slot = -1;
  long evicted_tag = -1;
};

constexpr int kMinCapacity = 1, kMaxCapacity = 1024, kDefaultCapacity = 64;
constexpr int kMinSeen = 2;   // the first pass of a key goes out kernel by kernel: the launchers set their kernels' LDS
                              // attributes on first use, which a capture must not see
constexpr int kDefaultMaxRows = 0;   // the engine captures partial passes of at most so many forward rows (0: of any size)

class Table {
 public:
  explicit Table(int capacity = kDefaultCapacity, int min_seen = kMinSeen)
      : capacity_(capacity), min_seen_(min_seen < 1 ? 1 : min_seen), entries_((size_t)capacity) {}

  int capacity() const { return capacity_; }
  int held() const { return (int)held_.size(); }
  uint64_t captures() const { return captures_; }
  uint64_t replays() const { return replays_; }
  uint64_t launches() const { return launches_; }
  uint64_t evictions() const { return evictions_; }

  // The next pass has key `k`; `tag` names it (the engine's pass count, the hook's step index) in a later evicted_tag.
  Step see(const Key& k, long tag) {
    ++clock_;
    Step s;
    auto h = held_.find(k);
    if (h != held_.end()) {
      entries_[h->second].used = clock_;
      ++replays_;
      s.action = kReplay;
      s.slot = h->second;
      return s;
    }
    // a sighting of a key not held: counted in a bounded map, the sighting longest ago forgotten first
    int seen = 1;
    auto f = seen_.find(k);
    if (f != seen_.end()) {
      seen = ++f->second->count;
      order_.splice(order_.end(), order_, f->second);
    } else {
      if (seen_.size() >= 4 * (size_t)capacity_) {
        seen_.erase(order_.front().key);
        order_.pop_front();
      }
      order_.push_back(Sighting{k, 1});
      seen_[k] = std::prev(order_.end());
    }
    if (seen < min_seen_) {
      ++launches_;
      return s;
    }
    // captured: the key leaves the sightings (evicted later, it starts again at none); a full table gives up the entry
    // replayed (or, never replayed, captured) longest ago
    seen_.erase(k);
    order_.pop_back();
    int slot = -1;
    if ((int)held_.size() < capacity_) {
      for (int i = 0; i < capacity_; ++i)
        if (!entries_[i].live) { slot = i; break; }
    } else {
      for (int i = 0; i < capacity_; ++i)
        if (slot < 0 || entries_[i].used < entries_[slot].used) slot = i;
      s.evicted_tag = entries_[slot].tag;
      held_.erase(entries_[slot].key);
      ++evictions_;
    }
    entries_[slot] = Entry{k, clock_, tag, true};
    held_[k] = slot;
    ++captures_;
    s.action = kCapture;
    s.slot = slot;
    return s;
  }

  // A pass that bypassed the table (calibration, a stopped engine) went out kernel by kernel
  void count_launch() { ++launches_; }

  // Every entry and every sighting goes; the counters stay.  The caller destroys the graphs of the live slots first.
  void clear() {
    held_.clear();
    seen_.clear();
    order_.clear();
    for (Entry& e : entries_) e.live = false;
  }

  bool live(int slot) const { return slot >= 0 && slot < capacity_ && entries_[slot].live; }

 private:
  struct Entry {
    Key key;
    uint64_t used = 0;   // clock of the capture or the last replay
    long tag = -1;
    bool live = false;
  };
  struct Sighting {
    Key key;
    int count;
  };
  int capacity_, min_seen_;
  uint64_t clock_ = 0, captures_ = 0, replays_ = 0, launches_ = 0, evictions_ = 0;
  std::vector<Entry> entries_;
  std::unordered_map<Key, int, KeyHash> held_;
  std::list<Sighting> order_;   // oldest sighting first
  std::unordered_map<Key, std::list<Sighting>::iterator, KeyHash> seen_;
};

// P3HIP_GRAPH_CACHE: the table's capacity.  Unset: the default; a whole number in 1..1024: that; anything else: 0
inline int capacity_from(const char* text) {
  if (!text) return kDefaultCapacity;
  if (!*text) return 0;
  long v = 0;
  for (const char* p = text; *p; ++p) {
    if (*p < '0' || *p > '9' || v > kMaxCapacity) return 0;
    v = v * 10 + (*p - '0');
  }
  return v >= kMinCapacity && v <= kMaxCapacity ? (int)v : 0;
}

}  // namespace gt
