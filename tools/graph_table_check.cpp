// graph_table_check.cpp — a stand-alone program over csrc/graph_table.h, the policy of a P3HIP_FLAG_LAUNCH_GRAPH_ANY
// engine's table of graphs: it feeds 10,000 random keys through gt::Table at each of the capacities
// 1, 2 and 64 and holds every step (action, evicted entry, slot discipline) and the counters against a naive model that
// keeps plain vectors and scans them.  Host code only; tests/test_graph_any_cpu.py builds it with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       tools/graph_table_check.cpp -o graph_table_check
// and runs it.  Prints one line per capacity; exit status 0: every step agreed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../p3achygo_amd/csrc/graph_table.h"

namespace {

// The policy once more, the slow way: vectors in order of age, linear scans.
struct Naive {
  struct Held { gt::Key key; uint64_t used; long tag; };
  struct Seen { gt::Key key; int count; };
  int capacity, min_seen;
  uint64_t clock = 0, captures = 0, replays = 0, launches = 0, evictions = 0;
  std::vector<Held> held;
  std::vector<Seen> seen;   // sighting longest ago first

  Naive(int c, int m) : capacity(c), min_seen(m) {}

  // action, and the tag of the entry given up (-1: none)
  void see(const gt::Key& k, long tag, int* action, long* evicted) {
    ++clock;
    *evicted = -1;
    for (Held& h : held)
      if (h.key == k) {
        h.used = clock;
        ++replays;
        *action = gt::kReplay;
        return;
      }
    int count = 1;
    size_t at = seen.size();
    for (size_t i = 0; i < seen.size(); ++i)
      if (seen[i].key == k) at = i;
    if (at < seen.size()) {
      count = seen[at].count + 1;
      seen.erase(seen.begin() + (long)at);
    } else if (seen.size() >= 4 * (size_t)capacity) {
      seen.erase(seen.begin());
    }
    if (count < min_seen) {
      seen.push_back(Seen{k, count});
      ++launches;
      *action = gt::kLaunch;
      return;
    }
    if ((int)held.size() >= capacity) {
      size_t lru = 0;
      for (size_t i = 1; i < held.size(); ++i)
        if (held[i].used < held[lru].used) lru = i;
      *evicted = held[lru].tag;
      held.erase(held.begin() + (long)lru);
      ++evictions;
    }
    held.push_back(Held{k, clock, tag});
    ++captures;
    *action = gt::kCapture;
  }
};

uint64_t next(uint64_t& s) {   // splitmix64
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int fail(int capacity, long step, const char* what) {
  fprintf(stderr, "capacity %d, step %ld: %s\n", capacity, step, what);
  return 1;
}

int check(int capacity, int min_seen, long steps, uint64_t seed) {
  gt::Table table(capacity, min_seen);
  Naive naive(capacity, min_seen);
  static const char bufs[3] = {0, 0, 0};
  // what each slot holds by the steps' own account: the tag of its capture, -1 empty
  std::vector<long> slot_tag((size_t)capacity, -1);
  uint64_t s = seed;
  for (long i = 0; i < steps; ++i) {
    // keys that come back often enough to be captured, replayed and evicted at every capacity: a few hot sizes, a
    // long tail, two feature buffers, two result targets, and now and then more rows than slots
    const uint64_t r = next(s);
    gt::Key k;
    k.npos = (r & 3) ? 1 + (int)((r >> 8) % 12) : 1 + (int)((r >> 8) % 700);
    k.total = ((r >> 20) & 7) == 0 ? k.npos + 7 : k.npos;
    k.feats = &bufs[(r >> 24) & 1];
    k.res = ((r >> 25) & 3) == 0 ? nullptr : &bufs[2];
    int want_action;
    long want_evicted;
    naive.see(k, i, &want_action, &want_evicted);
    const gt::Step got = table.see(k, i);
    if ((int)got.action != want_action) return fail(capacity, i, "the action differs from the model's");
    if (got.evicted_tag != want_evicted) return fail(capacity, i, "the evicted entry differs from the model's");
    if (got.action == gt::kLaunch) {
      if (got.slot != -1) return fail(capacity, i, "a launch names a slot");
    } else {
      if (got.slot < 0 || got.slot >= capacity || !table.live(got.slot)) return fail(capacity, i, "bad slot");
      if (got.action == gt::kCapture) {
        // the slot is empty, or holds exactly the entry that was given up
        if (slot_tag[(size_t)got.slot] != got.evicted_tag) return fail(capacity, i, "a capture lands on a slot in use");
        slot_tag[(size_t)got.slot] = i;
      } else if (slot_tag[(size_t)got.slot] < 0) {
        return fail(capacity, i, "a replay of an empty slot");
      }
    }
    if (table.held() != (int)naive.held.size() || table.held() > capacity) return fail(capacity, i, "graphs held");
    // now and then everything is dropped, as p3hip_set_symmetries and a failed capture do
    if ((r >> 40) % 2500 == 0) {
      table.clear();
      naive.held.clear();
      naive.seen.clear();
      for (long& t : slot_tag) t = -1;
      if (table.held() != 0) return fail(capacity, i, "clear left an entry");
    }
  }
  if (table.captures() != naive.captures || table.replays() != naive.replays || table.launches() != naive.launches ||
      table.evictions() != naive.evictions)
    return fail(capacity, steps, "the counters differ from the model's");
  if (table.captures() + table.replays() + table.launches() != (uint64_t)steps) return fail(capacity, steps, "the counters do not add up");
  printf("capacity %d: %ld steps, captures %llu replays %llu launches %llu evictions %llu held %d\n", capacity, steps,
         (unsigned long long)table.captures(), (unsigned long long)table.replays(), (unsigned long long)table.launches(),
         (unsigned long long)table.evictions(), table.held());
  return 0;
}

}  // namespace

int main() {
  int rc = 0;
  for (int capacity : {1, 2, 64}) rc |= check(capacity, gt::kMinSeen, 10000, 0x5EEDull + (uint64_t)capacity);
  rc |= check(3, 1, 2000, 7);   // min_seen 1 and 3: the policy's other knob
  rc |= check(3, 3, 2000, 8);
  // P3HIP_GRAPH_CACHE
  const struct { const char* text; int want; } caps[] = {{nullptr, 64}, {"1", 1}, {"64", 64}, {"1024", 1024}, {"0", 0}, {"1025", 0},
                                                         {"x", 0}, {"", 0}, {"-1", 0}, {"8 ", 0}, {"99999999999999999999", 0}};
  for (const auto& c : caps)
    if (gt::capacity_from(c.text) != c.want) {
      fprintf(stderr, "capacity_from(%s) is %d, not %d\n", c.text ? c.text : "unset", gt::capacity_from(c.text), c.want);
      rc = 1;
    }
  if (rc == 0) printf("ok\n");
  return rc;
}
