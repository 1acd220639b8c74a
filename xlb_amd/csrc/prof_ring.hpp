// Bookkeeping of the ring of per-timestep profile tables (time-dependent wall velocities, stepper.hip): which slot holds which
// timestep and which slots the next images go to.  Host arithmetic only — no HIP type or call, so that tests/test_prof_ring.py
// compiles it for the CPU; the device ring, the pinned rows, the events and the copies are stepper.hip's.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace xlb {

// The ring holds a byte budget's worth of table images, at least 4 and at most 64, an even count (the Python stepper stages
// chunks of half the ring, in pairs of steps).
static const size_t PROF_RING_BYTES = (size_t)64 << 20;
static const int PROF_RING_MIN = 4, PROF_RING_MAX = 64;

inline int prof_ring_slot_count(size_t image_bytes) {
  const size_t k = PROF_RING_BYTES / std::max<size_t>(image_bytes, 1);
  const int n = (int)std::min<size_t>(std::max<size_t>(k, PROF_RING_MIN), PROF_RING_MAX);
  return n & ~1;
}

struct ProfRing {
  struct Run {
    int first, len;  // consecutive slots: one copy
  };
  std::vector<int64_t> t;     // the timestep a slot holds
  std::vector<uint8_t> used;  // slot holds a staged image
  int head = 0;               // the slot the next image goes to

  int slots() const { return (int)t.size(); }
  void reset(int n) {
    t.assign((size_t)n, 0);
    used.assign((size_t)n, 0);
    head = 0;
  }
  // the slot that holds timestep `ts`, or -1
  int find(int64_t ts) const {
    for (int k = 0; k < slots(); ++k)
      if (used[(size_t)k] && t[(size_t)k] == ts) return k;
    return -1;
  }
  // the next n <= slots() slots from the head, as runs split where the ring wraps.  Their images are about to be replaced: they
  // stop being resident here and count again only once mark_resident says their copy is enqueued.
  std::vector<Run> take(int n) {
    std::vector<Run> runs;
    for (int r = 0; r < n; ++r) {
      const int k = head;
      head = (k + 1) % slots();
      used[(size_t)k] = 0;
      if (runs.empty() || k == 0)
        runs.push_back({k, 1});
      else
        ++runs.back().len;
    }
    return runs;
  }
  // slot run.first + i now holds timestep t_first + i; an older image of such a timestep in another slot is superseded
  void mark_resident(Run run, int64_t t_first) {
    for (int i = 0; i < run.len; ++i) {
      const int64_t ts = t_first + i;
      for (int j = 0; j < slots(); ++j)
        if (used[(size_t)j] && t[(size_t)j] == ts) used[(size_t)j] = 0;
      t[(size_t)(run.first + i)] = ts;
      used[(size_t)(run.first + i)] = 1;
    }
  }
};

}  // namespace xlb
