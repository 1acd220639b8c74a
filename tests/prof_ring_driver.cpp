// CPU driver of tests/test_prof_ring.py: the bookkeeping of the profile-table ring (xlb_amd/csrc/prof_ring.hpp) for the commands
// read from stdin, one answer line each.
//   slots BYTES       -> slot count of a ring of images of BYTES bytes
//   ring N            -> a fresh ring of N slots ("ok")
//   stage T_FIRST N   -> the copy runs "first,len first,len ..." of staging the timesteps T_FIRST .. T_FIRST + N - 1, each marked
//                        resident (what xlbhip_stepper_stage_bc_profiles does once a run's copy is enqueued)
//   find T            -> the slot that holds timestep T, or "absent"
//   resident          -> "slot:timestep" of every resident slot, in slot order
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "prof_ring.hpp"

int main() {
  xlb::ProfRing ring;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "slots") {
      unsigned long long bytes = 0;
      in >> bytes;
      std::printf("%d\n", xlb::prof_ring_slot_count((size_t)bytes));
    } else if (what == "ring") {
      int n = 0;
      in >> n;
      ring.reset(n);
      std::printf("ok\n");
    } else if (what == "stage") {
      long long t = 0;
      int n = 0;
      in >> t >> n;
      const char* sep = "";
      for (const xlb::ProfRing::Run run : ring.take(n)) {
        std::printf("%s%d,%d", sep, run.first, run.len);
        sep = " ";
        ring.mark_resident(run, t);
        t += run.len;
      }
      std::printf("\n");
    } else if (what == "find") {
      long long t = 0;
      in >> t;
      const int k = ring.find(t);
      if (k < 0)
        std::printf("absent\n");
      else
        std::printf("%d\n", k);
    } else if (what == "resident") {
      const char* sep = "";
      for (int k = 0; k < ring.slots(); ++k)
        if (ring.used[(size_t)k]) {
          std::printf("%s%d:%lld", sep, k, (long long)ring.t[(size_t)k]);
          sep = " ";
        }
      std::printf("\n");
    }
  }
  return 0;
}
