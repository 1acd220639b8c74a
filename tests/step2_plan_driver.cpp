// CPU driver of tests/test_step2_plan.py: the two-step launch plan (xlb_amd/csrc/step2_plan.hpp) for the cases read from stdin.
//   case nx ny nz halo has_bc n_bc kinds_packed needs_missing lattice collision fuse2 cus
//       -> eligible fuse tile_ty tile_tz segments  (fp32 store and compute, default options otherwise)
//   order tys tzs -> the block -> tile table
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "step2_plan.hpp"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "case") {
      xlb::Step2Case c{};
      int fuse2 = 0;
      long cus = 0;
      in >> c.nx >> c.ny >> c.nz >> c.halo >> c.has_bc >> c.n_bc >> c.kinds_packed >> c.needs_missing >> c.lattice >> c.collision >> fuse2 >> cus;
      c.compute_dtype = c.store_dtype = XLBHIP_F32;
      c.fast_math = 1;
      const xlb::Step2Tile t = xlb::step2_tile(c.lattice, c.collision, c.has_bc != 0);
      std::printf("%d %d %d %d %d\n", (int)xlb::step2_eligible(c), (int)xlb::step2_fuse(c, fuse2, cus, 0, true), t.ty, t.tz,
                  xlb::step2_segments(c, c.nx, cus, 0, true));
    } else if (what == "order") {
      int tys = 0, tzs = 0;
      in >> tys >> tzs;
      const std::vector<uint32_t> o = xlb::step2_tile_order(tys, tzs);
      for (size_t i = 0; i < o.size(); ++i) std::printf(i ? " %u" : "%u", o[i]);
      std::printf("\n");
    }
  }
  return 0;
}
