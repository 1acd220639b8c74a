// CPU driver of tests/test_bc_tables.py: the descriptor parser of the steppers (xlb_amd/csrc/bc_tables.hpp) and the block shape of the
// row kernels (xlb_amd/csrc/launch_shape.hpp) for the commands read from stdin, one answer line each.
//   parse WHO Q ID:KIND[:SLOT=VALUE]...  -> the image of the descriptors (in this order) for a lattice of Q populations, under the
//                                          acceptance rule of WHO (stepper / scalar / adjoint): "ids HEX kinds HEX moving BITS
//                                          needs_missing B extended_bcs B has_outflow B has_edge_kinds B", or "error TEXT"
//                                          (scalar and adjoint: the driver's own text "refused kind K" for a kind they do not take)
//   kind ID                             -> kind[ID] of the last image
//   vals ID                             -> vals[ID][0..26] of the last image
//   shape NZQ NY PLANES THREADS BLOCK_TZ -> "TZ TY GX GY GZ"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "bc_tables.hpp"
#include "launch_shape.hpp"

int main() {
  xlb::BcImage image;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "parse") {
      std::string who;
      int q = 0;
      in >> who >> q;
      std::vector<xlbhip_bc_desc> bcs;
      for (std::string item; in >> item;) {
        xlbhip_bc_desc b = {};
        int slot = 0, used = 0;
        double value = 0.0;
        std::sscanf(item.c_str(), "%d:%d%n", &b.id, &b.kind, &used);
        for (const char* p = item.c_str() + used; std::sscanf(p, ":%d=%lf%n", &slot, &value, &used) == 2; p += used) b.values[slot] = value;
        bcs.push_back(b);
      }
      const auto refusal = [&](int kind) -> const char* {
        if (who == "stepper") return xlb::bc_stepper_refusal(q, kind);
        return (who == "scalar" ? xlb::bc_scalar_accepts(kind) : xlb::bc_adjoint_accepts(kind)) ? nullptr : "refused kind %d";
      };
      const std::string err = xlb::bc_parse(q, (int)bcs.size(), bcs.data(), refusal, image);
      if (!err.empty())
        std::printf("error %s\n", err.c_str());
      else
        std::printf("ids %llx kinds %x moving %x needs_missing %d extended_bcs %d has_outflow %d has_edge_kinds %d\n", image.ids_packed, image.kinds_packed,
                    image.moving_mask, (int)image.needs_missing, (int)image.extended_bcs, (int)image.has_outflow, (int)image.has_edge_kinds);
    } else if (what == "kind" || what == "vals") {
      int id = 0;
      in >> id;
      if (what == "kind") {
        std::printf("%d\n", (int)image.kind[(size_t)id]);
      } else {
        for (int l = 0; l < 27; ++l) std::printf("%s%.17g", l ? " " : "", image.vals[(size_t)id * 27 + l]);
        std::printf("\n");
      }
    } else if (what == "shape") {
      int nzq = 0, ny = 0, planes = 0, threads = 0, block_tz = 0;
      in >> nzq >> ny >> planes >> threads >> block_tz;
      const xlb::RowBlockShape s = xlb::row_block_shape(nzq, ny, planes, threads, block_tz);
      std::printf("%d %d %d %d %d\n", s.tz, s.ty, s.gx, s.gy, s.gz);
    }
  }
  return 0;
}
