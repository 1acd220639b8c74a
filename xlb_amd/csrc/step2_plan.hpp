// Launch plan of the two-steps-per-pass kernel (step2_kernel.hpp): which steppers and fields it takes, when pairs pay, its tile,
// the x segments of a tile column and the order in which the blocks take the tiles.  Host rules on plain integers — no HIP:
// stepper.hip feeds them and keeps the memory, the caches and the launches; tests/test_step2_plan.py compiles them on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "xlbhip.h"

namespace xlb {

constexpr int MAX_FAST_BCS = 8;  // bc ids the kernels look up in their arguments (step_kernel.hpp); more leave the two-step kernel out

// what the rules look at, filled from the stepper and the launch (stepper.hip: plan_case)
struct Step2Case {
  int lattice, collision, compute_dtype, store_dtype;
  int fast_math;  // 1: tolerance-graded collisions allowed (exact_math = 0)
  int nx, ny, nz, halo;
  int has_bc;    // 0: no BCs; 1: basic kinds; 2: + Zou-He / Regularized
  int edge_ext;  // has_bc == 2 but every extended-kind cell sits in plane 0 or nx - 1
  int n_bc;
  unsigned kinds_packed;  // kinds of the first 8 BCs, one per nibble
  int needs_missing;      // halfway walls
};

struct Step2Tile {
  int ty, tz;
};

// The (TY x TZ) tile a block owns: (8 x 64), one block per CU (8 x 32 and 16 x 16 tiles with two blocks per CU were measured slower:
// profiles/r01/sweeps.md; 16 x 32: profiles/r02/sweeps.md).  D3Q27 KBC: (8 x 48) tiles — 8 waves per block, i.e. 2 per SIMD and 256
// VGPRs for the collision (the (8 x 64) tile's 11 waves leave 168: 3.8 KB of scratch in fp64); the grown tile is 500 cells for 384
// outputs, the same ratio as (8 x 64).  D3Q27 BGK with boundary conditions: the BC ring — 63 population-planes — fits the LDS on the
// same (8 x 48) tile: 126 KB.
inline Step2Tile step2_tile(int lattice, int collision, bool has_bc) {
  return {8, lattice == XLBHIP_D3Q27 && (collision == XLBHIP_KBC || has_bc) ? 48 : 64};
}

// Does a two-step kernel exist for this stepper and field layout?  (Otherwise the stepper runs single steps.)
inline bool step2_eligible(const Step2Case& p) {
  const Step2Tile t = step2_tile(p.lattice, p.collision, p.has_bc != 0);
  // do-nothing BCs would need a second redirected-load form (own cell, same population): not built; like the Zou-He
  // family they are fine on the x end planes, which the two-step kernel leaves to the single-step kernel (edge_ext)
  for (int i = 0; i < p.n_bc && i < 8; ++i)
    if (((p.kinds_packed >> (4 * i)) & 0xfu) == XLBHIP_BC_DO_NOTHING && !p.edge_ext) return false;
  if (!(p.store_dtype == XLBHIP_F32 && p.nx >= 4 && p.ny % t.ty == 0 && p.nz % t.tz == 0)) return false;
  if (p.lattice == XLBHIP_D3Q27) {  // without ghost planes only; BGK also with the basic boundary conditions, on (8 x 48) tiles (63 population-planes)
    if (!(p.halo == 0 && t.ty == 8)) return false;
    if (p.collision == XLBHIP_BGK)
      return p.compute_dtype == XLBHIP_F32 && (p.has_bc == 0 ? t.tz == 64 : (p.has_bc == 1 && t.tz == 48 && p.n_bc <= MAX_FAST_BCS));
    if (p.has_bc != 0) return false;
    // KBC: fp32 and fp64 compute, (8 x 48) tiles
    // (the bit-exact fp64 collision needs 940 B of scratch there — 12 ms per step: it stays on the single-step kernel)
    return p.collision == XLBHIP_KBC && (p.compute_dtype == XLBHIP_F32 || (p.compute_dtype == XLBHIP_F64 && p.fast_math)) && t.tz == 48;
  }
  return p.collision == XLBHIP_BGK && p.compute_dtype == XLBHIP_F32 && p.lattice == XLBHIP_D3Q19 && (p.halo == 0 || p.halo == 2) &&
         (p.has_bc <= 1 || (p.edge_ext && p.halo == 0 && p.nx >= 16)) && p.n_bc <= MAX_FAST_BCS;
}

// x segments per tile column of a launch over x_count planes.  One block per CU marches a segment, so the launch runs in
// ceil(tiles * n / CUs) rounds of (planes per segment + 3 warm-up planes): pick the n that minimises that product
// (320^3: 4 -> 8 segments = 3.1 -> 6.25 rounds, -9 %; 256^3: 2 segments = exactly one round).  xseg > 0 (the fuse2_xseg option)
// asks for that many, halved down to segments of >= 8 planes; clean: the fuse2_clean option.
inline int step2_segments(const Step2Case& c, int x_count, long cus, int xseg, bool clean) {
  if (xseg > 0) {
    int n = xseg;
    while (n > 1 && x_count / n < 8) n /= 2;
    return n;
  }
  const Step2Tile t = step2_tile(c.lattice, c.collision, c.has_bc != 0);
  const long tiles = (long)(c.ny / t.ty) * (c.nz / t.tz);
  // with boundary conditions finer items win twice: the expensive hull tiles balance better (halfway walls), and work
  // items free of boundary cells — most segments of an interior tile column — run the BC-free body (fuse2_clean):
  // take the most segments of >= 32 planes (measured at 256^3 ... 512^3: profiles/r01/sweeps.md, profiles/r02/step2_sweeps.txt)
  const bool finest = c.needs_missing || (c.has_bc && clean);
  int best = 1;
  long best_cost = -1;
  for (int n = 1; n <= 8; n *= 2) {
    if (n > 1 && x_count / n < 32) break;
    const long cost = ((tiles * n + cus - 1) / cus) * (x_count / n + 3);
    if (best_cost < 0 || cost < best_cost || finest) {
      best = n;
      best_cost = cost;
    }
  }
  return best;
}

// Whether a stepper runs pairs of steps through the two-step kernel (fuse2 = 1: where eligible and faster; 2: wherever eligible),
// once its Zou-He / Regularized / outflow / do-nothing cells are known to sit in the x end planes.  cus: the CUs to fill.
inline bool step2_fuse(const Step2Case& c, int fuse2, long cus, int xseg, bool clean) {
  if (!step2_eligible(c)) return false;
  if (fuse2 == 1) {
    // D3Q27 KBC pairs on request only (fuse2 = 2): ~1100 (fp32) / 810 (fast fp64) VALU instructions per cell and 8 waves per CU make
    // the two-step form issue-bound — 384^3: 2.41 (FP64FP32) / 2.52 (FP32FP32) ms per step against 2.21 / 2.16 of the HBM-bound
    // single-step kernel (profiles/r02/d3q27_kbc_two_step.txt); with the gamma reduction in fp32 (cell.hpp COLL_G32) still 2.28 against
    // 2.23 (profiles/r03/kbc_gamma32.md)
    if (c.lattice == XLBHIP_D3Q27 && c.collision == XLBHIP_KBC) return false;
    // D3Q27 BGK with boundary conditions (round 3, (8 x 48) tiles, 192 VGPRs): bit-exact, but 2.59-3.16 against 2.15-2.19 ms per step on
    // the 384^3 cavity (0.48-0.59 against 0.70-0.71 of the roofline, profiles/r03/d3q27_walls_two_step.md): on request only
    if (c.lattice == XLBHIP_D3Q27 && c.collision == XLBHIP_BGK && c.has_bc) return false;
    // one block per CU marches an (8 x 64) tile column segment: the work items must fill the chip in whole
    // rounds (128^3 = 32 tiles x 4 segments would leave half of the 256 CUs idle)
    const Step2Tile t = step2_tile(c.lattice, c.collision, c.has_bc != 0);
    const long tys = c.ny / t.ty, tzs = c.nz / t.tz;
    const long items = tys * tzs * step2_segments(c, c.nx, cus, xseg, clean);
    const long rounds = (items + cus - 1) / cus;
    if (items * 100 < rounds * cus * 85) return false;
    // halfway walls make the hull tiles ~1.5x as expensive as fluid tiles; when most tiles are hull tiles two single
    // steps are faster (256^3, 53 % hull tiles: fused 41.7 vs 38.2 GLUPS; thinner domains lose).  With the half-tile shift
    // of the tiling both walls of an axis share one tile row: tys + tzs - 1 hull tiles
    if (c.needs_missing && std::min(tys * tzs, tys + tzs - 1) * 100 > tys * tzs * 60) return false;
  }
  return true;
}

// Block -> tile table of a launch with boundary conditions on a (tys x tzs) tiling shifted by half a tile: hull tiles first (the
// expensive ones when there are walls), then the interior; both lists are dealt so that every XCD (block i runs on XCD i % 8) works
// on a CONTIGUOUS run of tiles — neighbours share their halo rows / lines through that XCD's L2.
inline std::vector<uint32_t> step2_tile_order(int tys, int tzs) {
  // half-tile shift: the walls of the y / z faces sit in the LAST tile row / column (the ones that wrap around)
  std::vector<uint32_t> hull, inner;
  for (int tz = 0; tz < tzs; ++tz) hull.push_back((uint32_t)((tys - 1) * tzs + tz));
  for (int ty = tys - 2; ty >= 0; --ty) hull.push_back((uint32_t)(ty * tzs + tzs - 1));
  for (int ty = 0; ty < tys - 1; ++ty)
    for (int tz = 0; tz < tzs - 1; ++tz) inner.push_back((uint32_t)(ty * tzs + tz));
  std::vector<uint32_t> order;
  order.reserve((size_t)tys * tzs);
  auto deal = [&](const std::vector<uint32_t>& list) {
    // chunk k = list[k * per ...]; the slot being filled decides the XCD (slot % 8) and takes the next tile of that
    // XCD's chunk (of the fullest chunk once its own is used up)
    const size_t n = list.size(), per = (n + 7) / 8;
    size_t cur[8], end[8];
    for (size_t k = 0; k < 8; ++k) {
      cur[k] = std::min(n, k * per);
      end[k] = std::min(n, (k + 1) * per);
    }
    for (size_t done = 0; done < n; ++done) {
      size_t k = order.size() % 8;
      if (cur[k] == end[k])
        for (size_t m = 0; m < 8; ++m)
          if (end[m] - cur[m] > end[k] - cur[k]) k = m;
      order.push_back(list[cur[k]++]);
    }
  };
  deal(hull);
  deal(inner);
  return order;
}

}  // namespace xlb
