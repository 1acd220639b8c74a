// Launcher of the two-steps-per-pass kernel, shared by its per-lattice translation units (step2_*.hip); what it shares with the
// single-step launcher comes from step_launch.hpp's step_args.
#pragma once
#include "step2_kernel.hpp"
#include "step_launch.hpp"

namespace xlb {

// effective launch geometry (shared by the kernel launch and the clean-flag pass: both must map blocks alike)
inline int step2_eff_segments(const Step2Launch& p) { return (p.x_segments > 1 && p.x_count >= 8 * p.x_segments) ? p.x_segments : 1; }
// thin end segments need >= 3 segments and inner segments of at least 8 planes
inline int step2_eff_cap(const Step2Launch& p) {
  const int n = step2_eff_segments(p);
  return (p.x_cap > 0 && n >= 3 && p.x_count - 2 * p.x_cap >= 8 * (n - 2)) ? p.x_cap : 0;
}
inline int step2_eff_swizzle(const Step2Launch& p, unsigned tiles) { return (p.xcd_swizzle && tiles % 8u == 0u) ? 1 : 0; }

template <class L, int HASBC, int TY, int TZ, bool SLAB, bool FAST, class T = float, int COLL = XLBHIP_BGK, int STRIPS = 0>
static int launch2f(const Step2Launch& p);

// fast_bgk = 1 (opt-in): the tolerance-graded fast BGK body (cell.hpp: bgk_fast).  Measured: 20 % fewer VALU instructions buy
// 2-4 % (profiles/r02/step2_sweeps.txt) — the kernel is bound by its real memory traffic, not by VALU issue — so the
// bit-exact body stays the default.
template <class L, int HASBC, int TY, int TZ, bool SLAB>
static int launch2(const Step2Launch& p) {
  return p.fast_bgk ? launch2f<L, HASBC, TY, TZ, SLAB, true>(p) : launch2f<L, HASBC, TY, TZ, SLAB, false>(p);
}

// T / COLL: compute type and collision (cell.hpp collide<>) of the instantiation; the store type is always fp32
template <class L, int HASBC, int TY, int TZ, bool SLAB, bool FAST, class T, int COLL, int STRIPS>
static int launch2f(const Step2Launch& p) {
  static_assert(HASBC == 0 || (sizeof(T) == 4 && COLL == XLBHIP_BGK), "boundary-condition tables of the two-step kernel are fp32 / BGK");
  StepArgs<T, float> a = step_args<T, float>(p, 1);
  // SLAB: pointers advanced to interior plane 0 (the kernel addresses the ghost planes with negative indices)
  const size_t ghost = (size_t)p.halo * p.ny * p.nz;
  a.src += ghost;
  a.dst += ghost;
  a.meta = p.meta ? p.meta + ghost : nullptr;
  a.tile_order = p.tile_order;
  a.clean = (HASBC != 0) ? p.clean : nullptr;
  // (the strip buffer mirrors the field at 1 / 32: its interior plane 0 sits ghost / 32 elements in)
  a.strips_src = (STRIPS & 1) ? static_cast<const float*>(p.strips_src) + (ghost >> 5) : nullptr;
  a.strips_dst = (STRIPS & 2) ? static_cast<float*>(p.strips_dst) + (ghost >> 5) : nullptr;
  if constexpr (STRIPS != 0) {
    XLB_REQUIRE(((STRIPS & 1) == 0 || p.strips_src) && ((STRIPS & 2) == 0 || p.strips_dst), "two-step kernel: strip buffers missing");
    XLB_REQUIRE(p.plane_stride % 32 == 0 && ((size_t)p.ny * p.nz) % 32 == 0, "two-step kernel: strip buffers need 32-element aligned planes");
  }
  a.x_segments = step2_eff_segments(p);
  a.x_cap = step2_eff_cap(p);
  a.tile_oy = p.tile_oy;
  a.tile_oz = p.tile_oz;
  a.prof_keys = nullptr;  // (profile BCs are Zou-He / Regularized: single-step kernel; no force either: extra.force stays zero)
  a.prof_vals = nullptr;
  a.n_prof = 0;
  a.dist_keys = nullptr;
  a.dist_vals = nullptr;
  a.n_dist = 0;
  const unsigned tiles = (unsigned)(p.ny / TY) * (unsigned)(p.nz / TZ);
  a.xcd_swizzle = step2_eff_swizzle(p, tiles);
  hipLaunchKernelGGL((k_step2<L, T, float, COLL, HASBC, TY, TZ, SLAB, FAST, STRIPS>), dim3(tiles * (unsigned)a.x_segments), dim3(S2Geom<L, HASBC, TY, TZ>::THREADS), 0, p.stream, a);
  XLB_HIP(hipGetLastError());
  return 0;
}

}  // namespace xlb
