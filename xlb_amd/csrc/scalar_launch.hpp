// Type-erased launch descriptor of the coupled fluid + scalar step and the per-lattice dispatcher that each scalar_<lattice>.hip
// instantiates (the scheme of step_launch.hpp).
#pragma once
#include "common.hpp"
#include "scalar_step_kernel.hpp"
#include "step_launch.hpp"

namespace xlb {

struct ScalarLaunch {
  StepLaunch f;  // the fluid's part (f.halo == 0, all of x)
  const void* gsrc;
  void* gdst;
  size_t g_plane_stride;
  const uint8_t* sc_rule;
  const void* sc_value;  // compute dtype [256]
  ScalarCoupling cp;
  double omega_s;
};

template <class L, class T, class S, int VEC, int COLL, int HASBC>
int launch_scalar_typed(const ScalarLaunch& q) {
  const StepLaunch& p = q.f;
  ScalarStepArgs<T, S> sa = {};
  StepArgs<T, S>& a = sa.f;
  a.src = static_cast<const S*>(p.src);
  a.dst = static_cast<S*>(p.dst);
  a.bc = p.bc;
  a.miss = p.miss;
  a.bc_kind = p.tab_kind;
  a.bc_values = static_cast<const T*>(p.tab_values);
  a.ids_packed = p.ids_packed;
  a.kinds_packed = p.kinds_packed;
  a.n_bc = p.n_bc;
  a.plane_stride = p.plane_stride;
  a.nx = p.nx;
  a.ny = p.ny;
  a.nz = p.nz;
  a.x_begin = 0;
  a.x_count = p.nx;
  a.nzq = p.nz / VEC;
  a.omega = static_cast<T>(p.omega);
  a.extra.smag_cs = p.smag_cs;
  sa.gsrc = static_cast<const S*>(q.gsrc);
  sa.gdst = static_cast<S*>(q.gdst);
  sa.g_plane_stride = q.g_plane_stride;
  sa.sc_rule = q.sc_rule;
  sa.sc_value = static_cast<const T*>(q.sc_value);
  sa.cp = q.cp;
  sa.omega_s = static_cast<T>(q.omega_s);
  // threads along z: a row in equal chunks of whole waves, as launch_typed does
  const int threads = 256;
  int tz = a.nzq;
  if (tz > threads) {
    const int chunks = (a.nzq + threads - 1) / threads;
    tz = (a.nzq + chunks - 1) / chunks;
    tz = (tz + 63) / 64 * 64;
    if (tz > threads) tz = threads;
  }
  int ty = threads / tz;
  if (ty < 1) ty = 1;
  if (ty > p.ny) ty = p.ny;
  dim3 block(tz, ty, 1);
  dim3 grid((a.nzq + tz - 1) / tz, (p.ny + ty - 1) / ty, p.nx);
  XLB_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "grid too large: ny/ty=%u nx=%u", grid.y, grid.z);
  hipLaunchKernelGGL((k_step_scalar<L, T, S, VEC, COLL, HASBC>), grid, block, 0, p.stream, sa);
  XLB_HIP(hipGetLastError());
  return 0;
}

template <class L, class T, class S, int COLL>
int launch_scalar_policy(const ScalarLaunch& q) {
  const StepLaunch& p = q.f;
  const int v = pick_vec(p.compute_dtype, p.nz, p.vec, COLL & 3);
  if constexpr (sizeof(T) == 4) {
    if (v == 4) return p.has_bc ? launch_scalar_typed<L, T, S, 4, COLL, 2>(q) : launch_scalar_typed<L, T, S, 4, COLL, 0>(q);
  }
  if (v == 2) return p.has_bc ? launch_scalar_typed<L, T, S, 2, COLL, 2>(q) : launch_scalar_typed<L, T, S, 2, COLL, 0>(q);
  return p.has_bc ? launch_scalar_typed<L, T, S, 1, COLL, 2>(q) : launch_scalar_typed<L, T, S, 1, COLL, 0>(q);
}

template <class L, int COLL>
int launch_scalar_coll(const ScalarLaunch& q) {
  const int c = q.f.compute_dtype, s = q.f.store_dtype;
  if (c == XLBHIP_F32 && s == XLBHIP_F32) return launch_scalar_policy<L, float, float, COLL>(q);
  if (c == XLBHIP_F64 && s == XLBHIP_F64) return launch_scalar_policy<L, double, double, COLL>(q);
  if (c == XLBHIP_F64 && s == XLBHIP_F32) return launch_scalar_policy<L, double, float, COLL>(q);
  XLB_FAIL("scalar transport is built for FP32FP32, FP64FP64 and FP64FP32 only (got compute=%d store=%d)", c, s);
}

// coll: XLBHIP_BGK / KBC / SMAGORINSKY_LES_BGK, | COLL_FORCED with a force vector or buoyancy
template <class L>
int launch_scalar_lattice(const ScalarLaunch& q, int coll) {
  switch (coll) {
    case XLBHIP_BGK: return launch_scalar_coll<L, XLBHIP_BGK>(q);
    case XLBHIP_BGK | COLL_FORCED: return launch_scalar_coll<L, XLBHIP_BGK | COLL_FORCED>(q);
    case XLBHIP_SMAGORINSKY_LES_BGK: return launch_scalar_coll<L, XLBHIP_SMAGORINSKY_LES_BGK>(q);
    case XLBHIP_SMAGORINSKY_LES_BGK | COLL_FORCED: return launch_scalar_coll<L, XLBHIP_SMAGORINSKY_LES_BGK | COLL_FORCED>(q);
  }
  if constexpr (L::ID != XLBHIP_D3Q19) {
    if (coll == XLBHIP_KBC) return launch_scalar_coll<L, XLBHIP_KBC>(q);
    if (coll == (XLBHIP_KBC | COLL_FORCED)) return launch_scalar_coll<L, XLBHIP_KBC | COLL_FORCED>(q);
  }
  XLB_FAIL("scalar transport: collision variant %d not built for this lattice", coll);
}

// defined one per translation unit (scalar_<lattice>.hip)
int launch_scalar_d2q9(const ScalarLaunch& q, int coll);
int launch_scalar_d3q19(const ScalarLaunch& q, int coll);
int launch_scalar_d3q27(const ScalarLaunch& q, int coll);

}  // namespace xlb
