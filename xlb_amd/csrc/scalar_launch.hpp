// Type-erased launch descriptor of the coupled fluid + scalar step and the per-lattice dispatcher that each scalar_<lattice>.hip
// instantiates (the scheme of step_launch.hpp; the fluid's arguments are step_args', the block is launch_shape.hpp's).
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
  sa.f = step_args<T, S>(p, VEC);
  sa.gsrc = static_cast<const S*>(q.gsrc);
  sa.gdst = static_cast<S*>(q.gdst);
  sa.g_plane_stride = q.g_plane_stride;
  sa.sc_rule = q.sc_rule;
  sa.sc_value = static_cast<const T*>(q.sc_value);
  sa.cp = q.cp;
  sa.omega_s = static_cast<T>(q.omega_s);
  const RowBlockShape sh = row_block_shape(sa.f.nzq, p.ny, p.nx, 256, 0);
  const dim3 block(sh.tz, sh.ty, 1), grid(sh.gx, sh.gy, sh.gz);
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
