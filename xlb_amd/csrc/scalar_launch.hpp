// Type-erased launch descriptor of the coupled fluid + scalar step and the per-lattice dispatcher that each scalar_<lattice>.hip
// instantiates.  From step_launch.hpp: the fluid's arguments (step_args), the policies (by_three_policies) and the launch (launch_rows);
// the block is launch_shape.hpp's.
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

// in whose name by_three_policies refuses a policy (the launch and xlbhip_scalar_create)
constexpr const char* SCALAR_POLICY_SUBJECT = "scalar transport is";

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
  return launch_rows(k_step_scalar<L, T, S, VEC, COLL, HASBC>, row_block_shape(sa.f.nzq, p.ny, p.nx, 256, 0), p.stream, sa);
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
  return by_three_policies(SCALAR_POLICY_SUBJECT, q.f.compute_dtype, q.f.store_dtype,
                           [&](auto T, auto S) { return launch_scalar_policy<L, decltype(T), decltype(S), COLL>(q); });
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
