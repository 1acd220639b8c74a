// Type-erased launch descriptors of the porous step and of its adjoint step, and the per-lattice dispatchers that each
// porous_<lattice>.hip instantiates.  From step_launch.hpp: step_args, by_three_policies, launch_rows; from adjoint_launch.hpp: the
// adjoint's descriptor and geometry (the block shape and the count of per-block partial sums).
#pragma once
#include "adjoint_launch.hpp"
#include "porous_step_kernel.hpp"

namespace xlb {

struct PorousLaunch {
  StepLaunch f;       // f.halo == 0, all of x
  const void* alpha;  // compute dtype, one value per cell
};

struct PorousAdjointLaunch {
  AdjointLaunch a;    // in_mode as the adjoint's, out_mode == ADJ_OUT_MU
  const void* alpha;  // compute dtype, one value per cell
  double* galpha;     // fp64, one value per cell
};

// in whose name by_three_policies refuses a policy (the launches and xlbhip_porous_create)
constexpr const char* POROUS_POLICY_SUBJECT = "the porous step is";

template <class L, class T, class S, int HASBC>
int launch_porous_typed(const PorousLaunch& q) {
  const StepLaunch& p = q.f;
  PorousArgs<T, S> pa = {};
  pa.f = step_args<T, S>(p, 1);
  pa.alpha = static_cast<const T*>(q.alpha);
  return launch_rows(k_porous_step<L, T, S, HASBC>, row_block_shape(p.nz, p.ny, p.x_count, 256, 0), p.stream, pa);
}

template <class L>
int launch_porous_lattice(const PorousLaunch& q) {
  return by_three_policies(POROUS_POLICY_SUBJECT, q.f.compute_dtype, q.f.store_dtype, [&](auto T, auto S) {
    return q.f.has_bc ? launch_porous_typed<L, decltype(T), decltype(S), 1>(q) : launch_porous_typed<L, decltype(T), decltype(S), 0>(q);
  });
}

template <class L, class T, class S, int IN, int HASBC>
int launch_porous_adjoint_typed(const PorousAdjointLaunch& q) {
  const StepLaunch& p = q.a.f;
  PorousAdjointArgs<T, S> pa = {};
  pa.a.f = step_args<T, S>(p, 1);  // (no dst: the kernel writes a.out)
  pa.a.in = static_cast<const S*>(q.a.in);
  pa.a.out = static_cast<S*>(q.a.out);
  pa.a.in_stride = q.a.in_stride;
  pa.a.out_stride = q.a.out_stride;
  pa.a.partial = q.a.partial;
  pa.a.gmask = q.a.gmask;
  pa.alpha = static_cast<const T*>(q.alpha);
  pa.galpha = q.galpha;
  return launch_rows(k_porous_adjoint_step<L, T, S, IN, ADJ_OUT_MU, HASBC>, adjoint_geometry(p.nx, p.ny, p.nz), p.stream, pa);
}

template <class L, class T, class S, int HASBC>
int launch_porous_adjoint_mode(const PorousAdjointLaunch& q) {
  XLB_REQUIRE(q.a.out_mode == ADJ_OUT_MU, "porous adjoint step: the launch that leaves lam is the plain adjoint's (out_mode=%d)", q.a.out_mode);
  return q.a.in_mode == ADJ_IN_LAMBDA ? launch_porous_adjoint_typed<L, T, S, ADJ_IN_LAMBDA, HASBC>(q)
                                      : launch_porous_adjoint_typed<L, T, S, ADJ_IN_MU, HASBC>(q);
}

template <class L>
int launch_porous_adjoint_lattice(const PorousAdjointLaunch& q) {
  return by_three_policies(POROUS_POLICY_SUBJECT, q.a.f.compute_dtype, q.a.f.store_dtype, [&](auto T, auto S) {
    return q.a.f.has_bc ? launch_porous_adjoint_mode<L, decltype(T), decltype(S), 1>(q) : launch_porous_adjoint_mode<L, decltype(T), decltype(S), 0>(q);
  });
}

// defined one per translation unit (porous_<lattice>.hip)
int launch_porous_d2q9(const PorousLaunch& q);
int launch_porous_d3q19(const PorousLaunch& q);
int launch_porous_d3q27(const PorousLaunch& q);
int launch_porous_adjoint_d2q9(const PorousAdjointLaunch& q);
int launch_porous_adjoint_d3q19(const PorousAdjointLaunch& q);
int launch_porous_adjoint_d3q27(const PorousAdjointLaunch& q);

}  // namespace xlb
