// Type-erased launch descriptor of the Shan-Chen step's kernels and the per-lattice dispatcher that each multiphase_<lattice>.hip
// instantiates.  From step_launch.hpp: the fluid's arguments (step_args), the policies (by_three_policies) and the launch (launch_rows);
// the block is launch_shape.hpp's.  One cell per thread: there are no `vec` variants.
#pragma once
#include "common.hpp"
#include "multiphase_step_kernel.hpp"
#include "step_launch.hpp"

namespace xlb {

enum class MultiphaseKernel : int { psi = 0, step = 1, out = 2 };

struct MultiphaseLaunch {
  StepLaunch f;  // the fluid's part (f.halo == 0, all of x); f.dst only for MultiphaseKernel::step
  void* psi;
  const void* psi_wall;  // compute dtype [256]
  int form;              // PSI_*
  double g;
  double par[4];
  double force[3];
  void *out_rho, *out_u, *out_force;  // MultiphaseKernel::out, compute dtype, each may be nullptr
  size_t u_stride, force_stride;
};

// in whose name by_three_policies refuses a policy (the launch and xlbhip_multiphase_create)
constexpr const char* MULTIPHASE_POLICY_SUBJECT = "the multiphase step is";

template <class L, class T, class S, int HASBC>
int launch_multiphase_typed(const MultiphaseLaunch& q, MultiphaseKernel which) {
  const StepLaunch& p = q.f;
  MultiphaseArgs<T, S> ma = {};
  ma.f = step_args<T, S>(p, 1);
  ma.psi = static_cast<T*>(q.psi);
  ma.psi_wall = static_cast<const T*>(q.psi_wall);
  ma.model.form = q.form;
  ma.model.neg_g = static_cast<T>(-q.g);
  for (int k = 0; k < 4; ++k) ma.model.par[k] = static_cast<T>(q.par[k]);
  for (int k = 0; k < 3; ++k) ma.model.force[k] = static_cast<T>(q.force[k]);
  ma.out_rho = static_cast<T*>(q.out_rho);
  ma.out_u = static_cast<T*>(q.out_u);
  ma.out_force = static_cast<T*>(q.out_force);
  ma.u_stride = q.u_stride;
  ma.force_stride = q.force_stride;
  void (*const kernel)(MultiphaseArgs<T, S>) = which == MultiphaseKernel::psi    ? k_psi<L, T, S, HASBC>
                                               : which == MultiphaseKernel::step ? k_step_multiphase<L, T, S, HASBC>
                                                                                 : k_multiphase_out<L, T, S, HASBC>;
  return launch_rows(kernel, row_block_shape(p.nz, p.ny, p.nx, 256, 0), p.stream, ma);
}

template <class L, class T, class S>
int launch_multiphase_policy(const MultiphaseLaunch& q, MultiphaseKernel which) {
  return q.f.has_bc ? launch_multiphase_typed<L, T, S, 1>(q, which) : launch_multiphase_typed<L, T, S, 0>(q, which);
}

template <class L>
int launch_multiphase_lattice(const MultiphaseLaunch& q, MultiphaseKernel which) {
  return by_three_policies(MULTIPHASE_POLICY_SUBJECT, q.f.compute_dtype, q.f.store_dtype,
                           [&](auto T, auto S) { return launch_multiphase_policy<L, decltype(T), decltype(S)>(q, which); });
}

// defined one per translation unit (multiphase_<lattice>.hip)
int launch_multiphase_d2q9(const MultiphaseLaunch& q, MultiphaseKernel which);
int launch_multiphase_d3q19(const MultiphaseLaunch& q, MultiphaseKernel which);
int launch_multiphase_d3q27(const MultiphaseLaunch& q, MultiphaseKernel which);

}  // namespace xlb
