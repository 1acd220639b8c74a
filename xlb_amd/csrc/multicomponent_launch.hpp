// Type-erased launch descriptor of the two-component Shan-Chen step's kernels and the per-lattice dispatcher that each
// multicomponent_<lattice>.hip instantiates.  From step_launch.hpp: the shared arguments (step_args), the policies (by_three_policies)
// and the launch (launch_rows); the block is launch_shape.hpp's.  One cell per thread: there are no `vec` variants.
#pragma once
#include "common.hpp"
#include "multicomponent_step_kernel.hpp"
#include "step_launch.hpp"

namespace xlb {

enum class MixKernel : int { density = 0, step = 1, out = 2 };

struct MixLaunch {
  StepLaunch f;  // component A's part and everything shared (f.halo == 0, all of x; f.omega: omega_A); f.dst only for MixKernel::step
  const void* src_b;
  void* dst_b;
  double omega_b;
  void *rho_a, *rho_b;
  const void *wall_a, *wall_b;  // compute dtype [256]
  double g_aa, g_ab, g_bb;
  double force[3];
  void *out_rho_a, *out_rho_b, *out_u, *out_force_a, *out_force_b;  // MixKernel::out, compute dtype, each may be nullptr
  size_t u_stride, force_a_stride, force_b_stride;
};

// in whose name by_three_policies refuses a policy (the launch and xlbhip_multicomponent_create)
constexpr const char* MULTICOMPONENT_POLICY_SUBJECT = "the multicomponent step is";

template <class L, class T, class S, int HASBC>
int launch_mix_typed(const MixLaunch& q, MixKernel which) {
  const StepLaunch& p = q.f;
  MixArgs<T, S> ma = {};
  ma.f = step_args<T, S>(p, 1);
  ma.src_b = static_cast<const S*>(q.src_b);
  ma.dst_b = static_cast<S*>(q.dst_b);
  ma.omega_b = static_cast<T>(q.omega_b);
  ma.rho_a = static_cast<T*>(q.rho_a);
  ma.rho_b = static_cast<T*>(q.rho_b);
  ma.wall_a = static_cast<const T*>(q.wall_a);
  ma.wall_b = static_cast<const T*>(q.wall_b);
  ma.model.g_aa = static_cast<T>(q.g_aa);
  ma.model.g_ab = static_cast<T>(q.g_ab);
  ma.model.g_bb = static_cast<T>(q.g_bb);
  for (int k = 0; k < 3; ++k) ma.model.force[k] = static_cast<T>(q.force[k]);
  ma.out_rho_a = static_cast<T*>(q.out_rho_a);
  ma.out_rho_b = static_cast<T*>(q.out_rho_b);
  ma.out_u = static_cast<T*>(q.out_u);
  ma.out_force_a = static_cast<T*>(q.out_force_a);
  ma.out_force_b = static_cast<T*>(q.out_force_b);
  ma.u_stride = q.u_stride;
  ma.force_a_stride = q.force_a_stride;
  ma.force_b_stride = q.force_b_stride;
  void (*const kernel)(MixArgs<T, S>) = which == MixKernel::density ? k_mix_density<L, T, S, HASBC>
                                        : which == MixKernel::step  ? k_mix_step<L, T, S, HASBC>
                                                                    : k_mix_out<L, T, S, HASBC>;
  return launch_rows(kernel, row_block_shape(p.nz, p.ny, p.nx, 256, 0), p.stream, ma);
}

template <class L, class T, class S>
int launch_mix_policy(const MixLaunch& q, MixKernel which) {
  return q.f.has_bc ? launch_mix_typed<L, T, S, 1>(q, which) : launch_mix_typed<L, T, S, 0>(q, which);
}

template <class L>
int launch_mix_lattice(const MixLaunch& q, MixKernel which) {
  return by_three_policies(MULTICOMPONENT_POLICY_SUBJECT, q.f.compute_dtype, q.f.store_dtype,
                           [&](auto T, auto S) { return launch_mix_policy<L, decltype(T), decltype(S)>(q, which); });
}

// defined one per translation unit (multicomponent_<lattice>.hip)
int launch_multicomponent_d2q9(const MixLaunch& q, MixKernel which);
int launch_multicomponent_d3q19(const MixLaunch& q, MixKernel which);
int launch_multicomponent_d3q27(const MixLaunch& q, MixKernel which);

}  // namespace xlb
