// Type-erased launch descriptor of the fused adjoint step and the per-lattice dispatcher that each adjoint_<lattice>.hip
// instantiates.  From step_launch.hpp: the forward part's arguments (step_args), the policies (by_three_policies) and the launch
// (launch_rows); the block is launch_shape.hpp's.
#pragma once
#include "adjoint_step_kernel.hpp"
#include "common.hpp"
#include "step_launch.hpp"

namespace xlb {

struct AdjointLaunch {
  StepLaunch f;  // the forward state f_n (f.src; unused by an OUT_LAMBDA launch) and the boundary tables; f.halo == 0, all of x
  const void* in;
  void* out;
  size_t in_stride, out_stride;
  int in_mode, out_mode;  // ADJ_IN_* / ADJ_OUT_*
  double* partial;        // [adjoint_blocks()] (OUT_MU)
  const uint32_t* gmask;  // gather bits (IN_MU with boundary conditions)
};

// One cell per thread, lanes along z, blocks of ADJ_BLOCK threads in the row kernels' shape (launch_shape.hpp): the launch and the
// count of per-block partial sums both come from here
inline RowBlockShape adjoint_geometry(int nx, int ny, int nz) { return row_block_shape(nz, ny, nx, ADJ_BLOCK, 0); }
inline size_t adjoint_blocks(int nx, int ny, int nz) {
  const RowBlockShape sh = adjoint_geometry(nx, ny, nz);
  return (size_t)sh.gx * sh.gy * sh.gz;
}

// in whose name by_three_policies refuses a policy (the launch and xlbhip_adjoint_create)
constexpr const char* ADJOINT_POLICY_SUBJECT = "the adjoint step is";

template <class L, class T, class S, int IN, int OUT, int HASBC>
int launch_adjoint_typed(const AdjointLaunch& q) {
  const StepLaunch& p = q.f;
  AdjointArgs<T, S> aa = {};
  aa.f = step_args<T, S>(p, 1);  // (nzq = nz: one cell per thread; no dst: p.dst is null, the kernel writes aa.out)
  aa.in = static_cast<const S*>(q.in);
  aa.out = static_cast<S*>(q.out);
  aa.in_stride = q.in_stride;
  aa.out_stride = q.out_stride;
  aa.partial = q.partial;
  aa.gmask = q.gmask;
  return launch_rows(k_adjoint_step<L, T, S, IN, OUT, HASBC>, adjoint_geometry(p.nx, p.ny, p.nz), p.stream, aa);
}

template <class L, class T, class S, int HASBC>
int launch_adjoint_mode(const AdjointLaunch& q) {
  if (q.in_mode == ADJ_IN_LAMBDA && q.out_mode == ADJ_OUT_MU) return launch_adjoint_typed<L, T, S, ADJ_IN_LAMBDA, ADJ_OUT_MU, HASBC>(q);
  if (q.in_mode == ADJ_IN_MU && q.out_mode == ADJ_OUT_MU) return launch_adjoint_typed<L, T, S, ADJ_IN_MU, ADJ_OUT_MU, HASBC>(q);
  if (q.in_mode == ADJ_IN_MU && q.out_mode == ADJ_OUT_LAMBDA) return launch_adjoint_typed<L, T, S, ADJ_IN_MU, ADJ_OUT_LAMBDA, HASBC>(q);
  XLB_FAIL("adjoint step: no kernel takes lam and leaves lam (in_mode=%d out_mode=%d)", q.in_mode, q.out_mode);
}

template <class L, class T, class S>
int launch_adjoint_policy(const AdjointLaunch& q) {
  return q.f.has_bc ? launch_adjoint_mode<L, T, S, 1>(q) : launch_adjoint_mode<L, T, S, 0>(q);
}

template <class L>
int launch_adjoint_lattice(const AdjointLaunch& q) {
  return by_three_policies(ADJOINT_POLICY_SUBJECT, q.f.compute_dtype, q.f.store_dtype,
                           [&](auto T, auto S) { return launch_adjoint_policy<L, decltype(T), decltype(S)>(q); });
}

// defined one per translation unit (adjoint_<lattice>.hip)
int launch_adjoint_d2q9(const AdjointLaunch& q);
int launch_adjoint_d3q19(const AdjointLaunch& q);
int launch_adjoint_d3q27(const AdjointLaunch& q);

}  // namespace xlb
