// Type-erased launch descriptor of the fused adjoint step and the per-lattice dispatcher that each adjoint_<lattice>.hip
// instantiates (the scheme of step_launch.hpp).
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

// One cell per thread, lanes along z: a row in equal chunks of whole waves, rows stacked to fill the block (launch_typed's shape)
inline void adjoint_geometry(int nx, int ny, int nz, dim3& block, dim3& grid) {
  int tz = nz;
  if (tz > ADJ_BLOCK) {
    const int chunks = (nz + ADJ_BLOCK - 1) / ADJ_BLOCK;
    tz = (nz + chunks - 1) / chunks;
    tz = (tz + 63) / 64 * 64;
    if (tz > ADJ_BLOCK) tz = ADJ_BLOCK;
  }
  int ty = ADJ_BLOCK / tz;
  if (ty < 1) ty = 1;
  if (ty > ny) ty = ny;
  block = dim3(tz, ty, 1);
  grid = dim3((nz + tz - 1) / tz, (ny + ty - 1) / ty, nx);
}
inline size_t adjoint_blocks(int nx, int ny, int nz) {
  dim3 block, grid;
  adjoint_geometry(nx, ny, nz, block, grid);
  return (size_t)grid.x * grid.y * grid.z;
}

template <class L, class T, class S, int IN, int OUT, int HASBC>
int launch_adjoint_typed(const AdjointLaunch& q) {
  const StepLaunch& p = q.f;
  AdjointArgs<T, S> aa = {};
  StepArgs<T, S>& a = aa.f;
  a.src = static_cast<const S*>(p.src);
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
  a.x_count = p.nx;
  a.nzq = p.nz;
  a.omega = static_cast<T>(p.omega);
  aa.in = static_cast<const S*>(q.in);
  aa.out = static_cast<S*>(q.out);
  aa.in_stride = q.in_stride;
  aa.out_stride = q.out_stride;
  aa.partial = q.partial;
  aa.gmask = q.gmask;
  dim3 block, grid;
  adjoint_geometry(p.nx, p.ny, p.nz, block, grid);
  XLB_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "grid too large: ny/ty=%u nx=%u", grid.y, grid.z);
  hipLaunchKernelGGL((k_adjoint_step<L, T, S, IN, OUT, HASBC>), grid, block, 0, p.stream, aa);
  XLB_HIP(hipGetLastError());
  return 0;
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
  const int c = q.f.compute_dtype, s = q.f.store_dtype;
  if (c == XLBHIP_F32 && s == XLBHIP_F32) return launch_adjoint_policy<L, float, float>(q);
  if (c == XLBHIP_F64 && s == XLBHIP_F64) return launch_adjoint_policy<L, double, double>(q);
  if (c == XLBHIP_F64 && s == XLBHIP_F32) return launch_adjoint_policy<L, double, float>(q);
  XLB_FAIL("the adjoint step is built for FP32FP32, FP64FP64 and FP64FP32 only (got compute=%d store=%d)", c, s);
}

// defined one per translation unit (adjoint_<lattice>.hip)
int launch_adjoint_d2q9(const AdjointLaunch& q);
int launch_adjoint_d3q19(const AdjointLaunch& q);
int launch_adjoint_d3q27(const AdjointLaunch& q);

}  // namespace xlb
