// The fused adjoint step: ONE kernel per step of a backward sweep.  Per cell it re-pulls the stencil of the forward state f_n, applies
// the streaming rules (cell.hpp: apply_streaming_bc) to get f*, gathers the incoming cotangent, applies the transposed rules of
// adjoint_kernels.hpp and stores q values.
//
// State carried between the steps of a sweep: mu_n = dL/df*_n (the output of the collision transpose) in the store dtype, NOT lam_n.
// The forward read map is not injective — f_n[opp l](x) at a halfway cell is read by the bounce-back at x and by the periodic pull of
// the cell behind the wall — so lam_n cannot be pushed with stores, and atomics would unpin the order of its sums.  Instead the
// READER gathers:  lam_n[l](y) = mu_n[l](y + c_l), or 0 where the cell y + c_l replaced its pull of l (one word of gather bits per
// cell, built once per pair of masks: k_adjoint_gather_mask), plus the reader's own redirected mu_n (adjoint_own_terms).  lam_n is rounded to the store dtype in
// registers, so that a sweep gives the bits of single steps chained through stored cotangents.  Three instantiations by what enters
// and leaves:
//   IN_LAMBDA, OUT_MU      first step of a sweep: the cotangent field is lam_{n+1} itself
//   IN_MU,     OUT_MU      every other step: 3 q s bytes per cell (f_n, mu_{n+1}, mu_n) + the masks
//   IN_MU,     OUT_LAMBDA  the end of a sweep: lam_0 from mu_0, no forward state
// Every OUT_MU launch also leaves one fp64 partial sum of the cells' omega terms per block (fixed order: see block_sum_fixed).
//
// Addressing is the row front end's (row_kernel.hpp) with one cell per thread.
#pragma once
#include "adjoint_kernels.hpp"
#include "step_kernel.hpp"

namespace xlb {

enum { ADJ_IN_LAMBDA = 0, ADJ_IN_MU = 1 };
enum { ADJ_OUT_LAMBDA = 0, ADJ_OUT_MU = 1 };
constexpr int ADJ_BLOCK = 256;

template <class T, class S>
struct AdjointArgs {
  StepArgs<T, S> f;  // the forward state and the boundary tables, as k_step takes them (f.src = f_n, f.halo == 0, f.dst unused)
  const S* in;       // lam_{n+1} (IN_LAMBDA) or mu_{n+1} (IN_MU)
  S* out;            // mu_n (OUT_MU) or lam_n (OUT_LAMBDA)
  size_t in_stride, out_stride;  // elements per population plane
  double* partial;   // [blocks] omega-term sums (OUT_MU)
  const uint32_t* gmask;  // (nx, ny, nz) gather bits of the transposed streaming (IN_MU with boundary conditions)
};

// Sum of one value per thread over the block in an order fixed by the block shape alone: a tree over ADJ_BLOCK slots (slots beyond
// the block hold 0).  Every thread of the block calls; the result is valid in thread 0.
__device__ __forceinline__ double block_sum_fixed(double v) {
  __shared__ double red[ADJ_BLOCK];
  const unsigned n = blockDim.x * blockDim.y, t = threadIdx.y * blockDim.x + threadIdx.x;
  red[t] = v;
  for (unsigned i = t + n; i < (unsigned)ADJ_BLOCK; i += n) red[i] = 0.0;
  __syncthreads();
  for (unsigned s = ADJ_BLOCK / 2; s > 0; s >>= 1) {
    for (unsigned i = t; i < s; i += n) red[i] += red[i + s];
    __syncthreads();
  }
  return red[0];
}

// HASBC: 0 = no boundary conditions, 1 = equilibrium, halfway, fullway, do-nothing
template <class L, class T, class S, int IN, int OUT, int HASBC>
__global__ void __launch_bounds__(ADJ_BLOCK) k_adjoint_step(const AdjointArgs<T, S> aa) {
  constexpr int Q = L::Q;
  const StepArgs<T, S>& a = aa.f;
  RowCell r;
  // (idle threads stay for the block sum; they load cell (y, z) = (0, 0) and store nothing)
  const bool active = row_cell_of_thread<1>(a, blockIdx.x, blockIdx.y, 0, r);
  const size_t xplane = (size_t)r.Xs[1] * r.plane_cells;  // the thread's own x plane; uniform
  const unsigned cell = r.cell_in_plane;

  unsigned id = 0u, kind = K_NONE, m = 0u;
  if constexpr (HASBC != 0) {
    unsigned ids[1];
    const bool any_bc = load_bc_ids<1>(a.bc + xplane, cell, ids);
    id = ids[0];
    if (any_bc) {
      kind = kind_of(a, id);
      m = ld(a.miss + xplane, opaque(cell * 4u));
    }
  }

  T lam[Q];
  if constexpr (IN == ADJ_IN_LAMBDA) {
    static_for<Q>([&](auto lc) {
      constexpr int l = decltype(lc)::value;
      lam[l] = to_compute<T, S>(ld(aa.in + (size_t)l * aa.in_stride + xplane, cell * (unsigned)sizeof(S)));
    });
  } else {
    // ---- transposed streaming: lam_n[l] = mu[l](cell + c_l) unless that cell replaced its pull of l, + the own redirected mu ----
    unsigned gbits = 0u;
    if constexpr (HASBC != 0) gbits = ld(aa.gmask + xplane, cell * 4u);
    static_for<Q>([&](auto lc) {
      constexpr int l = decltype(lc)::value;
      S w[1];
      pull_plane<L, opp<L>(l)>(aa.in + (size_t)l * aa.in_stride, r, w);  // the value at cell + c_l
      T v = to_compute<T, S>(w[0]);
      if constexpr (HASBC != 0) {
        if ((gbits >> l) & 1u) v = T(0);  // the cell there replaced its pull of l by its rule
      }
      lam[l] = v;
    });
    if constexpr (HASBC != 0) {
      if (kind == K_HW || kind == K_DN) {
        T own[Q];
        load_own_cell<L, false>(aa.in, aa.in_stride, xplane, cell, own);
        adjoint_own_terms<L, T>(kind, m, own, lam);
      }
    }
    if constexpr (sizeof(S) != sizeof(T)) {
      static_for<Q>([&](auto lc) {
        constexpr int l = decltype(lc)::value;
        lam[l] = to_compute<T, S>(to_store<S, T>(lam[l]));
      });
    }
  }

  T term = T(0);
  if constexpr (OUT == ADJ_OUT_MU) {
    // ---- f*: the forward pull of f_n and the streaming rule of the cell ----
    T fs[Q];
    static_for<Q>([&](auto lc) {
      constexpr int l = decltype(lc)::value;
      S w[1];
      pull_plane<L, l>(a.src + (size_t)l * a.plane_stride, r, w);
      fs[l] = to_compute<T, S>(w[0]);
    });
    if constexpr (HASBC != 0) {
      if (kind == K_EQ || kind == K_HW || kind == K_DN) {
        const T* val = opaque(a.bc_values + id * 27u);
        T pre[Q];
        load_own_cell<L, false>(a.src, a.plane_stride, xplane, cell, pre);
        const T none[5] = {T(0), T(0), T(0), T(0), T(0)};
        // (a constant kind per call: the rules of the kinds the adjoint does not cover fold away)
        if (kind == K_EQ)
          apply_streaming_bc<L, T>(XLBHIP_BC_EQUILIBRIUM, fs, pre, m, val, none, nullptr);
        else if (kind == K_HW)
          apply_streaming_bc<L, T>(XLBHIP_BC_HALFWAY_BB, fs, pre, m, val, none, nullptr);
        else
          apply_streaming_bc<L, T>(XLBHIP_BC_DO_NOTHING, fs, pre, m, val, none, nullptr);
      }
    }
    term = adjoint_local_cell<L, T>(kind, fs, lam, a.omega);
  }

  if (active) store_planes<true, 1, Q>(aa.out, aa.out_stride, xplane, cell, lam);

  if constexpr (OUT == ADJ_OUT_MU) {
    // (after the stores, so that they do not wait for the block's barriers)
    const double total = block_sum_fixed(active ? (double)term : 0.0);
    if (threadIdx.x == 0 && threadIdx.y == 0) aa.partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = total;
  }
}

}  // namespace xlb
