// The fused kernels of the porous step (porous_kernels.hpp): the forward step and the step of a backward sweep.
//
//   k_porous_step          the single-step kernel's pulls and non-temporal stores through the row front end (row_kernel.hpp), one cell
//                          per thread, + one compute-dtype value of alpha per cell: 2 q s + s_c bytes per cell (D3Q19 fp32: 156).
//   k_porous_adjoint_step  the fused adjoint step of adjoint_step_kernel.hpp with the porous transpose.  It leaves mu (OUT_MU), reads
//                          alpha and does a read-add-write of the cell's entry of the fp64 gradient field dL/dalpha:
//                          3 q s + s_c + 16 bytes per cell (D3Q19 fp32: 248).  The gradient cell belongs to its thread: no atomics, and
//                          the order of its sum across the steps of a sweep is the sweep's order.  The field is fp64 under every
//                          policy, like the omega scalar, so that long sweeps do not round small terms away.
//
// The closing launch of a sweep (IN_MU, OUT_LAMBDA) is the transposed streaming alone and does not depend on alpha: it is
// k_adjoint_step's.  The omega block sum is k_adjoint_step's too (block_sum_fixed).
#pragma once
#include "adjoint_step_kernel.hpp"
#include "porous_kernels.hpp"

namespace xlb {

template <class T, class S>
struct PorousArgs {
  StepArgs<T, S> f;  // as k_step takes it (fields without ghost planes: f.halo == 0)
  const T* alpha;    // (nx, ny, nz), compute dtype
};

template <class T, class S>
struct PorousAdjointArgs {
  AdjointArgs<T, S> a;  // as k_adjoint_step takes it
  const T* alpha;       // (nx, ny, nz), compute dtype
  double* galpha;       // (nx, ny, nz) dL/dalpha, read-add-written
};

// HASBC: 0 = no boundary conditions, 1 = equilibrium, halfway, fullway, do-nothing
template <class L, class T, class S, int HASBC>
__global__ void __launch_bounds__(256) k_porous_step(const PorousArgs<T, S> pa) {
  constexpr int Q = L::Q;
  const StepArgs<T, S>& a = pa.f;
  RowCell r;
  if (!row_cell_of_thread<1>(a, blockIdx.x, blockIdx.y, 0, r)) return;
  const size_t xplane = (size_t)r.Xs[1] * r.plane_cells;  // the thread's own x plane; uniform
  const unsigned cell = r.cell_in_plane;

  T f[Q];
  static_for<Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    S v[1];
    pull_plane<L, l>(a.src + (size_t)l * a.plane_stride, r, v);
    f[l] = to_compute<T, S>(v[0]);
  });
  const T alpha = ld(pa.alpha + xplane, cell * (unsigned)sizeof(T));

  bool fullway = false;
  if constexpr (HASBC != 0) {
    unsigned ids[1];
    if (load_bc_ids<1>(a.bc + xplane, cell, ids)) {
      const unsigned id = ids[0];
      const unsigned kind = kind_of(a, id);
      const T* val = opaque(a.bc_values + id * 27u);
      if (kind == K_EQ) {
        static_for<Q>([&](auto lc) {
          constexpr int l = decltype(lc)::value;
          f[l] = val[l];
        });
      } else if (kind == K_HW) {
        const unsigned m = ld(a.miss + xplane, opaque(cell * 4u));
        T own[Q];
        load_own_cell<L, true>(a.src, a.plane_stride, xplane, cell, own);
        static_for<Q>([&](auto lc) {
          constexpr int l = decltype(lc)::value;
          const T pre = own[l] + val[l];
          if ((m >> l) & 1u) f[l] = pre;
        });
      } else if (kind == K_DN) {
        load_own_cell<L, false>(a.src, a.plane_stride, xplane, cell, f);
      } else if (kind == K_FW) {
        fullway = true;
      }
    }
  }
  if (!fullway) {
    porous_collide<L, T>(f, a.omega, alpha);
  } else {
    adjoint_fullway<L, T>(f);  // f_out[l] = f*[opp l]: the swap is its own transpose
  }
  store_planes<true, 1, Q>(a.dst, a.plane_stride, xplane, cell, f);
}

// IN: ADJ_IN_LAMBDA (the first step of a sweep) or ADJ_IN_MU; OUT: ADJ_OUT_MU only (the closing launch is k_adjoint_step's)
template <class L, class T, class S, int IN, int OUT, int HASBC>
__global__ void __launch_bounds__(ADJ_BLOCK) k_porous_adjoint_step(const PorousAdjointArgs<T, S> pa) {
  static_assert(OUT == ADJ_OUT_MU, "the launch that leaves lam does not depend on alpha: k_adjoint_step");
  constexpr int Q = L::Q;
  const AdjointArgs<T, S>& aa = pa.a;
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

  // ---- f*: the forward pull of f_n and the streaming rule of the cell ----
  T fs[Q];
  static_for<Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    S w[1];
    pull_plane<L, l>(a.src + (size_t)l * a.plane_stride, r, w);
    fs[l] = to_compute<T, S>(w[0]);
  });
  const T alpha = ld(pa.alpha + xplane, cell * (unsigned)sizeof(T));
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
  const PorousTerms<T> terms = porous_adjoint_local_cell<L, T>(kind, fs, lam, a.omega, alpha);

  if (active) {
    store_planes<true, 1, Q>(aa.out, aa.out_stride, xplane, cell, lam);
    // the cell's own entry of dL/dalpha: this thread is its only writer in the launch, and launches run in stream order
    double* g = pa.galpha + xplane;
    const unsigned gb = cell * (unsigned)sizeof(double);
    const double sum = ld(g, gb) + (double)terms.alpha;
    *reinterpret_cast<double*>(reinterpret_cast<char*>(g) + gb) = sum;
  }

  // (after the stores, so that they do not wait for the block's barriers)
  const double total = block_sum_fixed(active ? (double)terms.omega : 0.0);
  if (threadIdx.x == 0 && threadIdx.y == 0) aa.partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = total;
}

}  // namespace xlb
