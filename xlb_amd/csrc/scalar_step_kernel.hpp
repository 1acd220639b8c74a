// The coupled fluid + scalar step: ONE kernel pulls and stores both fields (q + 2 d + 1 populations per cell each way; D3Q19 fp32:
// 208 B per cell against the fluid step's 152 B), because the scalar's collision needs the velocity the fluid step holds in registers
// and the fluid's force needs the scalar sum before it collides — a second pass would re-read the fluid field for either.
//
// Addressing, lane mapping, row-end handling, id and own-cell loads and the stores are the row front end's (row_kernel.hpp); the fluid's
// rule functions are cell.hpp's, the scalar's own rules are in scalar_kernels.hpp.
#pragma once
#include "scalar_kernels.hpp"
#include "step_kernel.hpp"

namespace xlb {

template <class T, class S>
struct ScalarStepArgs {
  StepArgs<T, S> f;  // the fluid's part, as k_step takes it (fields without ghost planes: f.halo == 0)
  const S* gsrc;
  S* gdst;
  size_t g_plane_stride;   // elements
  const uint8_t* sc_rule;  // [256] SCALAR_* by bc id
  const T* sc_value;       // [256] Dirichlet value by bc id
  ScalarCoupling cp;
  T omega_s;
};

// HASBC: 0 = no boundary conditions, 2 = every kind the coupled step supports (equilibrium, halfway, fullway, do-nothing, Zou-He /
// Regularized with constant values, extrapolation outflow).  Stores are non-temporal.
template <class L, class T, class S, int VEC, int COLL, int HASBC>
__global__ void __launch_bounds__(256) k_step_scalar(const ScalarStepArgs<T, S> sa) {
  typedef ScalarSet<L> G;
  constexpr int Q = L::Q, QS = G::Q;
  const StepArgs<T, S>& a = sa.f;
  RowCell r;
  if (!row_cell_of_thread<VEC>(a, blockIdx.x, blockIdx.y, 0, r)) return;
  const size_t xplane = (size_t)r.Xs[1] * r.plane_cells;  // the thread's own x plane; uniform

  T f[VEC][Q];
  T g[VEC][QS];

  // ---- pull streaming of both fields ----
  static_for<Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    S v[VEC];
    pull_plane<L, l>(a.src + (size_t)l * a.plane_stride, r, v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) f[k][l] = to_compute<T, S>(v[k]);
  });
  static_for<QS>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    S v[VEC];
    pull_plane<L, G::dir(j)>(sa.gsrc + (size_t)j * sa.g_plane_stride, r, v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) g[k][j] = to_compute<T, S>(v[k]);
  });

  unsigned ids[VEC];
  bool any_bc = false;
  if constexpr (HASBC != 0) any_bc = load_bc_ids<VEC>(a.bc + xplane, r.cell_in_plane, ids);

#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    bool fullway = false;
    if constexpr (HASBC != 0) {
      if (any_bc && ids[k] != 0u) {
        // rare path: every boundary cell reads its missing bits and its own pre-streaming scalar populations
        const unsigned id = ids[k];
        const unsigned kind = kind_of(a, id);
        const unsigned cell = r.cell_in_plane + (unsigned)k;
        const unsigned m = ld(a.miss + xplane, opaque(cell * 4u));
        const T* val = opaque(a.bc_values + id * 27u);
        if (kind == K_EQ) {
          static_for<Q>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            f[k][l] = val[l];
          });
        } else if (kind == K_HW) {
          T own[Q];
          load_own_cell<L, true>(a.src, a.plane_stride, xplane, cell, own);
          static_for<Q>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            const T pre = own[l] + val[l];
            if ((m >> l) & 1u) f[k][l] = pre;
          });
        } else if (kind == K_DN) {
          load_own_cell<L, false>(a.src, a.plane_stride, xplane, cell, f[k]);
        } else if (kind == K_FW) {
          fullway = true;
        } else if (kind == XLBHIP_BC_EXTRAPOLATION_OUTFLOW) {
          // last step's auxiliary data; the new ones are assembled by k_outflow_aux after this kernel
          T own[Q];
          load_own_cell<L, true>(a.src, a.plane_stride, xplane, cell, own);
          static_for<Q>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            if ((m >> l) & 1u) f[k][l] = own[l];
          });
        } else if (bc_is_zouhe_family(kind)) {
          T uw[5] = {val[0], val[1], val[2], val[3], val[4]};  // constant prescribed values only
          zouhe_apply<L, T>(kind, f[k], m, uw);
        }
        // the scalar's rule of this BC
        T pre[QS];
        load_own_cell<L, false>(sa.gsrc, sa.g_plane_stride, xplane, cell, pre);
        scalar_apply_rule<L, T>(opaque(sa.sc_rule)[id], opaque(sa.sc_value)[id], m, pre, g[k]);
      }
    }
    scalar_collide_cell<L, T, COLL>(f[k], g[k], fullway, a.omega, sa.omega_s, a.extra, sa.cp);
  }

  // ---- store both fields ----
  store_planes<true, VEC, Q>(a.dst, a.plane_stride, xplane, r.cell_in_plane, f[0]);
  store_planes<true, VEC, QS>(sa.gdst, sa.g_plane_stride, xplane, r.cell_in_plane, g[0]);
}

}  // namespace xlb
