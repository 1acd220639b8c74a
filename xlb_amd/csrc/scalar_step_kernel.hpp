// The coupled fluid + scalar step: ONE kernel pulls and stores both fields (q + 2 d + 1 populations per cell each way; D3Q19 fp32:
// 208 B per cell against the fluid step's 152 B), because the scalar's collision needs the velocity the fluid step holds in registers
// and the fluid's force needs the scalar sum before it collides — a second pass would re-read the fluid field for either.
//
// Addressing, lane mapping, row-end handling and the rare boundary path are those of k_step (step_kernel.hpp), whose rule functions
// (cell.hpp) it calls; the scalar's own rules are in scalar_kernels.hpp.  k_step itself is untouched.
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

// one direction's pull of a thread's VEC cells: aligned for c_z == 0, shifted by one element otherwise (k_step's scheme)
template <class S, int VEC, int cz>
__device__ __forceinline__ void pull_dir(const S* row, unsigned yb, unsigned zb, int z0, int nz, bool at_z_lo, bool at_z_hi, S (&v)[VEC]) {
  constexpr unsigned ES = sizeof(S);
  if constexpr (cz == 0) {
    ld_aligned<S, VEC, false>(row, yb + zb, v);
  } else if constexpr (VEC == 1) {
    int zs = z0 - cz;
    zs = zs < 0 ? nz - 1 : (zs == nz ? 0 : zs);
    v[0] = ld(row, yb + (unsigned)zs * ES);
  } else if constexpr (cz == 1) {
    S t[VEC];
    ld_shifted<S, VEC>(row, yb + zb - (at_z_lo ? 0u : ES), t);
    S wrapv = t[0];
    if (at_z_lo) wrapv = ld(row, yb + (unsigned)(nz - 1) * ES);
    v[0] = at_z_lo ? wrapv : t[0];
#pragma unroll
    for (int k = 1; k < VEC; ++k) v[k] = at_z_lo ? t[k - 1] : t[k];
  } else {
    S t[VEC];
    ld_shifted<S, VEC>(row, yb + zb + (at_z_hi ? 0u : ES), t);
    S wrapv = t[VEC - 1];
    if (at_z_hi) wrapv = ld(row, yb);
#pragma unroll
    for (int k = 0; k < VEC - 1; ++k) v[k] = at_z_hi ? t[k + 1] : t[k];
    v[VEC - 1] = at_z_hi ? wrapv : t[VEC - 1];
  }
}

// HASBC: 0 = no boundary conditions, 2 = every kind the coupled step supports (equilibrium, halfway, fullway, do-nothing, Zou-He /
// Regularized with constant values, extrapolation outflow).  Stores are non-temporal.
template <class L, class T, class S, int VEC, int COLL, int HASBC>
__global__ void __launch_bounds__(256) k_step_scalar(const ScalarStepArgs<T, S> sa) {
  typedef ScalarSet<L> G;
  constexpr int Q = L::Q, QS = G::Q;
  constexpr unsigned ES = sizeof(S);
  const StepArgs<T, S>& a = sa.f;
  const int zq = blockIdx.x * blockDim.x + threadIdx.x;
  const int y = blockIdx.y * blockDim.y + threadIdx.y;
  if (zq >= a.nzq || y >= a.ny) return;
  const int x = a.x_begin + blockIdx.z;  // block-uniform
  const int z0 = zq * VEC;
  const int ny = a.ny, nz = a.nz;

  int Xs[3];
  Xs[0] = (x + 1 == a.nx) ? 0 : x + 1;
  Xs[1] = x;
  Xs[2] = (x == 0) ? a.nx - 1 : x - 1;
  const size_t plane_cells = (size_t)ny * nz;
  unsigned Yb[3];
  Yb[0] = (unsigned)((y + 1 == ny) ? 0 : y + 1) * (unsigned)nz * ES;
  Yb[1] = (unsigned)y * (unsigned)nz * ES;
  Yb[2] = (unsigned)((y == 0) ? ny - 1 : y - 1) * (unsigned)nz * ES;

  const bool at_z_lo = (z0 == 0);
  const bool at_z_hi = (z0 + VEC == nz);
  const unsigned zb = (unsigned)z0 * ES;

  T f[VEC][Q];
  T g[VEC][QS];

  // ---- pull streaming of both fields ----
  static_for<Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    constexpr int cx = L::c(0, l), cy = L::c(1, l), cz = L::c(2, l);
    const S* row = a.src + (size_t)l * a.plane_stride + (size_t)Xs[cx + 1] * plane_cells;  // uniform
    S v[VEC];
    pull_dir<S, VEC, cz>(row, Yb[cy + 1], zb, z0, nz, at_z_lo, at_z_hi, v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) f[k][l] = to_compute<T, S>(v[k]);
  });
  static_for<QS>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    constexpr int l = G::dir(j);
    constexpr int cx = L::c(0, l), cy = L::c(1, l), cz = L::c(2, l);
    const S* row = sa.gsrc + (size_t)j * sa.g_plane_stride + (size_t)Xs[cx + 1] * plane_cells;  // uniform
    S v[VEC];
    pull_dir<S, VEC, cz>(row, Yb[cy + 1], zb, z0, nz, at_z_lo, at_z_hi, v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) g[k][j] = to_compute<T, S>(v[k]);
  });

  // ---- boundary ids of my VEC cells ----
  const unsigned cell_in_plane = (unsigned)y * (unsigned)nz + (unsigned)z0;  // elements, < 2^30
  unsigned ids[VEC];
  bool any_bc = false;
  if constexpr (HASBC != 0) {
    const uint8_t* bcp = a.bc + (size_t)Xs[1] * plane_cells;  // uniform
    if constexpr (VEC == 4) {
      const unsigned wrd = ld(reinterpret_cast<const unsigned*>(bcp), cell_in_plane);
      any_bc = wrd != 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) ids[k] = (wrd >> (8 * k)) & 0xffu;
    } else if constexpr (VEC == 2) {
      const unsigned wrd = ld(reinterpret_cast<const unsigned short*>(bcp), cell_in_plane);
      any_bc = wrd != 0u;
      ids[0] = wrd & 0xffu;
      ids[1] = (wrd >> 8) & 0xffu;
    } else {
      ids[0] = ld(bcp, cell_in_plane);
      any_bc = ids[0] != 0u;
    }
  }

#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    bool fullway = false;
    if constexpr (HASBC != 0) {
      if (any_bc && ids[k] != 0u) {
        // rare path: every boundary cell reads its missing bits and its own pre-streaming scalar populations
        const unsigned id = ids[k];
        const unsigned kind = kind_of(a, id);
        const unsigned cb = opaque((cell_in_plane + (unsigned)k) * ES);  // own cell, byte offset in the x-plane
        const unsigned m = ld(a.miss + (size_t)Xs[1] * plane_cells, opaque((cell_in_plane + (unsigned)k) * 4u));
        const T* val = opaque(a.bc_values + id * 27u);
        if (kind == K_EQ) {
          static_for<Q>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            f[k][l] = val[l];
          });
        } else if (kind == K_HW) {
          static_for<Q>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            const S* own = a.src + (size_t)opp<L>(l) * a.plane_stride + (size_t)Xs[1] * plane_cells;  // uniform
            const T pre = to_compute<T, S>(ld(own, cb)) + val[l];
            if ((m >> l) & 1u) f[k][l] = pre;
          });
        } else if (kind == K_DN) {
          static_for<Q>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            const S* own = a.src + (size_t)l * a.plane_stride + (size_t)Xs[1] * plane_cells;
            f[k][l] = to_compute<T, S>(ld(own, cb));
          });
        } else if (kind == K_FW) {
          fullway = true;
        } else if (kind == XLBHIP_BC_EXTRAPOLATION_OUTFLOW) {
          // last step's auxiliary data; the new ones are assembled by k_outflow_aux after this kernel
          static_for<Q>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            const S* own = a.src + (size_t)opp<L>(l) * a.plane_stride + (size_t)Xs[1] * plane_cells;  // uniform
            if ((m >> l) & 1u) f[k][l] = to_compute<T, S>(ld(own, cb));
          });
        } else if (bc_is_zouhe_family(kind)) {
          T uw[5] = {val[0], val[1], val[2], val[3], val[4]};  // constant prescribed values only
          zouhe_apply<L, T>(kind, f[k], m, uw);
        }
        // the scalar's rule of this BC
        T pre[QS];
        static_for<QS>([&](auto jc) {
          constexpr int j = decltype(jc)::value;
          const S* own = sa.gsrc + (size_t)j * sa.g_plane_stride + (size_t)Xs[1] * plane_cells;  // uniform
          pre[j] = to_compute<T, S>(ld(own, cb));
        });
        scalar_apply_rule<L, T>(opaque(sa.sc_rule)[id], opaque(sa.sc_value)[id], m, pre, g[k]);
      }
    }
    scalar_collide_cell<L, T, COLL>(f[k], g[k], fullway, a.omega, sa.omega_s, a.extra, sa.cp);
  }

  // ---- store both fields ----
  static_for<Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    S* drow = a.dst + (size_t)l * a.plane_stride + (size_t)Xs[1] * plane_cells;  // uniform
    S v[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = to_store<S, T>(f[k][l]);
    st_aligned<S, VEC, true>(drow, Yb[1] + zb, v);
  });
  static_for<QS>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    S* drow = sa.gdst + (size_t)j * sa.g_plane_stride + (size_t)Xs[1] * plane_cells;  // uniform
    S v[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = to_store<S, T>(g[k][j]);
    st_aligned<S, VEC, true>(drow, Yb[1] + zb, v);
  });
}

}  // namespace xlb
