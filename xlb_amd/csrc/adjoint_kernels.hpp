// Discrete adjoint of the fused BGK step: the cell-level transposed rules and the small whole-field kernels.
//
// One forward step is f_{n+1} = S(f_n; omega): pull streaming, the streaming-step boundary rules (cell.hpp: apply_streaming_bc), BGK,
// the fullway bounce.  With f* the post-streaming, post-BC populations of a cell and lam = dL/df_{n+1} at that cell, the transposes are
//
//   collision   mu_j = (1 - omega) lam_j + omega (A + sum_d (B_d / rho) (c_dj - u_d))
//               A   = sum_k lam_k w_k e_k,                 e_k = (1 + cu_k (1 + cu_k / 2)) - usqr,  cu_k = 3 (c_k . u)
//               B_d = sum_k lam_k rho w_k (3 c_dk (1 + cu_k) - 3 u_d)
//               dL/domega += sum_k lam_k (feq_k - f*_k)
//   fullway     mu_[opp l] = lam_l, nothing goes through the collision and nothing into dL/domega
//   equilibrium mu = 0 (f* does not depend on f_n); the cell still collides, so its dL/domega term counts
//   halfway     mu_l of a missing direction l goes to lam_n[opp l] of the SAME cell and is not streamed (the wall-velocity term is
//               a constant and drops out)
//   do-nothing  mu_l goes to lam_n[l] of the same cell, nothing is streamed
//   streaming   lam_n[l](y) += mu_l(y + c_l), periodic, for every mu_l the rules above did not redirect
//
// The Jacobian is that of the exact-arithmetic map: casts between store and compute dtype count as the identity.
//
// ORDER OF EVERY SUM (fixed; tests/_adjoint_ref.py restates it operation for operation and the library is built with
// -ffp-contract=off): A, B_d and the omega term run over k = 0 .. q-1 in one pass, the k = 0 term starts each sum, and for every k
// the terms are formed as  lam_k (w_k e_k),  lam_k ((rho w_k) g_dk)  with d ascending and g_dk = s_k - 3 u_d | (-s_k) - 3 u_d |
// -(3 u_d) for c_dk = 1 | -1 | 0, s_k = 3 (1 + cu_k),  and  lam_k (feq_k - f*_k).  Then Br_d = B_d / rho and
// mu_j = (1 - omega) lam_j + omega acc_j, acc_j = A, then acc_j += Br_d (c_dj - u_d) with d ascending and c_dj - u_d written as
// 1 - u_d | -1 - u_d | -u_d.  lam_n[l] = (gathered mu_l) + (the cell's own redirected mu).  rho, u, usqr, cu_k and feq_k are
// cell.hpp's (moments, usqr_of, feq_dir).
//
// Everything here compiles for the host too (tests/adjoint_cpu_emulation.cpp); the fused kernel, which needs the addressing of
// step_kernel.hpp, is in adjoint_step_kernel.hpp and calls the functions below for every cell.
#pragma once
#include "ops_kernels.hpp"

namespace xlb {

// c_dj - u_d for the internal axis a of direction j
template <class L, class T, int a, int j>
__device__ __forceinline__ T adjoint_c_minus_u(const T (&u)[3]) {
  if constexpr (L::c(a, j) == 1)
    return T(1.0) - u[a];
  else if constexpr (L::c(a, j) == -1)
    return T(-1.0) - u[a];
  else
    return -u[a];
}

// Transpose of the BGK collision at one cell: lam (dL/d post-collision) -> mu (dL/df*) IN PLACE; returns the cell's omega term
// sum_k lam_k (feq_k - f*_k).  fs: the post-streaming, post-BC populations.
template <class L, class T>
__device__ __forceinline__ T adjoint_collide(const T (&fs)[L::Q], T (&lam)[L::Q], T omega) {
  constexpr int Q = L::Q, A0 = 3 - L::D;
  T rho, u[3];
  moments<L, T>(fs, rho, u);
  const T usqr = usqr_of<L, T>(u);
  T tu[3] = {T(0), T(0), T(0)};
  static_for<L::D>([&](auto dc) {
    constexpr int a = decltype(dc)::value + A0;
    tu[a] = T(3.0) * u[a];
  });
  T A = T(0), B[3] = {T(0), T(0), T(0)}, term = T(0);
  static_for<Q>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    T dot = T(0);
    static_for<3>([&](auto ac) {
      constexpr int a = decltype(ac)::value;
      constexpr int cl = L::c(a, k);
      if constexpr (a >= A0) {
        if constexpr (cl == 1) dot = dot + u[a];
        if constexpr (cl == -1) dot = dot - u[a];
      }
    });
    const T cu = T(3.0) * dot;
    const T w = T(L::w(k));
    const T e = (T(1.0) + cu * (T(1.0) + T(0.5) * cu)) - usqr;
    const T ta = lam[k] * (w * e);
    const T s = T(3.0) * (T(1.0) + cu);
    const T rw = rho * w;
    if constexpr (k == 0)
      A = ta;
    else
      A = A + ta;
    static_for<L::D>([&](auto dc) {
      constexpr int a = decltype(dc)::value + A0;
      constexpr int cl = L::c(a, k);
      T g;
      if constexpr (cl == 1)
        g = s - tu[a];
      else if constexpr (cl == -1)
        g = (-s) - tu[a];
      else
        g = -tu[a];
      const T tb = lam[k] * (rw * g);
      if constexpr (k == 0)
        B[a] = tb;
      else
        B[a] = B[a] + tb;
    });
    const T tt = lam[k] * (feq_dir<L, T, k>(rho, u, usqr) - fs[k]);
    if constexpr (k == 0)
      term = tt;
    else
      term = term + tt;
  });
  T Br[3] = {T(0), T(0), T(0)};
  static_for<L::D>([&](auto dc) {
    constexpr int a = decltype(dc)::value + A0;
    Br[a] = B[a] / rho;
  });
  const T om1 = T(1.0) - omega;
  static_for<Q>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    T acc = A;
    static_for<L::D>([&](auto dc) {
      constexpr int a = decltype(dc)::value + A0;
      acc = acc + Br[a] * adjoint_c_minus_u<L, T, a, j>(u);
    });
    lam[j] = om1 * lam[j] + omega * acc;
  });
  return term;
}

// FullwayBounceBackBC: f_{n+1}[l] = f*[opp l]  =>  mu_[opp l] = lam_l, in place
template <class L, class T>
__device__ __forceinline__ void adjoint_fullway(T (&lam)[L::Q]) {
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    constexpr int o = opp<L>(l);
    if constexpr (l < o) {
      const T t = lam[l];
      lam[l] = lam[o];
      lam[o] = t;
    }
  });
}

// EquilibriumBC: f* is a constant, mu = 0
template <class L, class T>
__device__ __forceinline__ void adjoint_equilibrium(T (&mu)[L::Q]) {
  static_for<L::Q>([&](auto lc) { mu[decltype(lc)::value] = T(0); });
}

// HalfwayBounceBackBC: f*[l] = f_n[opp l] of the same cell where l is missing  =>  lam_n[opp l] += mu_l, i.e. lam_n[l] += mu_[opp l]
// where opp l is missing
template <class L, class T>
__device__ __forceinline__ void adjoint_halfway_own(unsigned m, const T (&mu_own)[L::Q], T (&lam_n)[L::Q]) {
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    constexpr int o = opp<L>(l);
    if ((m >> o) & 1u) lam_n[l] = lam_n[l] + mu_own[o];
  });
}

// DoNothingBC: f*[l] = f_n[l] of the same cell  =>  lam_n[l] += mu_l
template <class L, class T>
__device__ __forceinline__ void adjoint_do_nothing_own(const T (&mu_own)[L::Q], T (&lam_n)[L::Q]) {
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    lam_n[l] = lam_n[l] + mu_own[l];
  });
}

// Directions l whose forward pull at a cell of this kind was replaced by a rule: their mu_l is NOT streamed to the neighbour
__device__ __forceinline__ unsigned adjoint_pull_blocked(unsigned kind, unsigned m) {
  if (kind == XLBHIP_BC_EQUILIBRIUM || kind == XLBHIP_BC_DO_NOTHING) return ~0u;
  if (kind == XLBHIP_BC_HALFWAY_BB) return m;
  return 0u;
}

// The local transpose of one cell of boundary kind `kind` (0: none): lam -> mu in place, returns the omega term
template <class L, class T>
__device__ __forceinline__ T adjoint_local_cell(unsigned kind, const T (&fs)[L::Q], T (&lam)[L::Q], T omega) {
  if (kind == XLBHIP_BC_FULLWAY_BB) {
    adjoint_fullway<L, T>(lam);
    return T(0);
  }
  const T term = adjoint_collide<L, T>(fs, lam, omega);
  if (kind == XLBHIP_BC_EQUILIBRIUM) adjoint_equilibrium<L, T>(lam);
  return term;
}

// The own-cell part of the transposed streaming: lam_n (holding the gathered part) += the cell's own redirected mu
template <class L, class T>
__device__ __forceinline__ void adjoint_own_terms(unsigned kind, unsigned m, const T (&mu_own)[L::Q], T (&lam_n)[L::Q]) {
  if (kind == XLBHIP_BC_HALFWAY_BB)
    adjoint_halfway_own<L, T>(m, mu_own, lam_n);
  else if (kind == XLBHIP_BC_DO_NOTHING)
    adjoint_do_nothing_own<L, T>(mu_own, lam_n);
}

// ---- whole-field kernels (one thread per cell) --------------------------------------------------------------------------------

// The gather mask of the transposed streaming, built once per pair of masks: bit l of gmask(y) is set where the cell y + c_l
// (periodic) replaced its pull of l, so that y must not gather mu_l from it.  The fused kernel reads this one word per cell instead
// of the bc id (and missing bits) of its q neighbours.  Fields without ghost planes.
template <class L>
__global__ void k_adjoint_gather_mask(const uint8_t* bc, const uint32_t* miss, const uint8_t* kind /*[256]*/, uint32_t* gmask, Dims d) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  unsigned g = 0u;
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    const size_t n = ((size_t)wrap(x + L::c(0, l), d.nx) * d.ny + wrap(y + L::c(1, l), d.ny)) * d.nz + wrap(z + L::c(2, l), d.nz);
    const unsigned idn = bc[n];
    if (idn != 0u && ((adjoint_pull_blocked(kind[idn], miss[n]) >> l) & 1u)) g |= 1u << l;
  });
  gmask[((size_t)x * d.ny + y) * d.nz + z] = g;
}

// MacroscopicAdjoint()(f, rho_bar, u_bar, lam): the transpose of Macroscopic at f applied to (dL/drho, dL/du):
// lam_l = rho_bar + sum_d (u_bar_d / rho) (c_dl - u_d), the sum started at rho_bar, d ascending.  rho_bar / u_bar without data: zero.
template <class L, class T>
__global__ void k_macroscopic_adjoint(FieldView f, FieldView rho_bar, FieldView u_bar, FieldView lam, Dims d) {
  constexpr int A0 = 3 - L::D;
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  T ff[L::Q];
  const size_t i = cell_index(f, d, x, y, z);
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    ff[l] = load_rt<T>(f, (size_t)l * f.plane_stride + i);
  });
  T rho, u[3];
  moments<L, T>(ff, rho, u);
  const T rb = rho_bar.data ? load_rt<T>(rho_bar, cell_index(rho_bar, d, x, y, z)) : T(0);
  T ur[3] = {T(0), T(0), T(0)};
  static_for<L::D>([&](auto dc) {
    constexpr int a = decltype(dc)::value;
    const T ub = u_bar.data ? load_rt<T>(u_bar, (size_t)a * u_bar.plane_stride + cell_index(u_bar, d, x, y, z)) : T(0);
    ur[a + A0] = ub / rho;
  });
  const size_t o = cell_index(lam, d, x, y, z);
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    T acc = rb;
    static_for<L::D>([&](auto dc) {
      constexpr int a = decltype(dc)::value + A0;
      acc = acc + ur[a] * adjoint_c_minus_u<L, T, a, l>(u);
    });
    store_rt<T>(lam, (size_t)l * lam.plane_stride + o, acc);
  });
}

}  // namespace xlb
