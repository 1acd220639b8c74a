// The porous BGK step and its discrete adjoint: the cell-level rules.  Geometry is a continuous per-cell field, the solidity alpha(x)
// in [0, 1] (0: fluid, 1: the cell relaxes towards rest; after Pingen, Evgrafov and Maute 2007).  The step is the fused BGK step with
// the equilibrium taken at the damped velocity:
//
//   rho, u  = moments(f*)                         (cell.hpp)
//   kappa   = 1 - alpha
//   ut_d    = kappa u_d
//   f_out_l = f*_l - omega (f*_l - feq_l(rho, ut))
//
// Mass is conserved, momentum leaves at the rate omega alpha rho u per step.  alpha == 0 gives kappa == 1 and ut == u exactly: the
// plain BGK step bit for bit.  Values of alpha outside [0, 1] are the caller's business; nothing here checks them.
//
// With lam = dL/df_out at a cell that collides, the transpose is adjoint_collide's (adjoint_kernels.hpp) with its sums taken at ut:
//
//   A    = sum_k lam_k w_k e_k,                 e_k = (1 + cu_k (1 + cu_k / 2)) - usqr(ut),  cu_k = 3 (c_k . ut)
//   B_d  = sum_k lam_k rho w_k (3 c_dk (1 + cu_k) - 3 ut_d)
//   mu_j = (1 - omega) lam_j + omega (A + sum_d (kappa B_d / rho) (c_dj - u_d))        (u, not ut: d ut_d / d f_j = kappa (c_dj - u_d) / rho)
//   dL/domega += sum_k lam_k (feq_k(rho, ut) - f*_k)
//   dL/dalpha += -omega sum_d B_d u_d                                                     (d ut_d / d alpha = -u_d)
//
// Fullway cells do not collide: nothing into dL/domega and 0 into dL/dalpha.  Equilibrium, halfway and do-nothing cells collide and
// their terms count.  The streaming and boundary transposes are adjoint_kernels.hpp's, unchanged.
//
// ORDER OF EVERY OPERATION (fixed; tests/_porous_ref.py restates it operation for operation and the library is built with
// -ffp-contract=off): kappa = 1 - alpha; ut_d = kappa u_d; usqr = usqr_of(ut); feq_k = feq_dir(rho, ut, usqr).  A, B_d and the omega
// term run over k = 0 .. q-1 in one pass, the k = 0 term starts each sum, and for every k the terms are  lam_k (w_k e_k),
// lam_k ((rho w_k) g_dk)  with d ascending and g_dk = s_k - 3 ut_d | (-s_k) - 3 ut_d | -(3 ut_d) for c_dk = 1 | -1 | 0,
// s_k = 3 (1 + cu_k),  and  lam_k (feq_k - f*_k).  Then Br_d = (kappa B_d) / rho and mu_j = (1 - omega) lam_j + omega acc_j,
// acc_j = A, then acc_j += Br_d (c_dj - u_d) with d ascending and c_dj - u_d written as 1 - u_d | -1 - u_d | -u_d.  The alpha term is
// -(omega s), s = B_d u_d with d ascending, the first product starts the sum.
//
// KEEP IN STEP WITH adjoint_kernels.hpp: porous_adjoint_collide restates adjoint_collide with ut in the sums and kappa in Br_d; a change
// to the order of an operation there has to be made here (and in both restatements).
//
// Everything here compiles for the host too (tests/porous_cpu_emulation.cpp); the fused kernels are in porous_step_kernel.hpp.
#pragma once
#include "adjoint_kernels.hpp"

namespace xlb {

// ut = (1 - alpha) u; returns kappa
template <class L, class T>
__device__ __forceinline__ T porous_damped_velocity(const T (&u)[3], T alpha, T (&ut)[3]) {
  const T kappa = T(1.0) - alpha;
  static_for<3>([&](auto ac) {
    constexpr int a = decltype(ac)::value;
    if constexpr (a >= 3 - L::D)
      ut[a] = kappa * u[a];
    else
      ut[a] = T(0);
  });
  return kappa;
}

// The porous BGK collision at one cell, in place on the post-streaming, post-BC populations
template <class L, class T>
__device__ __forceinline__ void porous_collide(T (&f)[L::Q], T omega, T alpha) {
  T rho, u[3], ut[3];
  moments<L, T>(f, rho, u);
  porous_damped_velocity<L, T>(u, alpha, ut);
  const T usqr = usqr_of<L, T>(ut);
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    const T fneq = f[l] - feq_dir<L, T, l>(rho, ut, usqr);
    f[l] = f[l] - omega * fneq;
  });
}

// the two scalar terms a colliding cell adds to the gradients
template <class T>
struct PorousTerms {
  T omega;  // sum_k lam_k (feq_k(rho, ut) - f*_k)
  T alpha;  // -omega sum_d B_d u_d
};

// Transpose of the porous collision at one cell: lam (dL/d post-collision) -> mu (dL/df*) IN PLACE.  fs: the post-streaming, post-BC
// populations.
template <class L, class T>
__device__ __forceinline__ PorousTerms<T> porous_adjoint_collide(const T (&fs)[L::Q], T (&lam)[L::Q], T omega, T alpha) {
  constexpr int Q = L::Q, A0 = 3 - L::D;
  T rho, u[3], ut[3];
  moments<L, T>(fs, rho, u);
  const T kappa = porous_damped_velocity<L, T>(u, alpha, ut);
  const T usqr = usqr_of<L, T>(ut);
  T tu[3] = {T(0), T(0), T(0)};
  static_for<L::D>([&](auto dc) {
    constexpr int a = decltype(dc)::value + A0;
    tu[a] = T(3.0) * ut[a];
  });
  T A = T(0), B[3] = {T(0), T(0), T(0)}, term = T(0);
  static_for<Q>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    T dot = T(0);
    static_for<3>([&](auto ac) {
      constexpr int a = decltype(ac)::value;
      constexpr int cl = L::c(a, k);
      if constexpr (a >= A0) {
        if constexpr (cl == 1) dot = dot + ut[a];
        if constexpr (cl == -1) dot = dot - ut[a];
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
    const T tt = lam[k] * (feq_dir<L, T, k>(rho, ut, usqr) - fs[k]);
    if constexpr (k == 0)
      term = tt;
    else
      term = term + tt;
  });
  T Br[3] = {T(0), T(0), T(0)};
  T bu = T(0);
  static_for<L::D>([&](auto dc) {
    constexpr int a = decltype(dc)::value + A0;
    Br[a] = (kappa * B[a]) / rho;
    const T p = B[a] * u[a];
    if constexpr (a == A0)
      bu = p;
    else
      bu = bu + p;
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
  return {term, -(omega * bu)};
}

// The local transpose of one cell of boundary kind `kind` (0: none): lam -> mu in place, returns the omega and the alpha term
template <class L, class T>
__device__ __forceinline__ PorousTerms<T> porous_adjoint_local_cell(unsigned kind, const T (&fs)[L::Q], T (&lam)[L::Q], T omega, T alpha) {
  if (kind == XLBHIP_BC_FULLWAY_BB) {
    adjoint_fullway<L, T>(lam);
    return {T(0), T(0)};
  }
  const PorousTerms<T> terms = porous_adjoint_collide<L, T>(fs, lam, omega, alpha);
  if (kind == XLBHIP_BC_EQUILIBRIUM) adjoint_equilibrium<L, T>(lam);
  return terms;
}

}  // namespace xlb
