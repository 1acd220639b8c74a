// Single-component Shan-Chen pseudopotential flow (liquid-vapour): the cell-level rules.
//
// One step on the post-streaming populations f of cell x (after the streaming-step boundary rules, cell.hpp):
//   rho, u     = moments<L, T>(f)
//   psi(x)     = Psi(rho)                                      (a wall cell — fullway bounce-back or solid id 255 — carries Psi(rho_w))
//   S_a        = sum_{i = 1 .. Q-1, ascending} (w_i psi_i) c_{a,i}
//   F_a        = (-G psi(x)) S_a                               (zero at a wall cell)
//   delta_u_a  = force_vector_a + F_a / rho                    -> collide<L, T, BGK | COLL_FORCED> (exact-difference forcing)
// psi_i is the pseudopotential of the neighbour at x + c_i: the wall value Psi(rho_w) of the cell's own bc id where bit opp(i) of the
// cell's missing mask is set (population opp(i) would arrive from there: the neighbour is a wall), else psi[x + c_i], periodic.  The
// weights are the fluid lattice's own; sum_i w_i c c = cs^2 I gives the bulk pressure p = cs^2 rho + (G cs^2 / 2) psi^2 on all three.
// (Shan and Chen 1993; Kupershtokh's exact-difference forcing; Carnahan-Starling form after Yuan and Schaefer 2006.)
//
// Everything here compiles for the host too (tests/multiphase_cpu_emulation.cpp); the row kernels, which need the addressing of
// step_kernel.hpp, are in multiphase_step_kernel.hpp.  tests/_multiphase_ref.py restates the step in NumPy, operation for operation.
#pragma once
#include "ops_kernels.hpp"

namespace xlb {

// the forms of Psi(rho); par[] as xlbhip_multiphase_set_model takes them
enum { PSI_EXPONENTIAL = 0, PSI_DENSITY = 1, PSI_CARNAHAN_STARLING = 2 };
constexpr unsigned BC_ID_SOLID = 255u;  // cell_type.py: solid voxels of a mesh masker

template <class T>
struct PsiModel {
  int form;
  T neg_g;     // -G
  T par[4];    // exponential: rho0; Carnahan-Starling: T, a, b, R
  T force[3];  // force_vector, internal 3-component form
};

template <class T>
__device__ __forceinline__ T psi_exp(T x) {
  if constexpr (sizeof(T) == 4)
    return expf(x);
  else
    return exp(x);
}

// Psi(rho).  The exponential form is the only one with a transcendental; the others are sums, products, IEEE divisions and one
// IEEE square root, so their bits are those of the NumPy restatement.
template <class T>
__device__ __forceinline__ T psi_of(const PsiModel<T>& mo, T rho) {
  if (mo.form == PSI_DENSITY) return rho;
  if (mo.form == PSI_EXPONENTIAL) {
    const T rho0 = mo.par[0];
    return rho0 * (T(1) - psi_exp<T>(-(rho / rho0)));
  }
  // Carnahan-Starling: p = rho R T (1 + eta + eta^2 - eta^3) / (1 - eta)^3 - a rho^2, eta = b rho / 4;
  // psi = sqrt(2 (p - cs2 rho) / (G cs2)) with G = -1
  const T temp = mo.par[0], a = mo.par[1], b = mo.par[2], R = mo.par[3];
  const T eta = (b * rho) / T(4);
  const T e2 = eta * eta;
  const T e3 = e2 * eta;
  const T num = ((T(1) + eta) + e2) - e3;
  const T om = T(1) - eta;
  const T den = (om * om) * om;
  const T p = (((rho * R) * temp) * num) / den - (a * rho) * rho;
  const T cs2 = T(1.0 / 3.0);
  const T arg = (T(2) * (p - cs2 * rho)) / (T(-1) * cs2);
  return sqrt(arg);
}

// S_a += / -= (w_i psi_i) by the sign of c_{a,i}; called for i = 1 .. Q-1 in ascending order
template <class L, class T, int i>
__device__ __forceinline__ void psi_force_add(T psi_i, T (&s)[3]) {
  const T t = T(L::w(i)) * psi_i;
  static_for<3>([&](auto ac) {
    constexpr int a = decltype(ac)::value;
    if constexpr (L::c(a, i) == 1) s[a] = s[a] + t;
    if constexpr (L::c(a, i) == -1) s[a] = s[a] - t;
  });
}

// is the neighbour at x + c_i a wall?  m: the cell's missing bits (0 at a cell without a bc id)
template <class L, int i>
__device__ __forceinline__ bool psi_neighbour_is_wall(unsigned m) {
  return ((m >> opp<L>(i)) & 1u) != 0u;
}

// F = (-G psi) S from the neighbours' values nb[i] (nb[0] unused) — zero at a wall cell
template <class L, class T>
__device__ __forceinline__ void psi_force(const PsiModel<T>& mo, T psi, const T (&nb)[L::Q], unsigned m, T psi_wall, bool wall_cell, T (&F)[3]) {
  T s[3] = {T(0), T(0), T(0)};
  static_for<L::Q - 1>([&](auto ic) {
    constexpr int i = decltype(ic)::value + 1;
    psi_force_add<L, T, i>(psi_neighbour_is_wall<L, i>(m) ? psi_wall : nb[i], s);
  });
  const T gp = mo.neg_g * psi;
  static_for<3>([&](auto ac) {
    constexpr int a = decltype(ac)::value;
    F[a] = wall_cell ? T(0) : gp * s[a];
  });
}

// One cell after streaming and the streaming-step rules: the forced BGK collision, or the fullway bounce
template <class L, class T>
__device__ __forceinline__ void multiphase_collide_cell(T (&f)[L::Q], bool fullway, T omega, T rho, const T (&F)[3], const PsiModel<T>& mo) {
  if (!fullway) {
    CollideExtra ex;
    ex.smag_cs = 0.0;
    static_for<3>([&](auto ac) {
      constexpr int a = decltype(ac)::value;
      ex.force[a] = (double)(mo.force[a] + F[a] / rho);
    });
    collide<L, T, XLBHIP_BGK | COLL_FORCED>(f, omega, ex);
  } else {
    static_for<L::Q>([&](auto lc) {
      constexpr int l = decltype(lc)::value;
      constexpr int o = xlb::opp<L>(l);
      if constexpr (l < o) {
        const T t = f[l];
        f[l] = f[o];
        f[o] = t;
      }
    });
  }
}

// the physical velocity of the exact-difference scheme: u_bare + F / (2 rho)
template <class T>
__device__ __forceinline__ T multiphase_velocity(T u_bare, T F, T rho) {
  return u_bare + F / (T(2) * rho);
}

}  // namespace xlb
