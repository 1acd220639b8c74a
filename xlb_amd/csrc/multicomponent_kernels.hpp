// Two-component Shan-Chen flow (two immiscible fluids A and B on one lattice): the cell-level rules.
//
// One step on the post-streaming populations f^A, f^B of cell x (after the streaming-step boundary rules, per component, cell.hpp):
//   rho_s, u_s = moments<L, T>(f^s)                                               s in {A, B}
//   psi_s(x)   = rho_s                              (a wall cell — fullway bounce-back or solid id 255 — carries the wall density rho_w,s)
//   u'_a       = ((omega_A rho_A) u_A,a + (omega_B rho_B) u_B,a) / ((omega_A rho_A) + (omega_B rho_B))
//   S^s_a      = sum_{i = 1 .. Q-1, ascending} (w_i psi_s,i) c_{a,i}                                (psi_force_add of multiphase_kernels.hpp)
//   F^A_a      = (-psi_A) ((G_AA S^A_a) + (G_AB S^B_a))                                             (both zero at a wall cell)
//   F^B_a      = (-psi_B) ((G_AB S^A_a) + (G_BB S^B_a))
//   f^s_l     <- (f^s_l - omega_s (f^s_l - feq_l(rho_s, u'))) + (feq_l(rho_s, u' + (g + F^s / rho_s)) - feq_l(rho_s, u'))
// psi_s,i is the density of component s at x + c_i: the wall density rho_w,s of the cell's own bc id where bit opp(i) of the cell's
// missing mask is set, else the neighbour's value, periodic.  The weights are the lattice's own, so the bulk pressure is
// cs^2 (rho_A + rho_B) + cs^2 (G_AA rho_A^2 / 2 + G_AB rho_A rho_B + G_BB rho_B^2 / 2) on all three lattices.  The collision without the
// force conserves the total momentum by the definition of u'; the force adds F^A + F^B.  The physical (barycentric) velocity is
//   u_a = ((rho_A u_A,a + rho_B u_B,a) + (F^A_a + F^B_a) / 2) / (rho_A + rho_B).
// (Shan and Chen 1993; Shan and Doolen 1995; walls after Martys and Chen 1996; the exact-difference forcing of the other steppers.)
//
// Everything here compiles for the host too (tests/multicomponent_cpu_emulation.cpp); the row kernels are in
// multicomponent_step_kernel.hpp.  tests/_multicomponent_ref.py restates the step in NumPy, operation for operation.
#pragma once
#include "multiphase_kernels.hpp"

namespace xlb {

template <class T>
struct MixModel {
  T g_aa, g_ab, g_bb;
  T force[3];  // force_vector, internal 3-component form
};

// what the force of a cell is made from: the two stencil sums, accumulated direction by direction
template <class T>
struct MixSums {
  T a[3], b[3];
};

template <class T>
__device__ __forceinline__ void mix_sums_clear(MixSums<T>& s) {
  static_for<3>([&](auto ac) {
    constexpr int k = decltype(ac)::value;
    s.a[k] = T(0);
    s.b[k] = T(0);
  });
}

// direction i's term of both sums from the neighbours' densities (called for i = 1 .. Q-1 in ascending order); m: the cell's missing
// bits, wall_a / wall_b: the wall densities of the cell's own bc id
template <class L, class T, int i>
__device__ __forceinline__ void mix_sums_add(T nb_a, T nb_b, unsigned m, T wall_a, T wall_b, MixSums<T>& s) {
  const bool wall = psi_neighbour_is_wall<L, i>(m);
  psi_force_add<L, T, i>(wall ? wall_a : nb_a, s.a);
  psi_force_add<L, T, i>(wall ? wall_b : nb_b, s.b);
}

// the same from two neighbour arrays (nb[0] unused)
template <class L, class T>
__device__ __forceinline__ void mix_sums_of(const T (&nb_a)[L::Q], const T (&nb_b)[L::Q], unsigned m, T wall_a, T wall_b, MixSums<T>& s) {
  mix_sums_clear<T>(s);
  static_for<L::Q - 1>([&](auto ic) {
    constexpr int i = decltype(ic)::value + 1;
    mix_sums_add<L, T, i>(nb_a[i], nb_b[i], m, wall_a, wall_b, s);
  });
}

// F^A and F^B from the sums; psi_a, psi_b: the cell's own densities
template <class T>
__device__ __forceinline__ void mix_forces(const MixModel<T>& mo, T psi_a, T psi_b, const MixSums<T>& s, bool wall_cell, T (&Fa)[3], T (&Fb)[3]) {
  const T na = -psi_a, nb = -psi_b;
  static_for<3>([&](auto ac) {
    constexpr int k = decltype(ac)::value;
    Fa[k] = wall_cell ? T(0) : na * ((mo.g_aa * s.a[k]) + (mo.g_ab * s.b[k]));
    Fb[k] = wall_cell ? T(0) : nb * ((mo.g_ab * s.a[k]) + (mo.g_bb * s.b[k]));
  });
}

// u': the velocity both components relax to
template <class T>
__device__ __forceinline__ void mix_common_velocity(T omega_a, T rho_a, const T (&ua)[3], T omega_b, T rho_b, const T (&ub)[3], T (&uc)[3]) {
  const T wa = omega_a * rho_a, wb = omega_b * rho_b;
  const T den = wa + wb;
  static_for<3>([&](auto ac) {
    constexpr int k = decltype(ac)::value;
    uc[k] = ((wa * ua[k]) + (wb * ub[k])) / den;
  });
}

// One component of one cell after streaming and the streaming-step rules: BGK towards feq(rho, u') with the exact-difference shift
// g + F / rho, or the fullway bounce
template <class L, class T>
__device__ __forceinline__ void mix_collide_component(T (&f)[L::Q], bool fullway, T omega, T rho, const T (&uc)[3], const T (&F)[3], const MixModel<T>& mo) {
  if (!fullway) {
    T us[3];
    static_for<3>([&](auto ac) {
      constexpr int k = decltype(ac)::value;
      if constexpr (k >= 3 - L::D)
        us[k] = uc[k] + (mo.force[k] + F[k] / rho);
      else
        us[k] = T(0);
    });
    const T usqr = usqr_of<L, T>(uc), usqr_s = usqr_of<L, T>(us);
    static_for<L::Q>([&](auto lc) {
      constexpr int l = decltype(lc)::value;
      const T feq = feq_dir<L, T, l>(rho, uc, usqr);
      const T fneq = f[l] - feq;
      f[l] = (f[l] - omega * fneq) + (feq_dir<L, T, l>(rho, us, usqr_s) - feq);
    });
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

// the physical (barycentric) velocity of the exact-difference scheme, one axis
template <class T>
__device__ __forceinline__ T mix_velocity(T rho_a, T ua, T rho_b, T ub, T Fa, T Fb) {
  return (((rho_a * ua) + (rho_b * ub)) + (Fa + Fb) / T(2)) / (rho_a + rho_b);
}

}  // namespace xlb
