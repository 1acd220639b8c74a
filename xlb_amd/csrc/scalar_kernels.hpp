// Scalar transport (advection-diffusion of one scalar phi carried by the flow): the cell-level rules and the small whole-field kernels.
//
// The scalar lives on the sub-lattice of the fluid lattice L made of the rest direction and L's main directions (|c|_1 == 1) in
// ascending order: D2Q5 inside D2Q9, D3Q7 inside D3Q19 / D3Q27.  Its populations g (2 d + 1 of them, layout of f) are pulled like f,
// relaxed towards the LINEAR equilibrium  geq_j = w_j phi (1 + c_j.u / cs^2)  with the velocity u the fluid step holds in registers
// (the bare first moment of the post-streaming f), and — with buoyancy — phi = sum_j g_j enters the fluid's exact-difference force
// before the fluid collides: force = force_vector + buoyancy (phi - reference).  The diffusivity is cs^2 (1 / omega_s - 1/2).
//
// Everything here compiles for the host too (tests/scalar_cpu_emulation.cpp): the fused kernel, which needs the addressing of
// step_kernel.hpp, is in scalar_step_kernel.hpp and calls scalar_apply_rule and scalar_collide_cell below for every cell.
// tests/_scalar_ref.py restates the step in NumPy, operation for operation.
#pragma once
#include "ops_kernels.hpp"

namespace xlb {

// what a ScalarBC does where its fluid BC's cell misses a main direction (no second mask: the fluid's bc id and missing bits)
enum { SCALAR_ADIABATIC = 0, SCALAR_DIRICHLET = 1, SCALAR_DO_NOTHING = 2 };

template <class L>
struct ScalarSet {
  static constexpr int D = L::D, Q = 2 * L::D + 1;
  // fluid direction of scalar direction j
  static constexpr int dir(int j) {
    int n = 0;
    for (int l = 0; l < L::Q; ++l) {
      const int a = iabs(L::c(0, l)) + iabs(L::c(1, l)) + iabs(L::c(2, l));
      if (j == 0 && a == 0) return l;
      if (a == 1 && ++n == j) return l;
    }
    return -1;
  }
  static constexpr int opp(int j) {
    for (int k = 0; k < Q; ++k)
      if (dir(k) == xlb::opp<L>(dir(j))) return k;
    return -1;
  }
  static constexpr double w(int j) { return D == 3 ? (j == 0 ? 1.0 / 4.0 : 1.0 / 8.0) : (j == 0 ? 1.0 / 3.0 : 1.0 / 6.0); }
  static constexpr double inv_cs2 = D == 3 ? 4.0 : 3.0;
};

// force_vector + buoyancy (phi - reference), in the internal 3-component form
struct ScalarCoupling {
  double force[3];
  double buoyancy[3];
  double reference;
};

// The scalar's streaming-step rule at a boundary cell: g = pulled populations, pre = the cell's own pre-streaming ones,
// m = the FLUID's missing bits.  Dirichlet: anti-bounce-back, the scalar takes `value` at the link midpoint; adiabatic:
// bounce-back; do-nothing: the cell keeps its pre-streaming populations.
template <class L, class T>
__device__ __forceinline__ void scalar_apply_rule(unsigned rule, T value, unsigned m, const T (&pre)[ScalarSet<L>::Q], T (&g)[ScalarSet<L>::Q]) {
  typedef ScalarSet<L> G;
  if (rule == SCALAR_DO_NOTHING) {
    static_for<G::Q>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      g[j] = pre[j];
    });
    return;
  }
  static_for<G::Q - 1>([&](auto jc) {
    constexpr int j = decltype(jc)::value + 1;
    constexpr int l = G::dir(j), o = G::opp(j);  // (constants: evaluated here, not by a run-time walk of the lattice tables)
    if ((m >> l) & 1u) {
      if (rule == SCALAR_DIRICHLET)
        g[j] = -pre[o] + (T(2) * T(G::w(j))) * value;
      else
        g[j] = pre[o];
    }
  });
}

// phi = sum_j g_j, sequential in j
template <class L, class T>
__device__ __forceinline__ T scalar_sum(const T (&g)[ScalarSet<L>::Q]) {
  T phi = g[0];
  static_for<ScalarSet<L>::Q - 1>([&](auto jc) { phi = phi + g[decltype(jc)::value + 1]; });
  return phi;
}

template <class L, class T, int j>
__device__ __forceinline__ T scalar_geq_dir(T phi, const T (&u)[3]) {
  typedef ScalarSet<L> G;
  constexpr int l = G::dir(j);
  T cu = T(0);
  static_for<3>([&](auto ac) {
    constexpr int a = decltype(ac)::value;
    if constexpr (L::c(a, l) == 1) cu = u[a];
    if constexpr (L::c(a, l) == -1) cu = -u[a];
  });
  return (T(G::w(j)) * phi) * (T(1) + T(G::inv_cs2) * cu);
}

// g -> g - omega_s (g - geq(phi, u))
template <class L, class T>
__device__ __forceinline__ void scalar_collide(T (&g)[ScalarSet<L>::Q], T phi, const T (&u)[3], T omega_s) {
  static_for<ScalarSet<L>::Q>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    const T gneq = g[j] - scalar_geq_dir<L, T, j>(phi, u);
    g[j] = g[j] - omega_s * gneq;
  });
}

// One cell after streaming and the streaming-step rules of both fields: phi and u, the fluid's collision (forced per cell when COLL
// has COLL_FORCED), the scalar's, and the fullway bounce of both at a fullway cell.
template <class L, class T, int COLL>
__device__ __forceinline__ void scalar_collide_cell(T (&f)[L::Q], T (&g)[ScalarSet<L>::Q], bool fullway, T omega, T omega_s, const CollideExtra& ex,
                                                    const ScalarCoupling& cp) {
  typedef ScalarSet<L> G;
  const T phi = scalar_sum<L, T>(g);
  T rho, u[3];
  moments<L, T>(f, rho, u);
  if (!fullway) {
    if constexpr ((COLL & COLL_FORCED) != 0) {
      CollideExtra exc = ex;
      const T dphi = phi - T(cp.reference);
      static_for<3>([&](auto ac) {
        constexpr int a = decltype(ac)::value;
        exc.force[a] = (double)(T(cp.force[a]) + T(cp.buoyancy[a]) * dphi);
      });
      collide<L, T, COLL>(f, omega, exc);
    } else {
      collide<L, T, COLL>(f, omega, ex);
    }
    scalar_collide<L, T>(g, phi, u, omega_s);
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
    static_for<G::Q>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      constexpr int o = G::opp(j);
      if constexpr (j < o) {
        const T t = g[j];
        g[j] = g[o];
        g[o] = t;
      }
    });
  }
}

// ---- whole-field kernels (one thread per cell) -------------------------------------------------------------------------------

// g = geq(phi0, u(f)): the scalar's equilibrium at the initial FLOW.  phi: a cardinality-1 field, or no data -> the constant phi0
template <class L, class T>
__global__ void k_scalar_init(FieldView f, FieldView phi, T phi0, FieldView g, Dims d) {
  typedef ScalarSet<L> G;
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
  const T p = phi.data ? load_rt<T>(phi, cell_index(phi, d, x, y, z)) : phi0;
  const size_t o = cell_index(g, d, x, y, z);
  static_for<G::Q>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    store_rt<T>(g, (size_t)j * g.plane_stride + o, scalar_geq_dir<L, T, j>(p, u));
  });
}

// ScalarMoment()(g, phi): phi = sum_j g_j
template <class L, class T>
__global__ void k_scalar_moment(FieldView g, FieldView phi, Dims d) {
  typedef ScalarSet<L> G;
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  T gg[G::Q];
  const size_t i = cell_index(g, d, x, y, z);
  static_for<G::Q>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    gg[j] = load_rt<T>(g, (size_t)j * g.plane_stride + i);
  });
  store_rt<T>(phi, cell_index(phi, d, x, y, z), scalar_sum<L, T>(gg));
}

}  // namespace xlb
