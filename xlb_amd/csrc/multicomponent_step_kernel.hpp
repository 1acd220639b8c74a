// The row kernels of the two-component Shan-Chen step.  The forces at cell x need both densities of the post-streaming state at the
// neighbours of x, whose streaming is not known inside the same launch, so one step is TWO launches on one stream:
//   k_mix_density  pull + streaming rules of A -> rho_A, of B -> rho_B, stored in the compute dtype (one value per cell each; a wall
//                  cell stores its wall densities)
//   k_mix_step     pull + streaming rules of both sets again -> rho_s, u_s; both stencils by pull_plane, summed as the pulls arrive;
//                  u', F^A, F^B; both collisions; 2 q non-temporal stores
// and k_mix_out is the second launch storing rho_A, rho_B, the physical velocity and / or the forces instead of colliding.  Per cell
// 2 (3 q) s + 4 s_c bytes (s, s_c: store and compute element), D3Q19 fp32: 472 B, twice the single-component step's 236 B.
//
// All three share ONE front half (mix_front: mp_front of multiphase_step_kernel.hpp on either set), so that the densities behind the
// forces are the step's densities bit for bit.  One cell per thread; the step holds both population sets at once.
#pragma once
#include "multicomponent_kernels.hpp"
#include "multiphase_step_kernel.hpp"

namespace xlb {

template <class T, class S>
struct MixArgs {
  StepArgs<T, S> f;            // component A's part and everything shared, as k_step takes it (f.halo == 0; nzq == nz; f.omega: omega_A)
  const S* src_b;              // component B's populations, the layout of f.src
  S* dst_b;
  T omega_b;
  T *rho_a, *rho_b;            // [nx][ny][nz] each, written by k_mix_density, read by the others
  const T *wall_a, *wall_b;    // [256] wall densities by bc id
  MixModel<T> model;
  T *out_rho_a, *out_rho_b;    // k_mix_out: each may be nullptr
  T *out_u, *out_force_a, *out_force_b;  // d planes each, of u_stride / force_a_stride / force_b_stride elements
  size_t u_stride, force_a_stride, force_b_stride;
};

// the front half of one component: mp_front on the set `src`
template <class L, class T, class S, int HASBC>
__device__ __forceinline__ void mix_front(const StepArgs<T, S>& a, const S* src, const RowCell& r, T (&f)[L::Q], unsigned& id, unsigned& m, bool& fullway) {
  StepArgs<T, S> own = a;  // (uniform; only the source differs)
  own.src = src;
  mp_front<L, T, S, HASBC>(own, r, f, id, m, fullway);
}

template <class L, class T, class S, int HASBC>
__global__ void __launch_bounds__(256) k_mix_density(const MixArgs<T, S> ma) {
  const StepArgs<T, S>& a = ma.f;
  RowCell r;
  if (!row_cell_of_thread<1>(a, blockIdx.x, blockIdx.y, 0, r)) return;
  const size_t xplane = (size_t)r.Xs[1] * r.plane_cells;  // uniform
  static_for<2>([&](auto sc) {
    constexpr bool B = decltype(sc)::value == 1;
    T f[L::Q];
    unsigned id, m;
    bool fullway;
    mix_front<L, T, S, HASBC>(a, B ? ma.src_b : a.src, r, f, id, m, fullway);
    T rho, u[3];
    moments<L, T>(f, rho, u);
    if constexpr (HASBC != 0) {
      if (mp_is_wall_cell(id, fullway)) rho = opaque(B ? ma.wall_b : ma.wall_a)[id];
    }
    const T v[1] = {rho};
    st_aligned<T, 1, false>((B ? ma.rho_b : ma.rho_a) + xplane, r.cell_in_plane * (unsigned)sizeof(T), v);
  });
}

// what the second launch knows of the thread's cell before it collides or stores
template <class L, class T>
struct MixCell {
  T fa[L::Q], fb[L::Q];
  T rho_a, rho_b, ua[3], ub[3];  // bare moments
  T Fa[3], Fb[3];
  bool fullway;
};

template <class L, class T, class S, int HASBC>
__device__ __forceinline__ void mix_forces_of_cell(const MixArgs<T, S>& ma, const RowCell& r, MixCell<L, T>& c) {
  unsigned id, m;
  mix_front<L, T, S, HASBC>(ma.f, ma.f.src, r, c.fa, id, m, c.fullway);
  moments<L, T>(c.fa, c.rho_a, c.ua);
  mix_front<L, T, S, HASBC>(ma.f, ma.src_b, r, c.fb, id, m, c.fullway);
  moments<L, T>(c.fb, c.rho_b, c.ub);
  T wa = T(0), wb = T(0);
  bool wall_cell = false;
  if constexpr (HASBC != 0) {
    if (id != 0u) {
      wa = opaque(ma.wall_a)[id];
      wb = opaque(ma.wall_b)[id];
    }
    wall_cell = mp_is_wall_cell(id, c.fullway);
  }
  // the neighbour at x + c_i is a pull along opp(i)
  MixSums<T> s;
  mix_sums_clear<T>(s);
  static_for<L::Q - 1>([&](auto ic) {
    constexpr int i = decltype(ic)::value + 1;
    T va[1], vb[1];
    pull_plane<L, opp<L>(i)>(ma.rho_a, r, va);
    pull_plane<L, opp<L>(i)>(ma.rho_b, r, vb);
    mix_sums_add<L, T, i>(va[0], vb[0], m, wa, wb, s);
  });
  // (a fluid cell's own stored density is its rho bit for bit; a wall cell's force is zero whatever it carries)
  mix_forces<T>(ma.model, c.rho_a, c.rho_b, s, wall_cell, c.Fa, c.Fb);
}

template <class L, class T, class S, int HASBC>
__global__ void __launch_bounds__(256) k_mix_step(const MixArgs<T, S> ma) {
  const StepArgs<T, S>& a = ma.f;
  RowCell r;
  if (!row_cell_of_thread<1>(a, blockIdx.x, blockIdx.y, 0, r)) return;
  MixCell<L, T> c;
  mix_forces_of_cell<L, T, S, HASBC>(ma, r, c);
  T uc[3];
  mix_common_velocity<T>(a.omega, c.rho_a, c.ua, ma.omega_b, c.rho_b, c.ub, uc);
  const size_t xplane = (size_t)r.Xs[1] * r.plane_cells;
  mix_collide_component<L, T>(c.fa, c.fullway, a.omega, c.rho_a, uc, c.Fa, ma.model);
  store_planes<true, 1, L::Q>(a.dst, a.plane_stride, xplane, r.cell_in_plane, c.fa);
  mix_collide_component<L, T>(c.fb, c.fullway, ma.omega_b, c.rho_b, uc, c.Fb, ma.model);
  store_planes<true, 1, L::Q>(ma.dst_b, a.plane_stride, xplane, r.cell_in_plane, c.fb);
}

// rho_A, rho_B (the moments), the physical velocity and the two forces (the lattice's d components each) of the post-streaming state
template <class L, class T, class S, int HASBC>
__global__ void __launch_bounds__(256) k_mix_out(const MixArgs<T, S> ma) {
  RowCell r;
  if (!row_cell_of_thread<1>(ma.f, blockIdx.x, blockIdx.y, 0, r)) return;
  MixCell<L, T> c;
  mix_forces_of_cell<L, T, S, HASBC>(ma, r, c);
  const size_t cell = (size_t)r.Xs[1] * r.plane_cells + r.cell_in_plane;
  if (ma.out_rho_a) ma.out_rho_a[cell] = c.rho_a;
  if (ma.out_rho_b) ma.out_rho_b[cell] = c.rho_b;
  static_for<L::D>([&](auto dc) {
    constexpr int k = decltype(dc)::value, a = k + (3 - L::D);
    if (ma.out_u) ma.out_u[(size_t)k * ma.u_stride + cell] = mix_velocity<T>(c.rho_a, c.ua[a], c.rho_b, c.ub[a], c.Fa[a], c.Fb[a]);
    if (ma.out_force_a) ma.out_force_a[(size_t)k * ma.force_a_stride + cell] = c.Fa[a];
    if (ma.out_force_b) ma.out_force_b[(size_t)k * ma.force_b_stride + cell] = c.Fb[a];
  });
}

}  // namespace xlb
