// The row kernels of the Shan-Chen step.  The interaction force at cell x needs psi = Psi(rho) of the post-streaming state at the
// neighbours of x, whose streaming is not known inside the same launch, so one step is TWO launches on one stream:
//   k_psi              pull + streaming rules -> rho -> psi, stored in the compute dtype (one value per cell)
//   k_step_multiphase  pull + streaming rules again -> rho, u; the neighbours' psi by pull_plane; force; forced BGK;
//                      q non-temporal stores
// and k_multiphase_out is the second launch storing rho, the physical velocity and / or the force instead of colliding.  Per cell
// (3 q) s + 2 s_c bytes (s, s_c: store and compute element), D3Q19 fp32: 236 B against the fluid step's 152 B.  Fusing the two would
// mean taking psi from the previous step's density (a lagged force): another scheme, not built.
//
// All three share ONE front half (mp_front: the row front end of row_kernel.hpp, the rule functions of cell.hpp), so that the rho behind
// psi is the step's rho bit for bit.  One cell per thread.
#pragma once
#include "multiphase_kernels.hpp"
#include "row_kernel.hpp"
#include "step_kernel.hpp"

namespace xlb {

template <class T, class S>
struct MultiphaseArgs {
  StepArgs<T, S> f;     // the fluid's part, as k_step takes it (fields without ghost planes: f.halo == 0; nzq == nz)
  T* psi;               // [nx][ny][nz], written by k_psi, read by the others
  const T* psi_wall;    // [256] Psi(rho_w) by bc id
  PsiModel<T> model;
  T* out_rho;           // k_multiphase_out: each may be nullptr
  T* out_u;             // d planes of u_stride elements
  T* out_force;         // d planes of force_stride elements
  size_t u_stride, force_stride;
};

// The front half: the post-streaming populations of the cell after the streaming-step rules.  id: the cell's bc id (0 without
// boundary conditions), m: its missing bits (0 when id == 0), fullway: a fullway bounce-back cell.
// HASBC: 0 = no boundary conditions, 1 = halfway (constant wall velocity) and fullway bounce-back, solid cells.
template <class L, class T, class S, int HASBC>
__device__ __forceinline__ void mp_front(const StepArgs<T, S>& a, const RowCell& r, T (&f)[L::Q], unsigned& id, unsigned& m, bool& fullway) {
  constexpr int Q = L::Q;
  static_for<Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    S v[1];
    pull_plane<L, l>(a.src + (size_t)l * a.plane_stride, r, v);
    f[l] = to_compute<T, S>(v[0]);
  });
  id = 0u;
  m = 0u;
  fullway = false;
  if constexpr (HASBC != 0) {
    unsigned ids[1];
    const bool any_bc = load_bc_ids<1>(a.bc + (size_t)r.Xs[1] * r.plane_cells, r.cell_in_plane, ids);
    id = ids[0];
    if (any_bc) {
      // rare path: the missing bits of every boundary cell (the force needs them too)
      const unsigned kind = kind_of(a, id);
      m = ld(a.miss + (size_t)r.Xs[1] * r.plane_cells, opaque(r.cell_in_plane * 4u));
      if (kind == K_HW) {
        const T* val = opaque(a.bc_values + id * 27u);
        T pre[Q];
        load_own_cell<L, false>(a.src, a.plane_stride, (size_t)r.Xs[1] * r.plane_cells, r.cell_in_plane, pre);
        const T uw[5] = {T(0), T(0), T(0), T(0), T(0)};
        apply_streaming_bc<L, T>(XLBHIP_BC_HALFWAY_BB, f, pre, m, val, uw, nullptr);
      } else if (kind == K_FW) {
        fullway = true;
      }
    }
  }
}

// a cell that carries the wall's pseudopotential and feels no force
__device__ __forceinline__ bool mp_is_wall_cell(unsigned id, bool fullway) { return fullway || id == BC_ID_SOLID; }

template <class L, class T, class S, int HASBC>
__global__ void __launch_bounds__(256) k_psi(const MultiphaseArgs<T, S> ma) {
  const StepArgs<T, S>& a = ma.f;
  RowCell r;
  if (!row_cell_of_thread<1>(a, blockIdx.x, blockIdx.y, 0, r)) return;
  T f[L::Q];
  unsigned id, m;
  bool fullway;
  mp_front<L, T, S, HASBC>(a, r, f, id, m, fullway);
  T rho, u[3];
  moments<L, T>(f, rho, u);
  T psi = psi_of<T>(ma.model, rho);
  if constexpr (HASBC != 0) {
    if (mp_is_wall_cell(id, fullway)) psi = opaque(ma.psi_wall)[id];
  }
  T* prow = ma.psi + (size_t)r.Xs[1] * r.plane_cells;  // uniform
  const T v[1] = {psi};
  st_aligned<T, 1, false>(prow, r.cell_in_plane * (unsigned)sizeof(T), v);
}

// rho, u (bare) and F of the thread's cell from the front half and the psi field
template <class L, class T, class S, int HASBC>
__device__ __forceinline__ void mp_force_of_cell(const MultiphaseArgs<T, S>& ma, const RowCell& r, T (&f)[L::Q], bool& fullway, T& rho, T (&u)[3], T (&F)[3]) {
  unsigned id, m;
  mp_front<L, T, S, HASBC>(ma.f, r, f, id, m, fullway);
  moments<L, T>(f, rho, u);
  // the neighbour at x + c_i is a pull along opp(i)
  T nb[L::Q];
  nb[0] = T(0);
  static_for<L::Q - 1>([&](auto ic) {
    constexpr int i = decltype(ic)::value + 1;
    T v[1];
    pull_plane<L, opp<L>(i)>(ma.psi, r, v);
    nb[i] = v[0];
  });
  const T psi = ld(ma.psi + (size_t)r.Xs[1] * r.plane_cells, r.cell_in_plane * (unsigned)sizeof(T));
  T pw = T(0);
  bool wall_cell = false;
  if constexpr (HASBC != 0) {
    if (id != 0u) pw = opaque(ma.psi_wall)[id];
    wall_cell = mp_is_wall_cell(id, fullway);
  }
  psi_force<L, T>(ma.model, psi, nb, m, pw, wall_cell, F);
}

template <class L, class T, class S, int HASBC>
__global__ void __launch_bounds__(256) k_step_multiphase(const MultiphaseArgs<T, S> ma) {
  const StepArgs<T, S>& a = ma.f;
  RowCell r;
  if (!row_cell_of_thread<1>(a, blockIdx.x, blockIdx.y, 0, r)) return;
  T f[L::Q], rho, u[3], F[3];
  bool fullway;
  mp_force_of_cell<L, T, S, HASBC>(ma, r, f, fullway, rho, u, F);
  multiphase_collide_cell<L, T>(f, fullway, a.omega, rho, F, ma.model);
  store_planes<true, 1, L::Q>(a.dst, a.plane_stride, (size_t)r.Xs[1] * r.plane_cells, r.cell_in_plane, f);
}

// rho, u = u_bare + F / (2 rho) and F (the lattice's d components each) of the post-streaming state
template <class L, class T, class S, int HASBC>
__global__ void __launch_bounds__(256) k_multiphase_out(const MultiphaseArgs<T, S> ma) {
  RowCell r;
  if (!row_cell_of_thread<1>(ma.f, blockIdx.x, blockIdx.y, 0, r)) return;
  T f[L::Q], rho, u[3], F[3];
  bool fullway;
  mp_force_of_cell<L, T, S, HASBC>(ma, r, f, fullway, rho, u, F);
  const size_t cell = (size_t)r.Xs[1] * r.plane_cells + r.cell_in_plane;
  if (ma.out_rho) ma.out_rho[cell] = rho;
  static_for<L::D>([&](auto dc) {
    constexpr int k = decltype(dc)::value, a = k + (3 - L::D);
    if (ma.out_u) ma.out_u[(size_t)k * ma.u_stride + cell] = multiphase_velocity<T>(u[a], F[a], rho);
    if (ma.out_force) ma.out_force[(size_t)k * ma.force_stride + cell] = F[a];
  });
}

}  // namespace xlb
