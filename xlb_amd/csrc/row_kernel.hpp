// The front end of the row kernels (k_step, k_step_scalar, the multiphase kernels, k_adjoint_step): where a thread's cells sit, the
// pull of one direction, the boundary ids, the own-cell loads and the store; and the memory helpers the two-step kernel shares.
//   * Mapping: x is block-uniform (blockIdx.z), lanes run along z, a thread owns VEC consecutive z cells of one row and pulls each
//     direction once.
//   * Address form: every global access is `uniform base (SGPR pair) + 32-bit byte offset (VGPR)`.  The population plane and the x plane
//     go into the base by scalar arithmetic; the offset is (row + z) * element size.  RowCell keeps rows and cells in ELEMENTS inside
//     one x plane; pull_plane, load_own_cell and store_planes multiply by the size of the element they move, because the fields of one
//     kernel differ in it (populations in the store type, psi in the compute type, id bytes, words of missing bits).
//   * Bound: cell_in_plane < ny nz, and ny nz * element size must stay below 2^32 for every field of the kernel.  The single-rank
//     steppers require ny nz <= 2^28 (check_single_rank_grid, api_internal.hpp), which covers 8-byte elements.
//   * Row ends: the row is periodic.  For c_z = +-1 a thread loads its VEC elements shifted by one; the thread at z0 == 0 (c_z = +1) or
//     z0 + VEC == nz (c_z = -1) loads them unshifted instead, so that no vector load leaves the row, and takes the one wrapped element
//     (nz - 1 or 0) by a load of its own.
#pragma once
#include "cell.hpp"

namespace xlb {

template <class S, int N>
struct VecOf {
  typedef S aligned __attribute__((ext_vector_type(N), aligned(sizeof(S) * N)));
  typedef S shifted __attribute__((ext_vector_type(N), aligned(sizeof(S))));
};

// p = uniform base, boff = per-thread byte offset (32 bit) -> global_load ... v_off, s[base]
template <class S>
__device__ __forceinline__ S ld(const S* base, unsigned boff) {
  return *reinterpret_cast<const S*>(reinterpret_cast<const char*>(base) + boff);
}
template <class S, int VEC, bool NT = false>
__device__ __forceinline__ void ld_aligned(const S* base, unsigned boff, S (&out)[VEC]) {
  if constexpr (VEC == 1) {
    if constexpr (NT)
      out[0] = __builtin_nontemporal_load(reinterpret_cast<const S*>(reinterpret_cast<const char*>(base) + boff));
    else
      out[0] = ld(base, boff);
  } else {
    typedef typename VecOf<S, VEC>::aligned V;
    V v;
    if constexpr (NT)
      v = __builtin_nontemporal_load(reinterpret_cast<const V*>(reinterpret_cast<const char*>(base) + boff));
    else
      v = *reinterpret_cast<const V*>(reinterpret_cast<const char*>(base) + boff);
#pragma unroll
    for (int k = 0; k < VEC; ++k) out[k] = v[k];
  }
}
template <class S, int VEC>
__device__ __forceinline__ void ld_shifted(const S* base, unsigned boff, S (&out)[VEC]) {
  typedef typename VecOf<S, VEC>::shifted V;
  const V v = *reinterpret_cast<const V*>(reinterpret_cast<const char*>(base) + boff);
#pragma unroll
  for (int k = 0; k < VEC; ++k) out[k] = v[k];
}
template <class S, int VEC, bool NT>
__device__ __forceinline__ void st_aligned(S* base, unsigned boff, const S (&in)[VEC]) {
  char* p = reinterpret_cast<char*>(base) + boff;
  if constexpr (VEC == 1) {
    if constexpr (NT)
      __builtin_nontemporal_store(in[0], reinterpret_cast<S*>(p));
    else
      *reinterpret_cast<S*>(p) = in[0];
  } else {
    typedef typename VecOf<S, VEC>::aligned V;
    V v;
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = in[k];
    if constexpr (NT)
      __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
    else
      *reinterpret_cast<V*>(p) = v;
  }
}

// Identity the optimiser cannot see through.  The BC branches of the row kernels issue loads that are
// textually identical across branches (own-cell populations, per-BC constants); LLVM would hoist
// them above the branch and keep ~40 extra VGPRs live in the fluid fast path.
__device__ __forceinline__ unsigned opaque(unsigned v) {
  asm volatile("" : "+v"(v));
  return v;
}
template <class P>
__device__ __forceinline__ const P* opaque(const P* p) {
  asm volatile("" : "+v"(p));
  return p;
}

// where a thread's VEC cells sit
struct RowCell {
  int Xs[3];        // storage x plane of the source for c_x = -1, 0, +1 (index c_x + 1); uniform
  unsigned Ye[3];   // first element of the three y-neighbour rows inside an x plane (index c_y + 1)
  int z0, nz;       // first of the thread's cells in its row; row length
  bool at_z_lo, at_z_hi;
  size_t plane_cells;
  unsigned cell_in_plane;  // own row + z0
};

// Fills r for the thread of block column bx, block row by (blockIdx.x, blockIdx.y unless the caller remaps them) from the box of `a`
// (a StepArgs: nx, ny, nz, x_begin); halo: ghost planes per side of the field, 0: the periodic wrap in x is done here.
// false: the thread has no cell; r is then that of cell (y, z) = (0, 0), for callers that have to stay for a block-wide sum.
template <int VEC, class A>
__device__ __forceinline__ bool row_cell_of_thread(const A& a, unsigned bx, unsigned by, int halo, RowCell& r) {
  int zq = bx * blockDim.x + threadIdx.x;
  int y = by * blockDim.y + threadIdx.y;
  const bool inside = zq * VEC < a.nz && y < a.ny;  // (nz is a multiple of VEC)
  if (!inside) {
    zq = 0;
    y = 0;
  }
  const int x = a.x_begin + blockIdx.z;  // block-uniform
  const int ny = a.ny, nz = a.nz;
  if (halo) {
    r.Xs[0] = x + halo + 1;
    r.Xs[1] = x + halo;
    r.Xs[2] = x + halo - 1;
  } else {
    r.Xs[0] = (x + 1 == a.nx) ? 0 : x + 1;
    r.Xs[1] = x;
    r.Xs[2] = (x == 0) ? a.nx - 1 : x - 1;
  }
  r.Ye[0] = (unsigned)((y + 1 == ny) ? 0 : y + 1) * (unsigned)nz;
  r.Ye[1] = (unsigned)y * (unsigned)nz;
  r.Ye[2] = (unsigned)((y == 0) ? ny - 1 : y - 1) * (unsigned)nz;
  r.z0 = zq * VEC;
  r.nz = nz;
  r.at_z_lo = (r.z0 == 0);
  r.at_z_hi = (r.z0 + VEC == nz);
  r.plane_cells = (size_t)ny * nz;
  r.cell_in_plane = r.Ye[1] + (unsigned)r.z0;
  return inside;
}

// One direction's pull of a thread's VEC cells from the uniform x plane `row`, in BYTES (yb: the row, zb: z0): v[k] = row[y][z0 + k - cz],
// periodic.  FLAGS bit 1: non-temporal loads of the c_z == 0 directions; bit 2: of the z-shifted directions too (VEC == 1).
template <class S, int VEC, int cz, int FLAGS = 0>
__device__ __forceinline__ void pull_dir(const S* row, unsigned yb, unsigned zb, int z0, int nz, bool at_z_lo, bool at_z_hi, S (&v)[VEC]) {
  constexpr unsigned ES = sizeof(S);
  if constexpr (cz == 0) {
    ld_aligned<S, VEC, (FLAGS & 2) != 0>(row, yb + zb, v);
  } else if constexpr (VEC == 1) {
    int zs = z0 - cz;
    zs = zs < 0 ? nz - 1 : (zs == nz ? 0 : zs);
    ld_aligned<S, 1, (FLAGS & 4) != 0>(row, yb + (unsigned)zs * ES, v);
  } else if constexpr (cz == 1) {
    // need z0-1 .. z0+VEC-2 ; at the row start z0-1 wraps to nz-1
    S t[VEC];
    ld_shifted<S, VEC>(row, yb + zb - (at_z_lo ? 0u : ES), t);
    S wrapv = t[0];
    if (at_z_lo) wrapv = ld(row, yb + (unsigned)(nz - 1) * ES);
    v[0] = at_z_lo ? wrapv : t[0];
#pragma unroll
    for (int k = 1; k < VEC; ++k) v[k] = at_z_lo ? t[k - 1] : t[k];
  } else {
    // cz == -1: need z0+1 .. z0+VEC ; at the row end z0+VEC wraps to 0
    S t[VEC];
    ld_shifted<S, VEC>(row, yb + zb + (at_z_hi ? 0u : ES), t);
    S wrapv = t[VEC - 1];
    if (at_z_hi) wrapv = ld(row, yb);
#pragma unroll
    for (int k = 0; k < VEC - 1; ++k) v[k] = at_z_hi ? t[k + 1] : t[k];
    v[VEC - 1] = at_z_hi ? wrapv : t[VEC - 1];
  }
}

// The values of one population plane (`plane`: its storage plane 0, any element type) arriving at the thread's cells along direction d,
// i.e. from cell - c_d.  The value AT cell + c_i is the pull along d = opp(i).
template <class L, int d, int FLAGS = 0, class E, int VEC>
__device__ __forceinline__ void pull_plane(const E* plane, const RowCell& r, E (&v)[VEC]) {
  constexpr int cx = L::c(0, d), cy = L::c(1, d), cz = L::c(2, d);
  const E* row = plane + (size_t)r.Xs[cx + 1] * r.plane_cells;  // uniform
  pull_dir<E, VEC, cz, FLAGS>(row, r.Ye[cy + 1] * (unsigned)sizeof(E), (unsigned)r.z0 * (unsigned)sizeof(E), r.z0, r.nz, r.at_z_lo, r.at_z_hi, v);
}

// The boundary ids of a thread's VEC cells from the x plane `bcp` (uniform) of the id field: one word for VEC 4, a half word for VEC 2,
// a byte for VEC 1.  Returns whether any of them is a boundary cell.
template <int VEC>
__device__ __forceinline__ bool load_bc_ids(const uint8_t* bcp, unsigned cell_in_plane, unsigned (&ids)[VEC]) {
  static_assert(VEC == 1 || VEC == 2 || VEC == 4, "one load per thread");
  if constexpr (VEC == 4) {
    const unsigned wrd = ld(reinterpret_cast<const unsigned*>(bcp), cell_in_plane);
#pragma unroll
    for (int k = 0; k < 4; ++k) ids[k] = (wrd >> (8 * k)) & 0xffu;
    return wrd != 0u;
  } else if constexpr (VEC == 2) {
    const unsigned wrd = ld(reinterpret_cast<const unsigned short*>(bcp), cell_in_plane);
    ids[0] = wrd & 0xffu;
    ids[1] = (wrd >> 8) & 0xffu;
    return wrd != 0u;
  } else {
    ids[0] = ld(bcp, cell_in_plane);
    return ids[0] != 0u;
  }
}

// The pre-streaming populations of ONE cell (element `cell` of the x plane starting `xplane` elements into each of the field's N planes,
// `plane_stride` elements apart; all uniform): pre[l] = plane l, or plane opp(l) with OPP (N == L::Q then).  For the rare boundary
// path: the offset is opaque, so that the loads are not hoisted out of their branch into the fluid path.
template <class L, bool OPP, class T, class S, int N>
__device__ __forceinline__ void load_own_cell(const S* field, size_t plane_stride, size_t xplane, unsigned cell, T (&pre)[N]) {
  const unsigned cb = opaque(cell * (unsigned)sizeof(S));
  static_for<N>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    constexpr int p = OPP ? opp<L>(l) : l;
    pre[l] = to_compute<T, S>(ld(field + xplane + (size_t)p * plane_stride, cb));
  });
}

// Stores the N planes of a thread's VEC cells (f: the first element of ONE contiguous T[VEC][N], f[k * N + l]: cell k, plane l; a
// one-cell kernel passes its T[N]), cast to the store type, to the x plane starting `xplane` elements into each plane of `field`;
// NT: non-temporal.  (The order of the pointer sums here and in load_own_cell, and the compile-time loop, are what keeps every
// instantiation's registers: profiles/row_front_end.md.)
template <bool NT, int VEC, int N, class T, class S>
__device__ __forceinline__ void store_planes(S* field, size_t plane_stride, size_t xplane, unsigned cell_in_plane, const T* f) {
  static_for<N>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    S v[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = to_store<S, T>(f[k * N + l]);
    st_aligned<S, VEC, NT>(field + (size_t)l * plane_stride + xplane, cell_in_plane * (unsigned)sizeof(S), v);
  });
}

}  // namespace xlb
