// The boundary-masker kernels, launched by masker.hip only: the indices masker and the four mesh voxelisers (AABB, RAY, WINDING,
// AABB_CLOSE) with their wall distances.
#pragma once
#include "ops_kernels.hpp"

namespace xlb {

// ---- masker (indices_boundary_masker.py:73-143, JAX semantics) ---------------------------
// scatter `value` at the listed GLOBAL indices that fall inside this rank's planes
// [x_lo, x_hi) (storage plane = gx - x_lo)
static __global__ void k_scatter_u8(uint8_t* out, const int32_t* idx, int64_t n, uint8_t value, int x_lo, int x_hi, int gy,
                             int gz) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = idx[i], y = idx[n + i], z = idx[2 * n + i];
  if (x < x_lo || x >= x_hi || y < 0 || y >= gy || z < 0 || z >= gz) return;
  out[((size_t)(x - x_lo) * gy + y) * gz + z] = value;
}

// missing[l, x] = (x - c_l outside the global domain) | solid[x - c_l] | old_missing[l, x - c_l]
// solid has one ghost plane on each x side; old (bit-sets) uses the field's own halo.
template <class L>
__global__ void k_missing(uint32_t* out, const uint32_t* old, const uint8_t* solid, Dims d, int halo, int gnx, int x_offset) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  unsigned bits = 0;
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    const int xs = x - L::c(0, l), ys = y - L::c(1, l), zs = z - L::c(2, l);
    const int gxs = xs + x_offset;
    bool mis = gxs < 0 || gxs >= gnx || ys < 0 || ys >= d.ny || zs < 0 || zs >= d.nz;
    if (!mis) {
      mis = solid[((size_t)(xs + 1) * d.ny + ys) * d.nz + zs] != 0;
      if (!mis && (halo > 0 || (xs >= 0 && xs < d.nx)))
        mis = (old[((size_t)(xs + halo) * d.ny + ys) * d.nz + zs] >> l) & 1u;
    }
    bits |= (mis ? 1u : 0u) << l;
  });
  out[((size_t)(x + halo) * d.ny + y) * d.nz + z] = bits;
}

// ---- MeshMaskerAABB (boundary_masker/aabb.py:38-100, mesh_boundary_masker.py:62-181): surface voxelisation of a
// triangle mesh with the triangle / unit-box overlap test of Schwarz & Seidel (2010): the box straddles the triangle's
// plane AND its projection overlaps the triangle's projection on the xy, yz and zx planes.  fp32 throughout.
struct TriBox {
  float n[3], d1, d2;       // unit normal, plane offsets of the two critical box corners
  float ne[3][3][2], de[3][3];  // per projection axis-pair [ax] and edge [i]: 2-D edge normal and offset
};
__device__ inline bool tri_box_setup(const float* v /*[3][3]*/, TriBox& t) {
  float e[3][3];
  for (int a = 0; a < 3; ++a) {
    e[0][a] = v[3 + a] - v[a];
    e[1][a] = v[6 + a] - v[3 + a];
    e[2][a] = v[a] - v[6 + a];
  }
  float nx = e[0][1] * (-e[2][2]) - e[0][2] * (-e[2][1]);  // (v1 - v0) x (v2 - v0), v2 - v0 = -e[2]
  float ny = e[0][2] * (-e[2][0]) - e[0][0] * (-e[2][2]);
  float nz = e[0][0] * (-e[2][1]) - e[0][1] * (-e[2][0]);
  const float len = sqrtf(nx * nx + ny * ny + nz * nz);
  if (!(len > 0.0f)) return false;  // degenerate triangle: never intersects (mesh_boundary_masker.py:121)
  t.n[0] = nx / len;
  t.n[1] = ny / len;
  t.n[2] = nz / len;
  float c[3];
  for (int a = 0; a < 3; ++a) c[a] = t.n[a] > 0.0f ? 1.0f : 0.0f;
  t.d1 = t.n[0] * (c[0] - v[0]) + t.n[1] * (c[1] - v[1]) + t.n[2] * (c[2] - v[2]);
  t.d2 = t.n[0] * ((1.0f - c[0]) - v[0]) + t.n[1] * ((1.0f - c[1]) - v[1]) + t.n[2] * ((1.0f - c[2]) - v[2]);
  for (int ax0 = 0; ax0 < 3; ++ax0) {
    const int ax1 = (ax0 + 1) % 3, ax2 = (ax0 + 2) % 3;
    const float sgn = t.n[ax2] < 0.0f ? -1.0f : 1.0f;
    for (int i = 0; i < 3; ++i) {
      const float a0 = -sgn * e[i][ax1], a1 = sgn * e[i][ax0];
      t.ne[ax0][i][0] = a0;
      t.ne[ax0][i][1] = a1;
      t.de[ax0][i] = -(a0 * v[3 * i + ax0] + a1 * v[3 * i + ax1]) + fmaxf(0.0f, a0) + fmaxf(0.0f, a1);
    }
  }
  return true;
}
__device__ inline bool tri_box_overlap(const TriBox& t, float lx, float ly, float lz) {
  const float low[3] = {lx, ly, lz};
  const float np = t.n[0] * lx + t.n[1] * ly + t.n[2] * lz;
  if (!((np + t.d1) * (np + t.d2) <= 0.0f)) return false;
  for (int ax0 = 0; ax0 < 3; ++ax0) {
    const int ax1 = (ax0 + 1) % 3;
    for (int i = 0; i < 3; ++i)
      if (!(t.ne[ax0][i][0] * low[ax0] + t.ne[ax0][i][1] * low[ax1] + t.de[ax0][i] >= 0.0f)) return false;
  }
  return true;
}

// ---- what the mesh kernels share ----
// index of voxel (x, y, z) on a grid with ny x nz voxels per x plane
__device__ __forceinline__ size_t voxel(int x, int y, int z, int ny, int nz) { return ((size_t)x * ny + y) * nz + z; }
__device__ __forceinline__ size_t voxel(const Dims& d, int x, int y, int z) { return voxel(x, y, z, d.ny, d.nz); }
__device__ __forceinline__ bool in_box(const Dims& d, int x, int y, int z) { return x >= 0 && x < d.nx && y >= 0 && y < d.ny && z >= 0 && z < d.nz; }
// f(l as an integral constant) for every link but the rest one
template <class L, class F>
__device__ __forceinline__ void for_each_link(F&& f) {
  static_for<L::Q>([&](auto lc) {
    if constexpr (decltype(lc)::value != opp<L>(decltype(lc)::value)) f(lc);
  });
}
// the neighbour at +c_l is inside the box and solid
template <class L, int l>
__device__ __forceinline__ bool solid_ahead(const uint8_t* solid, const Dims& d, int x, int y, int z) {
  const int xn = x + L::c(0, l), yn = y + L::c(1, l), zn = z + L::c(2, l);
  return in_box(d, xn, yn, zn) && solid[voxel(d, xn, yn, zn)];
}
// resolve_out_of_bound_kernel (mesh_boundary_masker.py:156-176): the directions a voxel pulls from outside the box
template <class L>
__device__ __forceinline__ unsigned outside_bits(const Dims& d, int x, int y, int z) {
  unsigned bits = 0;
  for_each_link<L>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    if (!in_box(d, x - L::c(0, l), y - L::c(1, l), z - L::c(2, l))) bits |= 1u << l;
  });
  return bits;
}
// one thread per triangle: its nine coordinates, null past the end
__device__ __forceinline__ const float* tri_of_thread(const float* verts /*[n_tri][3][3]*/, int64_t n_tri) {
  const int64_t tix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  return tix < n_tri ? verts + 9 * tix : nullptr;
}
// f(i, j, k) over the voxels of one triangle's window on an nx x ny x nz grid, by one of two rules on its bounding box [mn, mx]:
// TOUCH: the unit voxels [i, i + 1] that touch it, on a grid padded by w voxels per side (voxel i is the cube at i - w):
//        i + 1 >= mn and i <= mx, the candidates of wp.mesh_query_aabb(low, low + 1) (mesh_boundary_masker.py:135-154).  ceil, not
//        floor: the overlap test is only exact for those; one cell further down, a voxel beyond an acute corner passes every edge
//        function without touching the triangle.
// else:  the voxels whose centre i + 0.5 lies within `reach` links of it, on the safe side: w = 1 for reach 1 (<= 1 per axis), 2 for 1.5
template <bool TOUCH, class F>
__device__ __forceinline__ void tri_window(const float* v, int nx, int ny, int nz, int w, F&& f) {
  int lo[3], hi[3];
  const int ext[3] = {nx, ny, nz};
  for (int a = 0; a < 3; ++a) {
    const float mn = fminf(v[a], fminf(v[3 + a], v[6 + a])), mx = fmaxf(v[a], fmaxf(v[3 + a], v[6 + a]));
    lo[a] = max(0, TOUCH ? (int)ceilf(mn) - 1 + w : (int)floorf(mn) - 1 - w);
    hi[a] = min(ext[a] - 1, (int)floorf(mx) + w);
  }
  for (int i = lo[0]; i <= hi[0]; ++i)
    for (int j = lo[1]; j <= hi[1]; ++j)
      for (int k = lo[2]; k <= hi[2]; ++k) f(i, j, k);
}

// one thread per triangle: every unit voxel its bounding box touches is tested, hits are marked solid.  The grid is the domain
// padded by `pad` voxels per side (AABB_CLOSE; 0 for AABB): voxel (i, j, k) is the unit cube at (i - pad, j - pad, k - pad)
static __global__ void k_mesh_solid(const float* verts, int64_t n_tri, uint8_t* solid, int nx, int ny, int nz, int pad) {
  const float* v = tri_of_thread(verts, n_tri);
  TriBox t;
  if (!v || !tri_box_setup(v, t)) return;
  tri_window<true>(v, nx, ny, nz, pad, [&](int i, int j, int k) {
    if (tri_box_overlap(t, (float)(i - pad), (float)(j - pad), (float)(k - pad))) solid[voxel(i, j, k, ny, nz)] = 1;
  });
}
// per voxel (aabb.py:57-79 + resolve_out_of_bound_kernel): solid voxels get BC_SOLID (255); a fluid voxel with a solid
// neighbour at +c_l gets the BC id and missing[opp l]; voxels of this id also miss every direction pulled from outside the box
template <class L>
__global__ void k_mesh_classify(const uint8_t* solid, uint8_t* bc, uint32_t* miss, Dims d, int id) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  const size_t c = voxel(d, x, y, z);
  if (bc[c] == 255 || solid[c]) {
    bc[c] = 255;
    return;
  }
  unsigned bits = 0;
  for_each_link<L>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    if (solid_ahead<L, l>(solid, d, x, y, z)) bits |= 1u << opp<L>(l);
  });
  if (bits != 0u) bc[c] = (uint8_t)id;
  if (bc[c] == id) bits |= outside_bits<L>(d, x, y, z);
  if (bits != 0u) miss[c] |= bits;
}

// ---- MeshMaskerRay (boundary_masker/ray.py:38-76): a voxel whose link along c_l (from its centre, length |c_l|) crosses the
// surface gets the BC id and missing[opp l].  One thread per triangle over the voxels around its bounding box; the
// segment / triangle test is Moeller-Trumbore in fp32 (both faces count, like a mesh ray query).
// closest-hit building block: true and *t_out = ray parameter when the segment p + t d, 0 <= t <= max_t, meets the triangle
__device__ inline bool seg_tri_t(const float* v, float px, float py, float pz, float dx, float dy, float dz, float max_t, float* t_out) {
  const float e1x = v[3] - v[0], e1y = v[4] - v[1], e1z = v[5] - v[2];
  const float e2x = v[6] - v[0], e2y = v[7] - v[1], e2z = v[8] - v[2];
  const float pvx = dy * e2z - dz * e2y, pvy = dz * e2x - dx * e2z, pvz = dx * e2y - dy * e2x;
  const float det = (e1x * pvx + e1y * pvy) + e1z * pvz;
  if (fabsf(det) < 1e-12f) return false;
  const float inv = 1.0f / det;
  const float tx = px - v[0], ty = py - v[1], tz = pz - v[2];
  const float u = ((tx * pvx + ty * pvy) + tz * pvz) * inv;
  if (u < 0.0f || u > 1.0f) return false;
  const float qx = ty * e1z - tz * e1y, qy = tz * e1x - tx * e1z, qz = tx * e1y - ty * e1x;
  const float w = ((dx * qx + dy * qy) + dz * qz) * inv;
  if (w < 0.0f || u + w > 1.0f) return false;
  const float t = ((e2x * qx + e2y * qy) + e2z * qz) * inv;
  *t_out = t;
  return t >= 0.0f && t <= max_t;
}
template <class L, int l>
__device__ __forceinline__ float link_len() {
  constexpr int n2 = L::c(0, l) * L::c(0, l) + L::c(1, l) * L::c(1, l) + L::c(2, l) * L::c(2, l);
  return n2 == 1 ? 1.0f : (n2 == 2 ? 1.41421356237309515f : 1.73205080756887719f);
}
// the cast along link l from the centre of voxel (i, j, k) over `reach` (1 or 1.5) link lengths: unit direction c_l / |c_l|
// component by component, max_t = reach |c_l|, *t = ray parameter of the hit (oracle/mesh_bc.py restates this operation order)
template <class L, int l>
__device__ __forceinline__ bool link_hit(const float* v, int i, int j, int k, float reach, float* t) {
  const float len = link_len<L, l>();
  return seg_tri_t(v, (float)i + 0.5f, (float)j + 0.5f, (float)k + 0.5f, (float)L::c(0, l) / len, (float)L::c(1, l) / len, (float)L::c(2, l) / len,
                   reach * len, t);
}
// smallest ray parameter so far of link l of voxel c (non-negative floats order like their bit patterns)
__device__ __forceinline__ void t_min(unsigned* tbuf, size_t cells, int l, size_t c, float t) {
  atomicMin(tbuf + (size_t)l * cells + c, __float_as_uint(t));
}
constexpr unsigned T_NONE = 0x7f800000u;  // +inf: no hit

// One thread per triangle over the voxels around its bounding box.  DIST (the wall distances of ray.py:69-76): additionally the
// smallest ray parameter of every link goes to tbuf[l][voxel], which k_mesh_weights_ray turns into distances; tbuf is unused otherwise
template <class L, bool DIST>
__global__ void k_mesh_ray(const float* verts, int64_t n_tri, uint8_t* bc, uint32_t* miss, unsigned* tbuf, Dims d, int id) {
  const float* v = tri_of_thread(verts, n_tri);
  if (!v) return;
  const size_t cells = (size_t)d.nx * d.ny * d.nz;
  tri_window<false>(v, d.nx, d.ny, d.nz, 1, [&](int i, int j, int k) {
    const size_t c = voxel(d, i, j, k);
    unsigned bits = 0;
    for_each_link<L>([&](auto lc) {
      constexpr int l = decltype(lc)::value;
      float t;
      if (link_hit<L, l>(v, i, j, k, 1.0f, &t)) {
        bits |= 1u << opp<L>(l);
        if constexpr (DIST) t_min(tbuf, cells, l, c, t);
      }
    });
    if (bits != 0u) {
      bc[c] = (uint8_t)id;
      atomicOr(miss + c, bits);
    }
  });
}
// voxels of this id miss the directions pulled from outside the box
template <class L>
__global__ void k_mesh_resolve(const uint8_t* bc, uint32_t* miss, Dims d, int id) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  const size_t c = voxel(d, x, y, z);
  if (bc[c] != id) return;
  const unsigned bits = outside_bits<L>(d, x, y, z);
  if (bits != 0u) miss[c] |= bits;
}
// RAY: distances[l] = t / |c_l| where a hit was recorded
template <class L>
__global__ void k_mesh_weights_ray(const unsigned* tbuf, FieldView dist, Dims d) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  const size_t cells = (size_t)d.nx * d.ny * d.nz, c = voxel(d, x, y, z);
  for_each_link<L>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    const unsigned tb = tbuf[(size_t)l * cells + c];
    if (tb != T_NONE) static_cast<float*>(dist.data)[(size_t)l * dist.plane_stride + c] = __uint_as_float(tb) / link_len<L, l>();
  });
}

// ---- MeshMaskerWinding (winding.py:46-103) ----
// inside test: generalized winding number of the triangle soup at the voxel centre, exact (sum of the signed solid angles,
// Van Oosterom & Strackee, fp64) instead of Warp's BVH approximation; > 0.5 = inside.  One thread per voxel of the mesh's
// bounding box, every thread walks all triangles (the triangle data is a broadcast read).
static __global__ void k_mesh_winding(const float* verts, int64_t n_tri, uint8_t* solid, Dims d, int lo0, int lo1, int lo2, int n0, int n1, int n2) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)n0 * n1 * n2) return;
  const int i = lo0 + (int)(t / ((int64_t)n1 * n2)), j = lo1 + (int)((t / n2) % n1), k = lo2 + (int)(t % n2);
  const double px = i + 0.5, py = j + 0.5, pz = k + 0.5;
  double sum = 0.0;
  for (int64_t f = 0; f < n_tri; ++f) {
    const float* v = verts + 9 * f;
    const double ax = v[0] - px, ay = v[1] - py, az = v[2] - pz;
    const double bx = v[3] - px, by = v[4] - py, bz = v[5] - pz;
    const double cx = v[6] - px, cy = v[7] - py, cz = v[8] - pz;
    const double la = sqrt(ax * ax + ay * ay + az * az), lb = sqrt(bx * bx + by * by + bz * bz), lc = sqrt(cx * cx + cy * cy + cz * cz);
    const double num = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
    const double den = la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la + (cx * ax + cy * ay + cz * az) * lb;
    sum += 2.0 * atan2(num, den);
  }
  if (sum / (4.0 * 3.14159265358979323846) > 0.5) solid[voxel(d, i, j, k)] = 1;
}
// rays out of the solid voxels: one thread per triangle over the SOLID voxels around its bounding box
template <class L>
__global__ void k_mesh_winding_rays(const float* verts, int64_t n_tri, const uint8_t* solid, unsigned* tbuf, Dims d) {
  const float* v = tri_of_thread(verts, n_tri);
  if (!v) return;
  const size_t cells = (size_t)d.nx * d.ny * d.nz;
  tri_window<false>(v, d.nx, d.ny, d.nz, 1, [&](int i, int j, int k) {
    const size_t c = voxel(d, i, j, k);
    if (!solid[c]) return;
    for_each_link<L>([&](auto lc) {
      constexpr int l = decltype(lc)::value;
      float t;
      if (link_hit<L, l>(v, i, j, k, 1.0f, &t)) t_min(tbuf, cells, l, c, t);
    });
  });
}
// tags: the fluid neighbour at +c_l of a solid voxel whose ray along c_l met the surface gets the id, missing[l] and
// distances[opp l] = (|c_l| - t) / |c_l|; written from the NEIGHBOUR's thread (one writer per voxel); solid voxels -> BC_SOLID
template <class L>
__global__ void k_mesh_winding_tag(const uint8_t* solid, const unsigned* tbuf, uint8_t* bc, uint32_t* miss, FieldView dist, Dims d, int id) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  const size_t cells = (size_t)d.nx * d.ny * d.nz, c = voxel(d, x, y, z);
  if (solid[c]) {
    bc[c] = 255;
    return;
  }
  unsigned bits = 0;
  for_each_link<L>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    const int xs = x - L::c(0, l), ys = y - L::c(1, l), zs = z - L::c(2, l);  // the solid voxel whose ray along c_l reaches me
    if (!in_box(d, xs, ys, zs)) return;
    const size_t cs = voxel(d, xs, ys, zs);
    if (!solid[cs]) return;
    const unsigned tb = tbuf[(size_t)l * cells + cs];
    if (tb == T_NONE) return;
    bits |= 1u << l;
    if (dist.data) {
      const float len = link_len<L, l>();
      static_cast<float*>(dist.data)[(size_t)opp<L>(l) * dist.plane_stride + c] = (len - __uint_as_float(tb)) / len;
    }
  });
  if (bits != 0u) {
    bc[c] = (uint8_t)id;
    miss[c] |= bits;
  }
}

// ---- MeshMaskerAABBClose (aabb_close.py:67-154, 216-263, 303-344) ----
// k_mesh_solid on the grid padded by 2 close_voxels per side, closed (dilated, then eroded) over close_voxels, cropped, classified.
// max (dilate) / min (erode) filter over the (2 h + 1)^3 cube; voxels within h of the padded grid's faces are copied
static __global__ void k_morph(const uint8_t* in, uint8_t* out, int px, int py, int pz, int h, int dilate) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)px * py * pz) return;
  const int i = (int)(t / ((int64_t)py * pz)), j = (int)((t / pz) % py), k = (int)(t % pz);
  if (i < h || i >= px - h || j < h || j >= py - h || k < h || k >= pz - h) {
    out[t] = in[t];
    return;
  }
  uint8_t acc = dilate ? 0 : 1;
  for (int a = -h; a <= h; ++a)
    for (int b = -h; b <= h; ++b)
      for (int c = -h; c <= h; ++c) {
        const uint8_t v = in[((size_t)(i + a) * py + (j + b)) * pz + (k + c)];
        acc = dilate ? (acc | v) : (acc & v);
      }
  out[t] = acc;
}
// crop the padded mask to the domain
static __global__ void k_crop(const uint8_t* in, uint8_t* out, Dims d, int py, int pz, int pad) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  out[voxel(d, x, y, z)] = in[voxel(x + pad, y + pad, z + pad, py, pz)];
}
// closest hit within 1.5 |c_l| along c_l for the boundary voxels (bc == id) whose neighbour at +c_l is solid
template <class L>
__global__ void k_mesh_close_rays(const float* verts, int64_t n_tri, const uint8_t* solid, const uint8_t* bc, unsigned* tbuf, Dims d, int id) {
  const float* v = tri_of_thread(verts, n_tri);
  if (!v) return;
  const size_t cells = (size_t)d.nx * d.ny * d.nz;
  tri_window<false>(v, d.nx, d.ny, d.nz, 2, [&](int i, int j, int k) {
    const size_t c = voxel(d, i, j, k);
    if (bc[c] != id) return;
    for_each_link<L>([&](auto lc) {
      constexpr int l = decltype(lc)::value;
      float t;
      if (solid_ahead<L, l>(solid, d, i, j, k) && link_hit<L, l>(v, i, j, k, 1.5f, &t)) t_min(tbuf, cells, l, c, t);
    });
  });
}
// distances[l] = (t - 0.5 |c_l|) / |c_l| with a hit, 1.0 without, for every link of a boundary voxel that ends in a solid voxel
template <class L>
__global__ void k_mesh_weights_close(const uint8_t* solid, const uint8_t* bc, const unsigned* tbuf, FieldView dist, Dims d, int id) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  const size_t cells = (size_t)d.nx * d.ny * d.nz, c = voxel(d, x, y, z);
  if (bc[c] != id || solid[c]) return;
  for_each_link<L>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    if (!solid_ahead<L, l>(solid, d, x, y, z)) return;
    const unsigned tb = tbuf[(size_t)l * cells + c];
    const float len = link_len<L, l>();
    static_cast<float*>(dist.data)[(size_t)l * dist.plane_stride + c] = tb == T_NONE ? 1.0f : (__uint_as_float(tb) - 0.5f * len) / len;
  });
}

}  // namespace xlb
