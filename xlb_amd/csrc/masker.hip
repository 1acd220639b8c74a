// libxlbhip: the boundary maskers.  The indices masker (bc_mask and missing_mask from index lists) and the mesh voxelisers
// (boundary_masker/{aabb,ray,winding,aabb_close}.py) with their wall distances.
#include <algorithm>
#include <vector>

#include "api_internal.hpp"
#include "masker_kernels.hpp"

using namespace xlb;

// Every masker kernel has one work item per thread, 256 threads per block
template <class K, class... A>
static void launch_flat(K kernel, size_t n, hipStream_t st, A... args) {
  hipLaunchKernelGGL(kernel, blocks_for(n), 256, 0, st, args...);
}

// Mesh voxelisation, all methods (boundary_masker/{aabb,ray,winding,aabb_close}.py), with the wall distances where `dist` is given:
// the argument checks, the mesh's extent, the upload and the passes of the method.
static int mesh_mask(xlbhip_ctx* c, int lattice, int method, int bc_id, int64_t n_triangles, const float* vertices, int close_voxels, xlbhip_field* bcm,
                     xlbhip_field* miss, xlbhip_field* dist) {
  XLB_REQUIRE(c && bcm && miss && (n_triangles == 0 || vertices), "mesh masker: null argument");
  XLB_REQUIRE((method == XLBHIP_MESH_AABB && !dist) || method == XLBHIP_MESH_RAY || method == XLBHIP_MESH_WINDING || method == XLBHIP_MESH_AABB_CLOSE,
              "mesh masker: method %d has no wall distances (RAY, WINDING, AABB_CLOSE do)", method);
  XLB_REQUIRE(lattice == XLBHIP_D3Q19 || lattice == XLBHIP_D3Q27, "MeshBoundaryMasker is only implemented for 3D velocity sets!");
  XLB_REQUIRE(bcm->dtype == XLBHIP_U8 && bcm->card == 1 && bcm->halo == 0, "mesh masker: bc_mask must be a (1, nx, ny, nz) uint8 field without ghost planes");
  XLB_REQUIRE(miss->dtype == XLBHIP_MISSING && miss->card == lattice_q(lattice) && same_grid(miss, bcm) && miss->halo == 0, "mesh masker: bad missing_mask field");
  XLB_REQUIRE(bc_id >= 1 && bc_id <= 254, "bc id %d out of range 1..254", bc_id);
  XLB_REQUIRE(!dist || (dist->dtype == XLBHIP_F32 && dist->card == lattice_q(lattice) && same_grid(dist, bcm) && dist->halo == 0),
              "mesh masker: distances must be a (q, nx, ny, nz) fp32 field on the masks' grid");
  XLB_REQUIRE(method != XLBHIP_MESH_AABB_CLOSE || (close_voxels >= 1 && close_voxels <= 8), "AABB_CLOSE: close_voxels must be 1..8 (got %d)", close_voxels);
  // the mesh must lie inside the domain (mesh_boundary_masker.py:196-201); its bounding box [lo, hi] is WINDING's window
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int64_t i = 0; i < n_triangles * 3; ++i)
    for (int a = 0; a < 3; ++a) {
      const float p = vertices[3 * i + a];
      const int ext = a == 0 ? bcm->nx : (a == 1 ? bcm->ny : bcm->nz);
      XLB_REQUIRE(p >= 0.0f && p < (float)ext, "Mesh extents exceed domain dimensions (%d,%d,%d). The mesh must be fully contained within the domain.",
                  bcm->nx, bcm->ny, bcm->nz);
      lo[a] = i == 0 ? p : std::min(lo[a], p);
      hi[a] = i == 0 ? p : std::max(hi[a], p);
    }
  touch(bcm);
  touch(miss);
  if (dist) touch(dist);
  if (n_triangles == 0) return 0;
  hipStream_t st = c->stream;
  DeviceScratch scratch(st);  // every exit releases the temporaries, after the stream has drained
  const Dims d = dims(bcm);
  const size_t cells = bcm->cells(), nt = (size_t)n_triangles;
  const int q = lattice_q(lattice);
  float* dv = nullptr;
  XLB_HIP(scratch.alloc(&dv, nt * 9 * sizeof(float)));
  XLB_HIP(hipMemcpyAsync(dv, vertices, nt * 9 * sizeof(float), hipMemcpyHostToDevice, st));
  unsigned* tbuf = nullptr;  // closest ray parameter per (link, voxel), +inf = none
  if (dist || method == XLBHIP_MESH_WINDING) {
    XLB_HIP(scratch.alloc(&tbuf, (size_t)q * cells * sizeof(unsigned)));
    hipLaunchKernelGGL(k_fill<unsigned>, blocks_capped((size_t)q * cells), 256, 0, st, tbuf, (size_t)q * cells, T_NONE);
  }
  uint8_t* solid = nullptr;
  if (method != XLBHIP_MESH_RAY) XLB_HIP(scratch.alloc(&solid, cells));
  uint8_t* bcp = static_cast<uint8_t*>(bcm->data);
  uint32_t* mp = static_cast<uint32_t*>(miss->data);
  const FieldView dview = view(dist);
  return by_lattice(lattice, [&](auto L) {
    using LL = decltype(L);
    if (method == XLBHIP_MESH_RAY) {
      launch_flat(dist ? k_mesh_ray<LL, true> : k_mesh_ray<LL, false>, nt, st, dv, n_triangles, bcp, mp, tbuf, d, bc_id);
      if (dist) launch_flat(k_mesh_weights_ray<LL>, cells, st, tbuf, dview, d);
    } else if (method == XLBHIP_MESH_WINDING) {
      XLB_HIP(hipMemsetAsync(solid, 0, cells, st));
      int b0[3], nb[3];
      const int ext[3] = {d.nx, d.ny, d.nz};
      for (int a = 0; a < 3; ++a) {
        b0[a] = std::max(0, (int)floorf(lo[a]) - 1);
        nb[a] = std::min(ext[a] - 1, (int)floorf(hi[a]) + 1) - b0[a] + 1;
      }
      launch_flat(k_mesh_winding, (size_t)nb[0] * nb[1] * nb[2], st, dv, n_triangles, solid, d, b0[0], b0[1], b0[2], nb[0], nb[1], nb[2]);
      launch_flat(k_mesh_winding_rays<LL>, nt, st, dv, n_triangles, solid, tbuf, d);
      launch_flat(k_mesh_winding_tag<LL>, cells, st, solid, tbuf, bcp, mp, dview, d, bc_id);
    } else {
      if (method == XLBHIP_MESH_AABB) {
        XLB_HIP(hipMemsetAsync(solid, 0, cells, st));
        launch_flat(k_mesh_solid, nt, st, dv, n_triangles, solid, d.nx, d.ny, d.nz, 0);
      } else {  // AABB_CLOSE: voxelise on a padded grid, close the gaps (dilate, erode), crop
        const int h = close_voxels, pad = 2 * h;
        const int px = d.nx + 2 * pad, py = d.ny + 2 * pad, pz = d.nz + 2 * pad;
        const size_t pcells = (size_t)px * py * pz;
        uint8_t *pa = nullptr, *pb = nullptr;
        XLB_HIP(scratch.alloc(&pa, pcells));
        XLB_HIP(scratch.alloc(&pb, pcells));
        XLB_HIP(hipMemsetAsync(pa, 0, pcells, st));
        launch_flat(k_mesh_solid, nt, st, dv, n_triangles, pa, px, py, pz, pad);
        launch_flat(k_morph, pcells, st, pa, pb, px, py, pz, h, 1);
        launch_flat(k_morph, pcells, st, pb, pa, px, py, pz, h, 0);
        launch_flat(k_crop, cells, st, pa, solid, d, py, pz, pad);
      }
      launch_flat(k_mesh_classify<LL>, cells, st, solid, bcp, mp, d, bc_id);
      if (dist) {
        launch_flat(k_mesh_close_rays<LL>, nt, st, dv, n_triangles, solid, bcp, tbuf, d, bc_id);
        launch_flat(k_mesh_weights_close<LL>, cells, st, solid, bcp, tbuf, dview, d, bc_id);
      }
    }
    if (method == XLBHIP_MESH_RAY || method == XLBHIP_MESH_WINDING)  // (k_mesh_classify resolves the out-of-box directions itself)
      launch_flat(k_mesh_resolve<LL>, cells, st, bcp, mp, d, bc_id);
    XLB_HIP(hipGetLastError());
    return 0;
  });
}

extern "C" {

int xlbhip_build_masks(xlbhip_ctx* c, int lattice, int n_bc, const int32_t* ids, const int32_t* const* tag_idx, const int64_t* tag_count,
                       const int32_t* const* solid_idx, const int64_t* solid_count, const int32_t gshape[3], int x_offset,
                       xlbhip_field* bcm, xlbhip_field* miss) {
  XLB_REQUIRE(c && bcm && miss && gshape, "null argument");
  XLB_REQUIRE(bcm->dtype == XLBHIP_U8 && bcm->card == 1, "bc_mask must be a (1,...) uint8 field");
  XLB_REQUIRE(miss->dtype == XLBHIP_MISSING && miss->card == lattice_q(lattice), "missing_mask must be a (q,...) missing field");
  XLB_REQUIRE(same_grid(bcm, miss) && bcm->halo == miss->halo, "masks live on different grids");
  XLB_REQUIRE(gshape[1] == bcm->ny && gshape[2] == bcm->nz && x_offset >= 0 && x_offset + bcm->nx <= gshape[0],
              "slab (offset %d, nx %d) does not fit global shape (%d,%d,%d)", x_offset, bcm->nx, gshape[0], gshape[1], gshape[2]);
  XLB_REQUIRE(n_bc == 0 || (ids && tag_idx && tag_count), "null bc arrays");
  touch(bcm);
  touch(miss);
  hipStream_t st = c->stream;
  const Dims d = dims(bcm);
  const size_t plane = (size_t)d.ny * d.nz;
  // every exit releases the temporaries (the stream is drained first: copies may still read them)
  DeviceScratch scratch(st);
  // solid scratch with one ghost plane per side
  uint8_t* solid = nullptr;
  const size_t solid_bytes = (size_t)(d.nx + 2) * plane;
  XLB_HIP(scratch.alloc(&solid, solid_bytes));
  XLB_HIP(hipMemsetAsync(solid, 0, solid_bytes, st));
  uint8_t* bc_base = static_cast<uint8_t*>(bcm->data) + (size_t)bcm->halo * plane;  // interior plane 0
  for (int i = 0; i < n_bc; ++i) {
    XLB_REQUIRE(ids[i] >= 1 && ids[i] <= 255, "bc id %d out of range 1..255", ids[i]);
    if (solid_idx && solid_idx[i] && solid_count && solid_count[i] > 0) {
      const int64_t n = solid_count[i];
      int32_t* dv = nullptr;
      XLB_HIP(scratch.alloc(&dv, (size_t)n * 3 * sizeof(int32_t)));
      XLB_HIP(hipMemcpyAsync(dv, solid_idx[i], (size_t)n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, st));
      launch_flat(k_scatter_u8, (size_t)n, st, solid, dv, n, (uint8_t)1, x_offset - 1, x_offset + d.nx + 1, d.ny, d.nz);
    }
    if (tag_count[i] > 0) {
      const int64_t n = tag_count[i];
      int32_t* dv = nullptr;
      XLB_HIP(scratch.alloc(&dv, (size_t)n * 3 * sizeof(int32_t)));
      XLB_HIP(hipMemcpyAsync(dv, tag_idx[i], (size_t)n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, st));
      launch_flat(k_scatter_u8, (size_t)n, st, bc_base, dv, n, (uint8_t)ids[i], x_offset, x_offset + d.nx, d.ny, d.nz);
    }
  }
  // stream the (old | solid | outside) marks: missing'[l, x] = marks[l, x - c_l]
  uint32_t* old = nullptr;
  const size_t mbytes = miss->cells_with_halo() * sizeof(uint32_t);
  XLB_HIP(scratch.alloc(&old, mbytes));
  XLB_HIP(hipMemcpyAsync(old, miss->data, mbytes, hipMemcpyDeviceToDevice, st));
  const size_t n = bcm->cells();
  return by_lattice(lattice, [&](auto L) {
    launch_flat(k_missing<decltype(L)>, n, st, (uint32_t*)miss->data, old, solid, d, miss->halo, gshape[0], x_offset);
    XLB_HIP(hipGetLastError());
    return 0;
  });
}

int xlbhip_mesh_mask(xlbhip_ctx* c, int lattice, int method, int bc_id, int64_t n_triangles, const float* vertices, int close_voxels,
                                xlbhip_field* bcm, xlbhip_field* miss, xlbhip_field* dist) {
  return mesh_mask(c, lattice, method, bc_id, n_triangles, vertices, close_voxels, bcm, miss, dist);
}

// The two methods without distances under their first names.  Like every method, they return after the checks when the mesh has no
// triangle (they once still ran their per-voxel pass over the fields then).
int xlbhip_mesh_mask_aabb(xlbhip_ctx* c, int lattice, int bc_id, int64_t n_triangles, const float* vertices, xlbhip_field* bcm,
                                     xlbhip_field* miss) {
  return mesh_mask(c, lattice, XLBHIP_MESH_AABB, bc_id, n_triangles, vertices, 0, bcm, miss, nullptr);
}
int xlbhip_mesh_mask_ray(xlbhip_ctx* c, int lattice, int bc_id, int64_t n_triangles, const float* vertices, xlbhip_field* bcm,
                                    xlbhip_field* miss) {
  return mesh_mask(c, lattice, XLBHIP_MESH_RAY, bc_id, n_triangles, vertices, 0, bcm, miss, nullptr);
}

}  // extern "C"
