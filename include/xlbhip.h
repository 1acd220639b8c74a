/*
 * xlbhip.h — C ABI of the MI355X-native LBM stepper (libxlbhip.so).
 *
 * This is the drop-in boundary for the per-timestep hot path of hsalehipour/XLB.
 * The reference has no native code: its "FFI" for this path is the set of Python
 * methods registered with @Operator.register_backend(ComputeBackend.X)
 * (reference xlb/operator/operator.py:74-133).  Every entry point below names the
 * reference method(s) whose body a `hip_implementation` replaces; the ctypes stub a
 * maintainer would add is shown in INTEGRATION.md and shipped in xlb_amd/_lib.py.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types.
 *  - every call returns 0 on success, non-zero on failure; the message is available
 *    from xlbhip_last_error() (thread-local).  The Python shim turns it into an
 *    exception, mirroring the reference's exception-only error model
 *    (operator.py:128-133).
 *  - calls only ENQUEUE work on the context's compute stream (asynchronous, like
 *    wp.launch in the reference) except *_download, *_sync and *_timed.
 *  - host arrays are C-order (cardinality, nx, ny, nz), population index slowest,
 *    last spatial axis fastest — the reference layout (xlb/grid/warp_grid.py:26,
 *    xlb/grid/jax_grid.py:44-46).  2-D grids (nx, ny) are passed as (1, nx, ny):
 *    the lattice's two components then act on the last two axes.
 */
#ifndef XLBHIP_H
#define XLBHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xlbhip_ctx xlbhip_ctx;
typedef struct xlbhip_field xlbhip_field;
typedef struct xlbhip_stepper xlbhip_stepper;
typedef struct xlbhip_ibm xlbhip_ibm;
typedef struct xlbhip_stats xlbhip_stats;
typedef struct xlbhip_scalar xlbhip_scalar;
typedef struct xlbhip_adjoint xlbhip_adjoint;
typedef struct xlbhip_multiphase xlbhip_multiphase;
typedef struct xlbhip_multicomponent xlbhip_multicomponent;

/* element types of a field; mirrors Precision in xlb/precision_policy.py:13-54 */
enum {
  XLBHIP_F64 = 0,
  XLBHIP_F32 = 1,
  XLBHIP_F16 = 2,
  XLBHIP_U8 = 3,
  XLBHIP_BOOL = 4,      /* one byte per element, 0/1 */
  XLBHIP_MISSING = 5    /* missing_mask: host view (q,nx,ny,nz) u8 0/1; device: one u32 bit-set per cell */
};

/* velocity sets; xlb/velocity_set/{d2q9,d3q19,d3q27}.py */
enum { XLBHIP_D2Q9 = 0, XLBHIP_D3Q19 = 1, XLBHIP_D3Q27 = 2 };

/* collision models; xlb/operator/stepper/nse_stepper.py:78-84 */
enum {
  XLBHIP_BGK = 0,
  XLBHIP_KBC = 1,
  XLBHIP_SMAGORINSKY_LES_BGK = 2, /* xlb/operator/collision/smagorinsky_les_bgk.py:44-60 (section 8f rank 3) */
  /* regularised BGK (not in the reference): fneq rebuilt from its second Hermite moment (Latt & Chopard 2006), and with the
   * third-order moments that follow from it recursively (Malaspinas 2015).  Single-step kernel, FP32FP32 / FP64FP64 / FP64FP32 */
  XLBHIP_REGULARIZED_BGK = 3,
  XLBHIP_RECURSIVE_REGULARIZED_BGK = 4
};

/* boundary-condition kinds (in scope: SURVEY.md section 8 rows a7-a9, + DoNothing) */
enum {
  XLBHIP_BC_EQUILIBRIUM = 1,  /* bc_equilibrium.py:72-80   (post-streaming) */
  XLBHIP_BC_HALFWAY_BB = 2,   /* bc_halfway_bounce_back.py:116-134 (post-streaming) */
  XLBHIP_BC_FULLWAY_BB = 3,   /* bc_fullway_bounce_back.py:50-56   (post-collision) */
  XLBHIP_BC_DO_NOTHING = 4,   /* bc_do_nothing.py:50-54    (post-streaming) */
  /* SURVEY.md section 8f rank 1 — inlet/outlet family with CONSTANT prescribed values (JAX semantics:
   * the value lives in the BC object, bc_zouhe.py:120-121, not in the f_1 aux encoding) */
  XLBHIP_BC_ZOUHE_VELOCITY = 5,        /* bc_zouhe.py:218-304, values[0..2] = velocity (3-component internal form) */
  XLBHIP_BC_ZOUHE_PRESSURE = 6,        /* values[0] = density */
  XLBHIP_BC_REGULARIZED_VELOCITY = 7,  /* bc_regularized.py:78-137 */
  XLBHIP_BC_REGULARIZED_PRESSURE = 8,
  /* ExtrapolationOutflowBC, JAX branch (bc_extrapolation_outflow.py:98-145): streaming step = the missing populations
   * take the cell's own opposite PRE-stream population; after the collision the outgoing populations are overwritten
   * with cs * f_post_stream(neighbour behind the face) + (1 - cs) * f_post_stream(cell) ("auxiliary data", read back by
   * the next step).  values[0..2] = outward face normal (internal 3-component form), values[3] = cs = 1/sqrt(3) and
   * values[4] = 1 - cs, both rounded in the compute dtype by the host side. */
  XLBHIP_BC_EXTRAPOLATION_OUTFLOW = 9,
  /* HybridBC (bc_hybrid.py:254-358; kernel backends only in the reference), 3-D lattices.  values[0..2] = wall velocity
   * (3-component internal form), values[3] != 0: moving-wall treatment, values[4] != 0: use the wall-distance weights the
   * mesh masker produced (xlbhip_stepper_set_bc_distances) */
  XLBHIP_BC_HYBRID_BB_REGULARIZED = 10,  /* interpolated bounce-back + regularisation (bc_hybrid.py:256-290) */
  XLBHIP_BC_HYBRID_BB_GRADS = 11,        /* interpolated bounce-back + Grad's approximation (:292-326) */
  XLBHIP_BC_HYBRID_NEQ_REGULARIZED = 12, /* non-equilibrium bounce-back + regularisation (:328-358) */
  /* halfway bounce-back whose wall velocity is a per-cell table (xlbhip_stepper_set_bc_profile): the reference's
     HalfwayBounceBackBC(profile=...) of the kernel backends, bc_halfway_bounce_back.py:144-169 + helper_functions_bc.py:230-250 */
  XLBHIP_BC_HALFWAY_BB_PROFILE = 13
};

/* One boundary condition as the stepper sees it.  `values` holds, in COMPUTE
 * precision widened to double (exactly representable): for EQUILIBRIUM the q
 * populations feq(rho0,u0); for HALFWAY_BB the q moving-wall terms
 * 6 w_l (c_l . u_wall) (all zero for no-slip).  Computed on the host by the
 * Python operator exactly as the reference's JAX branch does. */
typedef struct {
  int32_t id;        /* value in bc_mask, 1..253; boundary_condition_registry.py:16-27 */
  int32_t kind;      /* XLBHIP_BC_* */
  double values[27];
} xlbhip_bc_desc;

/* ---- context ------------------------------------------------------------ */
/* replaces: xlb.init backend branch, xlb/default_config.py:78-100 */
int xlbhip_create(int device, xlbhip_ctx** out);
int xlbhip_destroy(xlbhip_ctx* ctx);
int xlbhip_sync(xlbhip_ctx* ctx);                 /* wp.synchronize(), mlups_3d.py:230 */
const char* xlbhip_last_error(void);
int xlbhip_device_info(xlbhip_ctx* ctx, char* name, int name_len, int* compute_units, uint64_t* hbm_bytes);
/* tuning knobs (kernel variant selection etc.); unknown keys are an error.  The ones with semantics:
 *   exact_math      0 (default): fp64-compute D3Q27 KBC runs the tolerance-graded fast collision (rounding-level
 *                   differences from the bit-exact build, <= 4e-16 measured; north-star tolerance 1e-6); 1: bit-exact builds only
 *   fast_bgk        1 (default 0): the two-step kernel uses the tolerance-graded fast BGK body (rounding-level differences,
 *                   <= 3e-7 measured over 10 steps in fp32; +2-4 %); ignored with exact_math=1
 *   fuse2           xlbhip_run* pair their steps through the two-step kernel: 0 never, 1 where eligible and the work
 *                   items fill the chip, 2 wherever eligible
 *   external_halo   1: the caller refills the ghost planes before every xlbhip_step / xlbhip_step2 (host-staged transports)
 *   overlap         0: no overlap of the halo exchange with the interior launch (measurement)
 * Pure tuning (results identical): vec, nt_store, nt_load, plane_pad_bytes (at field creation), block_threads, block_tz,
 * xcd_swizzle, fuse2_xseg / _lpt / _xcd / _clean / _xcap / _shift / _tile / _cus (csrc/api.hip: xlbhip_create). */
int xlbhip_set_option(xlbhip_ctx* ctx, const char* key, int64_t value);
int xlbhip_get_option(xlbhip_ctx* ctx, const char* key, int64_t* value);

/* lattice tables as compiled into the kernels, for cross-checking against the
 * Python VelocitySet (velocity_set.py:63-83): c is (3,q) row-major (2-D sets have a
 * leading zero row), w (q), opp (q), cc (q,6) */
int xlbhip_lattice_info(int lattice, int* d, int* q, int32_t* c, double* w, int32_t* opp, int32_t* cc);

/* ---- fields ------------------------------------------------------------- */
/* replaces: WarpGrid.create_field, xlb/grid/warp_grid.py:17-35.
 * halo = number of ghost x-planes on each side: 0, or 1 / 2 for slab-decomposed runs (2 lets xlbhip_run fuse
 * two steps per pass across rank boundaries). */
int xlbhip_field_create(xlbhip_ctx* ctx, int cardinality, int nx, int ny, int nz, int dtype, int halo,
                        double fill_value, xlbhip_field** out);
int xlbhip_field_destroy(xlbhip_field* f);
int xlbhip_field_fill(xlbhip_field* f, double value);
int xlbhip_field_copy(xlbhip_field* dst, const xlbhip_field* src);            /* wp.copy, nse_stepper.py:124 */
/* streaming copy by a plain kernel (4 or 16 bytes per lane): bandwidth yardstick and the
 * known-byte-count calibration of the rocprofv3 FETCH_SIZE / WRITE_SIZE counters (tools/) */
int xlbhip_field_copy_kernel(xlbhip_field* dst, const xlbhip_field* src, int bytes_per_lane);
/* the same copy with the launch shape of the two-step kernel: one 704-thread block per CU, (8 x 64) tiles marching along x, a plane's
 * stores and pulls separated by a barrier — the second yardstick of bench.py (roofline.pattern_copy_*); 4-byte elements, ny % 8 == 0,
 * nz % 64 == 0.  Measurement only: nothing in the reference corresponds (its harness times the step alone, examples/performance/mlups_3d.py:225-242) */
int xlbhip_field_copy_tiles(xlbhip_field* dst, const xlbhip_field* src);
int xlbhip_field_upload(xlbhip_field* f, const void* host, size_t host_bytes);   /* interior only */
int xlbhip_field_download(const xlbhip_field* f, void* host, size_t host_bytes); /* interior only; synchronous */
/* one x-plane of one population, addressed by STORAGE plane (0 .. nx + 2 halo - 1, ghosts included):
 * host-staged halo transports and tests */
int xlbhip_field_plane_download(const xlbhip_field* f, int population, int storage_plane, void* host, size_t bytes);
int xlbhip_field_plane_upload(xlbhip_field* f, int population, int storage_plane, const void* host, size_t bytes);
/* Tell the library that somebody wrote the field behind its back — through a zero-copy alias (Field.__dlpack__ /
 * __cuda_array_interface__, the replacement of utils.py:340-447's ToJAX): bumps the contents version that the stepper's
 * per-mask caches (meta words, clean-item flags, end-plane scan) are keyed on */
int xlbhip_field_touch(xlbhip_field* f);
/* (backend-internal, no reference counterpart) free / total device memory (hipMemGetInfo): the Python stepper refuses to pair reference-style calls when the
 * temporary third field a read of the virtual f(t+1) needs would not fit */
int xlbhip_mem_info(xlbhip_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);
int xlbhip_field_info(const xlbhip_field* f, int* cardinality, int* nx, int* ny, int* nz, int* dtype, int* halo,
                      uint64_t* plane_stride_elems, void** device_ptr);

/* ---- whole-field operators (kernel-backend out-of-place style) ---------- */
/* Stream()(f_0, f_1): stream.py:96-125 */
int xlbhip_stream(xlbhip_ctx* ctx, int lattice, const xlbhip_field* f_src, xlbhip_field* f_dst);
/* QuadraticEquilibrium()(rho, u, f): quadratic_equilibrium.py:23-30, :91-103 */
int xlbhip_equilibrium(xlbhip_ctx* ctx, int lattice, int compute_dtype, const xlbhip_field* rho, const xlbhip_field* u,
                       xlbhip_field* f);
/* Macroscopic()(f, rho, u): macroscopic.py:21-26, :57-64 */
int xlbhip_macroscopic(xlbhip_ctx* ctx, int lattice, int compute_dtype, const xlbhip_field* f, xlbhip_field* rho,
                       xlbhip_field* u);
/* SecondMoment()(f, pi): second_moment.py:35-55 */
int xlbhip_second_moment(xlbhip_ctx* ctx, int lattice, int compute_dtype, const xlbhip_field* f, xlbhip_field* pi);
/* as xlbhip_apply_bc for a Zou-He / Regularized BC with per-cell prescribed values (see xlbhip_stepper_set_bc_profile) */
int xlbhip_apply_bc_profile(xlbhip_ctx* ctx, int lattice, int compute_dtype, const xlbhip_bc_desc* bc, const xlbhip_field* f_pre,
                            xlbhip_field* f_post, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, int64_t n,
                            const uint32_t* storage_cells, const double* values);
/* MomentumTransfer(no_slip_bc)(f_0, f_1, bc_mask, missing_mask) -> net force on the solid behind the BC
 * (force/momentum_transfer.py:167-205, JAX; f_0 = post-collision populations, i.e. the field a step returned).
 * The BC must be a halfway or fullway bounce-back; force_out = (F_x, F_y, F_z) in the internal 3-component form,
 * the sum over THIS rank's cells (slab runs add the ranks' vectors).  Synchronous. */
int xlbhip_momentum_transfer(xlbhip_ctx* ctx, int lattice, int compute_dtype, const xlbhip_bc_desc* no_slip_bc, const xlbhip_field* f_0,
                             const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double force_out[3]);
/* Vorticity()(u, bc_mask, vorticity, vorticity_magnitude): postprocess/vorticity.py:30-93 (3-D; cells one layer inside the
 * box whose six face neighbours are all fluid get the curl of u by central differences and its magnitude; every other cell of
 * the outputs is left untouched).  Arithmetic in u's dtype (fp32 / fp64). */
int xlbhip_vorticity(xlbhip_ctx* ctx, const xlbhip_field* u, const xlbhip_field* bc_mask, xlbhip_field* vorticity,
                     xlbhip_field* vorticity_magnitude);
/* GridToPoint()(grid, points, point_values): postprocess/grid_to_point.py:28-104 — trilinear interpolation of component 0 of a
 * 3-D field at n points (host float[n][3] in, host values[n] in the field's dtype out; synchronous).  Unlike the reference,
 * points whose surrounding cube leaves the field are an error instead of an out-of-bounds read. */
int xlbhip_grid_to_point(xlbhip_ctx* ctx, const xlbhip_field* grid, int64_t n, const float* points, void* point_values);
/* QCriterion()(u, bc_mask, norm_mu, q): postprocess/q_criterion.py:36-139; Q = (|Omega|^2 - |S|^2) / 2, same cells */
int xlbhip_q_criterion(xlbhip_ctx* ctx, const xlbhip_field* u, const xlbhip_field* bc_mask, xlbhip_field* norm_mu, xlbhip_field* q);
/* BGK()/KBC()(f, feq, fout, omega): bgk.py:27-32,:78-91; kbc.py:40-79.  The regularised collisions take rho and u from f */
int xlbhip_collide(xlbhip_ctx* ctx, int lattice, int collision, int compute_dtype, const xlbhip_field* f,
                   const xlbhip_field* feq, xlbhip_field* fout, double omega);
/* bc(f_pre, f_post, bc_mask, missing_mask) -> f_post (in place): boundary_condition.py:146-180 */
int xlbhip_apply_bc(xlbhip_ctx* ctx, int lattice, int compute_dtype, const xlbhip_bc_desc* bc, const xlbhip_field* f_pre,
                    xlbhip_field* f_post, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask);

/* ---- boundary masker ----------------------------------------------------- */
/* replaces: IndicesBoundaryMasker (JAX semantics), indices_boundary_masker.py:73-143.
 * For BC i: tag_idx[i] is an int32 (3, tag_count[i]) row-major array of GLOBAL cell
 * indices that receive bc_ids[i] in bc_mask (later BCs overwrite earlier ones);
 * solid_idx[i] (may be NULL / count 0) are GLOBAL indices whose every population is
 * marked missing before the mask is streamed (the "interior geometry" branch,
 * :107-121).  global_shape is the whole domain; x_offset is the global x index of this
 * rank's first interior plane (the start_index of :76,:106).  Existing contents of
 * missing_mask are streamed too, as in the reference. */
int xlbhip_build_masks(xlbhip_ctx* ctx, int lattice, int n_bc, const int32_t* bc_ids, const int32_t* const* tag_idx,
                       const int64_t* tag_count, const int32_t* const* solid_idx, const int64_t* solid_count,
                       const int32_t global_shape[3], int x_offset, xlbhip_field* bc_mask, xlbhip_field* missing_mask);

/* MeshMaskerAABB()(bc, f_1, bc_mask, missing_mask): boundary_masker/aabb.py:38-100 + mesh_boundary_masker.py:62-245.
 * vertices = n_triangles x 3 corners x (x, y, z) in lattice units (voxel i spans [i, i+1]), fully inside the domain.
 * Voxels the surface passes through become BC_SOLID (255); fluid voxels next to one get bc_id and the missing bits of the
 * directions pulled out of it; voxels of bc_id also miss the directions pulled from outside the box.  Existing mask
 * contents are kept (other BCs' ids, earlier solid voxels).  Single-rank fields.  Synchronous. */
int xlbhip_mesh_mask_aabb(xlbhip_ctx* ctx, int lattice, int bc_id, int64_t n_triangles, const float* vertices, xlbhip_field* bc_mask,
                          xlbhip_field* missing_mask);

/* MeshMaskerRay()(bc, f_1, bc_mask, missing_mask): boundary_masker/ray.py:38-76 — a voxel whose lattice link along c_l
 * (from the voxel centre, length |c_l|) crosses the surface gets bc_id and missing[opp l]; no solid voxels are marked.
 * Same conventions as xlbhip_mesh_mask_aabb. */
int xlbhip_mesh_mask_ray(xlbhip_ctx* ctx, int lattice, int bc_id, int64_t n_triangles, const float* vertices, xlbhip_field* bc_mask,
                         xlbhip_field* missing_mask);

/* Mesh voxelisation methods (xlb/operator/boundary_masker/mesh_voxelization_method.py:13-55) */
enum { XLBHIP_MESH_AABB = 1, XLBHIP_MESH_RAY = 2, XLBHIP_MESH_AABB_CLOSE = 3, XLBHIP_MESH_WINDING = 4 };

/* All mesh maskers behind one entry, with the wall distances ("weights") curved-wall BCs interpolate with.  Replaces the
 * warp_implementation of MeshMaskerAABB (aabb.py:38-100), MeshMaskerRay (ray.py:38-101), MeshMaskerWinding
 * (winding.py:19-115) and MeshMaskerAABBClose (aabb_close.py:26-365; `close_voxels` = half width of the (2h+1)^3
 * structuring element of the morphological close) — masker(bc, distances, bc_mask, missing_mask).
 * `distances`: NULL, or a (q, nx, ny, nz) fp32 field that receives, like the reference's `distances` argument,
 *   RAY        distances[l]     = t / |c_l|            at a boundary voxel whose link along c_l crosses the surface at t
 *   WINDING    distances[opp l] = (|c_l| - t) / |c_l|  at the fluid neighbour (+c_l) of a solid voxel
 *   AABB_CLOSE distances[l]     = (t - |c_l| / 2) / |c_l| within 1.5 |c_l|, 1.0 without a hit, for links ending in a solid voxel
 * (untouched elsewhere).  The Warp BVH queries are replaced by exhaustive closest-hit / exact winding-number loops over
 * the triangles: O(voxels near the surface x triangles near the voxel) for the rays, O(bounding-box voxels x triangles)
 * for the winding number. */
int xlbhip_mesh_mask(xlbhip_ctx* ctx, int lattice, int method, int bc_id, int64_t n_triangles, const float* vertices, int close_voxels,
                     xlbhip_field* bc_mask, xlbhip_field* missing_mask, xlbhip_field* distances);

/* out[i][l] = field[l][cells[i]] for n interior linear cell indices ((x * ny + y) * nz + z), element type of the field;
 * blocking.  How boundary-cell data (e.g. the distances above) reach the host without downloading whole fields. */
int xlbhip_field_gather(const xlbhip_field* f, int64_t n, const uint32_t* cells, void* out, size_t bytes);

/* ---- the stepper (the hot path) ------------------------------------------ */
/* replaces: IncompressibleNavierStokesStepper._construct_warp + launch,
 * nse_stepper.py:335-476, with the JAX step order of :237-282. */
int xlbhip_stepper_create(xlbhip_ctx* ctx, int lattice, int collision, int compute_dtype, int store_dtype, int n_bc,
                          const xlbhip_bc_desc* bcs, xlbhip_stepper** out);
int xlbhip_stepper_destroy(xlbhip_stepper* s);
/* Per-cell prescribed values of a Zou-He / Regularized BC built with a profile (bc_zouhe.py:122-124,225-232: the
 * array the profile returns, broadcast over the grid, evaluated at the BC's cells): storage_cells[i] =
 * ((x_local + halo) * ny + y) * nz + z of a cell of bc_id on this rank, values[3 i .. 3 i + 2] = its velocity vector
 * (internal 3-component form) or its density in values[3 i].  Replaces the kernel backends' encoding of these values in
 * f_1 (helper_functions_bc.py:371-499, nse_stepper.py:398-425).  May be called once per BC; tables are merged. */
int xlbhip_stepper_set_bc_profile(xlbhip_stepper* s, int bc_id, int64_t n, const uint32_t* storage_cells, const double* values);

/* Wall-distance weights of HybridBC cells: n storage cell indices (as for set_bc_profile) and q floats each, in the
 * layout of the mesh masker's `distances` (the weight of missing direction l in slot opp l).  The reference keeps them
 * in f_1 and recovers them every step (bc_hybrid.py:207-214, nse_stepper.py:398-425); here they live in a sorted table
 * that the boundary lanes of the step kernel search.  Calls accumulate (one per mesh BC). */
int xlbhip_stepper_set_bc_distances(xlbhip_stepper* s, int64_t n, const uint32_t* storage_cells, const float* weights);
/* MomentumTransfer for a HybridBC or a profile wall of this stepper (the kernel backends' path, force/momentum_transfer.py:225-262 with
 * FetchPopulations :75-92): f_post_stream = that BC applied to (own populations of f_0, populations pulled from f_0) with the stepper's
 * wall-distance and wall-velocity tables; force[3] in the internal 3-component form.  Fields without ghost planes. */
int xlbhip_stepper_momentum_transfer(xlbhip_stepper* s, int bc_id, const xlbhip_field* f_0, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask,
                                     double force[3]);
/* Time-dependent wall velocities: HalfwayBounceBackBC / HybridBC whose profile is profile(index, timestep) (bc_halfway_bounce_back.py:147-155,
 * bc_hybrid.py:163-172 and :228-239; the stepper passes its timestep to every BC functional, nse_stepper.py:370-378).  The BC's storage
 * cells (as for set_bc_profile) are declared ONCE; they become entries of the stepper's profile table whose values arrive per timestep.
 * Calls accumulate (one per BC); the declaration order of all calls is the order of the values of xlbhip_stepper_stage_bc_profiles. */
int xlbhip_stepper_set_bc_profile_cells(xlbhip_stepper* s, int bc_id, int64_t n, const uint32_t* storage_cells);
/* Number of per-timestep tables the stepper keeps resident (a ring of device slots sized from a byte budget, 4 .. 64, even); 0 without
 * time-dependent cells.  At most this many timesteps can be staged by one call. */
int xlbhip_stepper_profile_slots(xlbhip_stepper* s, int* slots);
/* The wall velocities of the timesteps t_first .. t_first + n_steps - 1: values = n_steps rows, each row 3 doubles (internal
 * 3-component form, already rounded to the compute dtype) per declared cell in declaration order.  Each row is scattered into a full
 * image of the table (the static Zou-He / profile entries stay) and copied into the next slot of the ring through a pinned host buffer
 * by hipMemcpyAsync on the compute stream; the host waits only for the previous copy out of the same pinned row.  A timestep that is
 * staged again replaces its older image.  Every launch of a step from timestep t (xlbhip_step, xlbhip_step2: t and t + 1, xlbhip_run*:
 * t0 .. t0 + n - 1) reads t's image and fails, before enqueuing anything, when it is not resident. */
int xlbhip_stepper_stage_bc_profiles(xlbhip_stepper* s, int64_t t_first, int64_t n_steps, const double* values);
/* xlbhip_stepper_momentum_transfer with the wall velocities of `timestep` (force/momentum_transfer.py:88 evaluates the wall at timestep
 * 0, which is what xlbhip_stepper_momentum_transfer does); a time-dependent wall needs that timestep staged. */
int xlbhip_stepper_momentum_transfer_at(xlbhip_stepper* s, int bc_id, int64_t timestep, const xlbhip_field* f_0, const xlbhip_field* bc_mask,
                                        const xlbhip_field* missing_mask, double force[3]);
/* ForcedCollision with the exact-difference scheme (forced_collision.py:44-50, exact_difference_force.py:61-83):
 * force[3] in the internal 3-component form; NULL switches forcing off */
int xlbhip_stepper_set_force(xlbhip_stepper* s, const double* force);
/* Smagorinsky constant of XLBHIP_SMAGORINSKY_LES_BGK (default 0.17, smagorinsky_les_bgk.py:36) */
int xlbhip_stepper_set_smagorinsky(xlbhip_stepper* s, double coef);
/* one step: reads f_src, writes f_dst (caller swaps); omega is cast to compute dtype (bgk.py:31); timestep selects the staged wall
 * velocities of time-dependent profiles (xlbhip_stepper_stage_bc_profiles) and is ignored otherwise */
int xlbhip_step(xlbhip_stepper* s, const xlbhip_field* f_src, xlbhip_field* f_dst, const xlbhip_field* bc_mask,
                const xlbhip_field* missing_mask, double omega, int64_t timestep);
/* n_steps steps with the A/B swap done natively; the result is in f_a if n_steps is even, else f_b */
int xlbhip_run(xlbhip_stepper* s, xlbhip_field* f_a, xlbhip_field* f_b, const xlbhip_field* bc_mask,
               const xlbhip_field* missing_mask, double omega, int64_t first_timestep, int64_t n_steps);
/* TWO steps in one pass (f(t) in f_src -> f(t+2) in f_dst, f(t+1) never reaches HBM): what xlbhip_run uses for
 * pairs of steps where xlbhip_step2_eligible() says 1 (D3Q19 BGK fp32, basic BCs, ny % 8 == nz % 64 == 0, fields
 * with 0 or 2 ghost planes, enough tiles to fill the chip).  Same arithmetic in the same order as two xlbhip_step
 * calls (nse_stepper.py:237-282 twice): bit-identical results.  With the "external_halo" option the caller has
 * filled f_src's ghost planes to depth 2 and the ghost planes of the masks to depth 1. */
int xlbhip_step2_eligible(xlbhip_stepper* s, const xlbhip_field* f_src, xlbhip_field* f_dst, const xlbhip_field* bc_mask,
                          const xlbhip_field* missing_mask);
int xlbhip_step2(xlbhip_stepper* s, const xlbhip_field* f_src, xlbhip_field* f_dst, const xlbhip_field* bc_mask,
                 const xlbhip_field* missing_mask, double omega, int64_t timestep);
/* Read-only report of the two-step launches the next pass f_src -> f_dst would make (same arguments as xlbhip_step2_eligible, which
 * must say 1).  Nothing is stepped and no field changes; the meta words, the tile order and the clean flags are built through the
 * caches a pass uses, so the report is what the next xlbhip_run / xlbhip_step2 on these fields and options launches.  Covers fields
 * without ghost planes, the slab launches of fields with two (interior + two edges, or whole) and the middle launch of the
 * inlet / outlet path (the end planes' single steps are not listed).  int32 words: [0] = launches; per launch x_begin, x_count,
 * effective x segments, effective cap (planes of the thin end segments, 0 = uniform cuts), tile_ty, tile_tz, tile_oy, tile_oz (the
 * tiling's shift), strips mode (0 none, 2 write, 3 read + write, 4 row-aligned lanes only; as if the strip buffers can be allocated),
 * items; then per item, in block order: tile index (ty * tiles_z + tz), x_lo, x_hi (planes [x_lo, x_hi)) and the clean flag the block
 * reads (1 = it runs the body without boundary conditions; 0 also where the launch has no flags).  *n_words = words of the report;
 * they are written to out when capacity >= *n_words (call with capacity 0 to size the buffer). */
int xlbhip_step2_plan(xlbhip_stepper* s, const xlbhip_field* f_src, xlbhip_field* f_dst, const xlbhip_field* bc_mask,
                      const xlbhip_field* missing_mask, int32_t* out, int64_t capacity, int64_t* n_words);
/* as xlbhip_run without the placement contract: every pair of steps may be fused (xlbhip_run keeps an even number of fused
 * passes and finishes with single steps to honour its contract); *result_in_b = 1 when the result is in f_b */
int xlbhip_run_any(xlbhip_stepper* s, xlbhip_field* f_a, xlbhip_field* f_b, const xlbhip_field* bc_mask,
                   const xlbhip_field* missing_mask, double omega, int64_t first_timestep, int64_t n_steps, int* result_in_b);
/* the same loop bracketed by HIP events on the compute stream; returns device ms for the whole loop.
 * result_in_b == NULL: xlbhip_run's placement; otherwise as xlbhip_run_any */
int xlbhip_run_timed(xlbhip_stepper* s, xlbhip_field* f_a, xlbhip_field* f_b, const xlbhip_field* bc_mask,
                     const xlbhip_field* missing_mask, double omega, int64_t first_timestep, int64_t n_steps,
                     float* device_ms, int* result_in_b);

/* ---- immersed-boundary stepper -------------------------------------------- */
/* replaces: IBMStepper.warp_implementation and its kernels, xlb/operator/stepper/ibm_stepper.py:156-178 (Peskin's 4-point
 * weights) and :264-476 (the multi-direct-forcing sweeps).  One xlbhip_ibm_step = xlbhip_step of `stepper` (never the two-step
 * kernel), then the coupling on the field it wrote: the Lagrangian forces start at zero; per sweep the marker forces are spread to
 * the cells (acc = sum_k w A F, W = sum_k w), G = relaxation (acc / W - u) where W > 0, the fluid velocity is interpolated back and
 * F_k += U_k - u_k; from the second sweep on a sweep raises a flag when any |F_k - prev_k|^2 > tolerance^2 and the next sweep runs
 * only if it was raised (tolerance 0: all sweeps run); finally f_1 += store(feq(rho, u + G) - feq(rho, u)).
 * Cell (i, j, k) sits at (i + 1/2, j + 1/2, k + 1/2); supports are clipped at the box faces (no periodic wrap).
 * Everything runs on the markers' footprint (cells with W > 0): no launch and no buffer of the coupling scales with the grid except
 * one int32 per cell (cell -> footprint slot).  acc and W are accumulated in 64-bit fixed point (per cell: quantum 2^-40 of its largest weight) with integer atomics:
 * results are bit-identical run to run and independent of the order of the markers.  The early exit is taken on the device; no call
 * below waits for it except _forces, _iterations and _footprint.
 * 3-D lattices, fp32 / fp64 storage, fields without ghost planes of nx x ny x nz cells; max_iterations 0 .. 64. */
int xlbhip_ibm_create(xlbhip_ctx* ctx, xlbhip_stepper* stepper, int lattice, int compute_dtype, int store_dtype, int nx, int ny, int nz,
                      int max_iterations, double tolerance, double relaxation, xlbhip_ibm** out);
int xlbhip_ibm_destroy(xlbhip_ibm* ibm);
/* n markers: positions (n, 3), areas (n), velocities (n, 3), float32, any of them NULL = keep what the device holds (all three are
 * needed when n changes).  Copied through a pinned staging buffer by hipMemcpyAsync on the compute stream; the host waits only for
 * the previous copy out of that buffer.  The footprint is rebuilt only when the positions differ from the last ones passed. */
int xlbhip_ibm_set_markers(xlbhip_ibm* ibm, int64_t n, const float* positions, const float* areas, const float* velocities);
/* one step f_src -> f_dst with the coupling applied to f_dst (caller swaps), ibm_stepper.py:379-476 */
int xlbhip_ibm_step(xlbhip_ibm* ibm, const xlbhip_field* f_src, xlbhip_field* f_dst, const xlbhip_field* bc_mask,
                    const xlbhip_field* missing_mask, double omega, int64_t timestep);
/* n_steps such steps with fixed markers and the A/B swap done natively; *result_in_b = 1 when the result is in f_b */
int xlbhip_ibm_run(xlbhip_ibm* ibm, xlbhip_field* f_a, xlbhip_field* f_b, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask,
                   double omega, int64_t first_timestep, int64_t n_steps, int* result_in_b);
/* the Lagrangian forces of the last step (ibm_stepper.py:476: s_lagr_forces), (n, 3) widened to double.  Synchronous. */
int xlbhip_ibm_forces(xlbhip_ibm* ibm, int64_t n, double* forces);
/* the number of sweeps the last step ran (0 without markers).  Synchronous. */
int xlbhip_ibm_iterations(xlbhip_ibm* ibm, int* sweeps);
/* size of the footprint and, with cells != NULL, its linear cell indices ((x * ny + y) * nz + z, in slot order).  Synchronous. */
int xlbhip_ibm_footprint(xlbhip_ibm* ibm, int64_t* n_cells, int64_t capacity, uint32_t* cells);

/* -- rigid bodies with prescribed motion, and the loads on them --
 * replaces: the `rotate_rotor` kernel of examples/ibm/wind_turbine_ibm.py:160-199, which turns the rotor's vertices and sets their
 * velocities on the device after every step; the call order is that of xlb/operator/stepper/ibm_stepper.py:379-476 with the markers
 * placed first.  The per-body force and torque have no counterpart in the reference (its drivers sum marker forces on the host).
 *
 * A body is a range [first, first + count) of the markers; bodies are disjoint, at most 64.  moving[i] is 0 (at rest), 1 (prescribed:
 * staged poses) or 2 (dynamic: see "free rigid bodies" below).  moving[i] != 0: before every step
 * marker k of body i is placed at X = c + R (X0 - centre0_i) and given U = v + w x (X - c), with X0 the position last UPLOADED
 * (the reference position), and (R, c, w, v) the body's pose at that timestep: 18 doubles, R row-major first.  fp64 in the order
 * X_a = ((R_a0 d_0 + R_a1 d_1) + R_a2 d_2) + c_a, rounded to float32; U is evaluated on the rounded X.  The uploaded velocities of
 * such markers are ignored.  Markers of bodies at rest and of no body are never touched.  When at least one body moves the
 * footprint is rebuilt every step; bodies at rest alone leave the step's launches as they are and only add the loads.
 * After the coupling of every step: loads[i] = (-sum_k A_k F_k, -sum_k A_k (X_k - c_i) x F_k) over the body's markers, every
 * factor a double before any product, summed over chunks of 256 consecutive markers with a fixed tree and the chunks in index order
 * (no floating-point atomics: bit-identical from run to run); c_i is the step's pose centre, centre0_i while no body moves.
 * Replaces any earlier declaration; n_bodies = 0 returns to the plain stepper.  Waits for the stream (set-up call).  The number of
 * markers cannot change while bodies are declared. */
int xlbhip_ibm_set_bodies(xlbhip_ibm* ibm, int n_bodies, const int64_t* first, const int64_t* count, const int* moving,
                          const double* centre0);
/* the poses [n_steps][n_bodies][18] of timesteps first_timestep .. first_timestep + n_steps - 1 (every body, also those at rest),
 * replacing what was staged before; at most XLBHIP_IBM_POSE_BYTES at once.  Copied through a pinned buffer by hipMemcpyAsync on the
 * compute stream, behind the steps already enqueued; the host waits only for the previous copy out of that buffer.  While a body
 * moves, xlbhip_ibm_step / _run fail BEFORE enqueuing anything when a timestep of theirs is not staged (the message names it). */
#define XLBHIP_IBM_POSE_BYTES (1 << 20)
int xlbhip_ibm_stage_poses(xlbhip_ibm* ibm, int64_t first_timestep, int64_t n_steps, const double* poses);
/* the loads of the last step, [n_bodies][6] (zero before the first).  Synchronous. */
int xlbhip_ibm_loads(xlbhip_ibm* ibm, int n_bodies, double* loads);
/* from now on every step also writes its loads to the next of n_rows rows of a device buffer (n_rows = 0: stop; steps beyond the
 * last row are not recorded); _loads_history reads the first n_rows rows recorded so far, [n_rows][n_bodies][6], and is asked
 * before the recording is stopped or restarted.  Synchronous. */
int xlbhip_ibm_record_loads(xlbhip_ibm* ibm, int64_t n_rows);
int xlbhip_ibm_loads_history(xlbhip_ibm* ibm, int64_t n_rows, double* loads);
/* the markers as the device holds them now (after the last step's move), (n, 3) float32 each; NULL: skipped.  Synchronous. */
int xlbhip_ibm_download_markers(xlbhip_ibm* ibm, int64_t n, float* positions, float* velocities);

/* -- free (force-driven) rigid bodies --
 * No counterpart in the reference (examples/ibm/wind_turbine_ibm.py prescribes its rotor's rate).  moving[i] == 2 in
 * xlbhip_ibm_set_bodies declares body i DYNAMIC: its pose is not staged but advanced on the device, once per step and after the
 * loads of that step, by the explicit scheme stated in csrc/ibm_dynamics_kernels.hpp (symplectic Euler for the centre, a Cayley
 * update of a unit quaternion for the rotation; fp64, dt = 1, one stated operation order).  A dynamic body counts as moving: its
 * markers are placed by the same rule as a prescribed body's and the footprint is rebuilt every step.  Staged poses are demanded
 * only while a PRESCRIBED body moves; the rows staged for dynamic bodies are ignored.
 *
 * _set_dynamics: for every declared body (the entries of bodies that are not dynamic are ignored) the rotation mode — 0 locked,
 * 1 about a fixed world axis, 2 free — 32 doubles of parameters and 16 doubles of initial state:
 *   params: 0 1/mass | 1-3 translate (0. or 1. per world axis) | 4-6 force | 7-9 torque | 10-12 spring anchor | 13-15 stiffness |
 *           16-18 damping | 19-27 inverse body-frame inertia, row-major | 28-30 axis (unit) | 31 1 / (inertia about the axis)
 *   state:  0-2 c | 3-5 v | 6-9 unit quaternion (w, x, y, z) | 10-12 world-frame angular momentum (axis mode: [10] is the rate) | 0 0 0
 * Called after xlbhip_ibm_set_bodies and before the first step (steps fail until it is); calling it again resets the state and
 * clears the status word.  Waits for the stream (set-up call). */
int xlbhip_ibm_set_dynamics(xlbhip_ibm* ibm, int n_bodies, const int* rotate, const double* params, const double* state);
/* the poses [n_bodies][18] (R | c | w | v) the NEXT step would read — the state of the dynamic bodies, the rest pose of every
 * other body (the caller knows the prescribed ones) — and the sticky status word: bit i set = a new state of body i had a component
 * that was not finite and was not stored; the body has stood still since.  Synchronous. */
int xlbhip_ibm_body_poses(xlbhip_ibm* ibm, int n_bodies, double* poses, uint64_t* status);
/* as _record_loads / _loads_history for the poses that the move and the loads of every step read, [n_rows][n_bodies][18]: the
 * state of dynamic bodies, the staged rows of prescribed ones, the rest poses of bodies at rest. */
int xlbhip_ibm_record_poses(xlbhip_ibm* ibm, int64_t n_rows);
int xlbhip_ibm_poses_history(xlbhip_ibm* ibm, int64_t n_rows, double* poses);

/* -- virtual mass and contact forces of the free bodies --
 * No counterpart in the reference.  Both are opt-in and evaluated inside the integrator's launch (csrc/ibm_dynamics_kernels.hpp
 * states every operation); a stepper that switches neither on enqueues exactly the launches it did without them.  All three are
 * called after xlbhip_ibm_set_dynamics; xlbhip_ibm_set_bodies and xlbhip_ibm_set_dynamics switch both off again.
 *
 * _set_virtual_mass: per declared body (entries of bodies that are not dynamic are ignored) the virtual mass m_v and the virtual
 * inertia I_v (added as I_v E to the body-frame inertia), finite and >= 0, after Schwarz, Kempe & Froehlich, J. Comput. Phys. 281
 * (2015) 591: a = (F + m_v a_prev) / (mass + m_v), T' = T + I_v alpha_prev, with the acceleration and the change of the angular
 * velocity of the PREVIOUS step, which the device keeps (6 doubles per body, zeroed by this call and by _set_dynamics).  The caller
 * has put 1 / (mass + m_v), the inverse of (Ib + I_v E) and 1 / (I_a + I_v) into slots 0, 19-27 and 31 of the parameters of
 * _set_dynamics, and the angular momentum of that inertia into the state.  Waits for the stream (set-up call). */
int xlbhip_ibm_set_virtual_mass(xlbhip_ibm* ibm, int n_bodies, const double* virtual_mass, const double* virtual_inertia);
/* _set_contact: a central repulsive force on every dynamic body i with radius[i] > 0 (0: the body does not take part), from the
 * centres of the step's poses: k (range - gap)^2 (c_i - c_j) / d against every other body j with a radius — prescribed bodies and
 * bodies at rest are obstacles — while gap = d - (r_i + r_j) < range and d > 0, and kw (range - gap)^2 along +a (-a) from the plane
 * x_a = lo[a] (hi[a]) while gap = |c_a - plane| - r_i < range.  lo / hi: 3 doubles each, -inf / +inf switch a plane off, NULL all
 * three; lo[a] < hi[a].  radius, range, stiffness and wall_stiffness are finite and >= 0.  The force enters the integrator's F and
 * not the loads, which stay hydrodynamic; it exerts no torque.  With no radius above zero contact is off.  Waits for the stream. */
int xlbhip_ibm_set_contact(xlbhip_ibm* ibm, int n_bodies, const double* radius, double range, double stiffness, double wall_stiffness,
                           const double* lo, const double* hi);
/* the contact force on every body in the last step, [n_bodies][3] (zero before the first step, for bodies that are not dynamic or
 * have no radius, and while contact is off).  Synchronous. */
int xlbhip_ibm_contact_forces(xlbhip_ibm* ibm, int n_bodies, double* forces);

/* ---- flow statistics ------------------------------------------------------- */
/* No counterpart in the reference: its drivers copy whole fields to the host and reduce them in NumPy (e.g.
 * examples/cfd/turbulent_channel_3d.py).  The object keeps running fp64 sums on the device of, per sampled cell: 1 (count), rho,
 * rho^2, u_a (d components), u_a u_b (xx, xy, xz, yy, yz, zz; three in 2-D) with order 2 (12 channels in 3-D, 8 in 2-D), or count,
 * rho, u_a with order 1.  rho and u are the values xlbhip_macroscopic writes (compute dtype), promoted to double before any product
 * or sum.  keep_mask says which STORAGE axes are kept (bit 0: x, bit 1: y, bit 2: z; a 2-D grid is nx = 1); the others are summed
 * over, so there are (kept nx) * (kept ny) * (kept nz) bins, x slowest.  exclude: 256 bits, bit v set = cells whose bc_mask value is
 * v are not sampled.  Ghost planes are never sampled.  No floating-point atomics: which cells meet in which partial sum, and the
 * order the partial sums are added in, depend on (nx, ny, nz, keep_mask, order) only, so the sums are bit-identical from run to run
 * and from device to device.  The partial sums take at most 48 MiB of scratch; the running sums channels * bins * 8 bytes. */
int xlbhip_stats_create(xlbhip_ctx* ctx, int lattice, int compute_dtype, int nx, int ny, int nz, int keep_mask, int order,
                        const uint32_t exclude[8], xlbhip_stats** out);
int xlbhip_stats_destroy(xlbhip_stats* stats);
/* add one sample of f (any store dtype the compute dtype can hold; with or without ghost planes) to the running sums; bc_mask NULL:
 * every cell is sampled.  Enqueues on the compute stream; the host neither waits nor reads anything. */
int xlbhip_stats_sample(xlbhip_stats* stats, const xlbhip_field* f, const xlbhip_field* bc_mask);
/* Synchronous.  sums (capacity = channels * bins doubles, [channel][bin]; NULL: skipped), the number of samples since the last
 * reset, the largest u.u over the sampled cells of the LAST sample (compute-dtype arithmetic, (ux ux + uy uy) + uz uz), and the
 * number of sampled cells whose rho or u was not finite: nonfinite[0] in the last sample, nonfinite[1] since the last reset.  Such
 * a cell adds to these counters and to nothing else. */
int xlbhip_stats_read(xlbhip_stats* stats, int64_t capacity, double* sums, int64_t* samples, double* max_u2, int64_t nonfinite[2]);
/* zero the sums, the sample count and the watchdog (enqueued) */
int xlbhip_stats_reset(xlbhip_stats* stats);

/* ---- slab decomposition over ranks (one process per GPU) ------------------ */
/* semantics reference: xlb/distribute/distribute.py:18-48 (ring exchange of the
 * face-crossing populations along the slowest spatial axis). */
#define XLBHIP_UNIQUE_ID_BYTES 128
int xlbhip_comm_unique_id(void* out_id_bytes);     /* rank 0; broadcast by the host side */
/* n_ranks == 1 with a non-NULL id creates a real one-rank RCCL communicator (self send/recv): used to
 * exercise the RCCL code path on a single GPU; with a NULL id the ghosts are refilled by device copies */
int xlbhip_comm_init(xlbhip_ctx* ctx, int rank, int n_ranks, const void* id_bytes, int periodic_x);
/* replaces: the same two lax.ppermute calls (xlb/distribute/distribute.py:31-41) as xlbhip_comm_init, by another transport.
 * The same exchange without RCCL: every rank exports the buffers it exchanges (hipIpcGetMemHandle) and PULLS the
 * neighbours' planes on the communication stream — by one small copy kernel per exchange (option "ipc_copy" = 1, the
 * default: 8 blocks per plane, no LDS) or by plane-sized hipMemcpyAsync calls (= 0: copy engines, no compute unit;
 * "or hipMemcpyPeerAsync ... over xGMI").  Processes are ordered by sequence counters in a host
 * shared-memory control block /dev/shm/xlbhip-ipc-<token> (created by rank 0, unlinked as soon as every rank mapped
 * it) that one-lane kernels post and poll; every wait is bounded by the option "ipc_timeout_ms" (default 180 s; a timed-out wait
 * makes the next xlbhip_sync fail).  One node; the ranks may share a device.  `token`: letters / digits / '-' / '_',
 * fresh per job (the host side broadcasts a random one).  Ranks must exchange the same buffers in the same order. */
int xlbhip_comm_init_ipc(xlbhip_ctx* ctx, int rank, int n_ranks, const char* token, int periodic_x);
int xlbhip_comm_destroy(xlbhip_ctx* ctx);
/* (no counterpart in the reference's JAX path; Neon's skeleton reports its overlap mode in the benchmark's JSON, mlups_3d.py:434-488)
 * Telemetry of the slab protocol: the time the compute stream spent waiting for the halo event after the interior
 * launch, summed over `halo_waits` exchanges since the last reset (option "halo_telemetry", default on).  With a
 * working overlap it is the event overhead only (a few microseconds per exchange).  Blocking. */
int xlbhip_comm_stats(xlbhip_ctx* ctx, double* halo_wait_ms, int64_t* halo_waits, int reset);
/* fill the ghost planes of f from the neighbours (blocking w.r.t. the compute stream order) */
int xlbhip_halo_exchange(xlbhip_ctx* ctx, int lattice, xlbhip_field* f);
/* the exchange a fused pair of steps needs (fields with 2 ghost planes): every population of the neighbours' edge
 * planes and the face-crossing populations of the planes behind them */
int xlbhip_halo_exchange_wide(xlbhip_ctx* ctx, int lattice, xlbhip_field* f);

/* ---- scalar transport ------------------------------------------------------------------------------------------------------
 * (no counterpart in the reference, which only names the physics: PhysicsType.ADE, xlb/physics_type.py; pinned by the NumPy
 * restatement tests/_scalar_ref.py)  One scalar phi advected and diffused by the flow on the sub-lattice of rest + main directions
 * (D2Q5 / D3Q7; scalar direction 0 = rest, 1.. = the lattice's main directions in ascending order), updated in the SAME kernel as
 * the fluid: geq_j = w_j phi (1 + c_j.u / cs^2) with the post-streaming velocity u, g <- g - omega_scalar (g - geq), diffusivity
 * cs^2 (1 / omega_scalar - 1/2), cs^2 = 1/4 (3-D) or 1/3 (2-D).  With a force or buoyancy the fluid collides through the
 * exact-difference forced path with the per-cell force  force + buoyancy * (phi - reference)  (internal 3-component form), phi the
 * sum of the post-streaming g.  Fields without ghost planes, FP32FP32 / FP64FP64 / FP64FP32, the bit-exact collisions.
 * bcs: as for xlbhip_stepper_create; kinds 1..9 with constant values (no HybridBC, no profile walls). */
int xlbhip_scalar_create(xlbhip_ctx* ctx, int lattice, int collision, int compute_dtype, int store_dtype, int n_bc, const xlbhip_bc_desc* bcs,
                         xlbhip_scalar** out);
int xlbhip_scalar_destroy(xlbhip_scalar* s);
/* The scalar's rule at the cells of bc id bc_ids[i], acting where the FLUID's missing_mask bit of a main direction is set:
 * rules[i] = 0 adiabatic (bounce-back; the default of every bc id), 1 Dirichlet (anti-bounce-back: phi = values[i] at the link
 * midpoint; refused on a fullway wall), 2 do-nothing (the cell keeps its pre-streaming g, every direction).  At fullway cells the
 * scalar is bounced fullway after the collision.  Replaces all rules set before. */
int xlbhip_scalar_set_rules(xlbhip_scalar* s, int n, const int32_t* bc_ids, const int32_t* rules, const double* values);
/* force, buoyancy: 3 doubles each or NULL (both NULL: passive scalar, the fluid is that of xlbhip_step bit for bit) */
int xlbhip_scalar_set_coupling(xlbhip_scalar* s, const double* force, const double* buoyancy, double reference, double smagorinsky_coef);
/* g_0 = geq(phi, u(f_0)); phi: a cardinality-1 float field, or NULL for the constant phi0 */
int xlbhip_scalar_init(xlbhip_scalar* s, const xlbhip_field* f_0, const xlbhip_field* phi, double phi0, xlbhip_field* g_0);
/* ScalarMoment()(g, phi): phi = sum_j g_j, sequential in j, in the compute dtype */
int xlbhip_scalar_moment(xlbhip_ctx* ctx, int lattice, int compute_dtype, const xlbhip_field* g, xlbhip_field* phi);
/* one coupled step (f, g)(t) -> (f, g)(t + 1); omega, omega_scalar in (0, 2] */
int xlbhip_scalar_step(xlbhip_scalar* s, const xlbhip_field* f_src, xlbhip_field* f_dst, const xlbhip_field* g_src, xlbhip_field* g_dst,
                       const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega, double omega_scalar, int64_t timestep);
/* n_steps x (step, swap both pairs) enqueued without a host wait; *result_in_b: the result is in (f_b, g_b) */
int xlbhip_scalar_run(xlbhip_scalar* s, xlbhip_field* f_a, xlbhip_field* f_b, xlbhip_field* g_a, xlbhip_field* g_b, const xlbhip_field* bc_mask,
                      const xlbhip_field* missing_mask, double omega, double omega_scalar, int64_t first_timestep, int64_t n_steps, int* result_in_b);

/* ---- discrete adjoint of the fused BGK step ---------------------------------------------------------------------------------
 * (the reference differentiates its stepper through jax.grad and ships a Warp forward / backward stepper pair,
 * examples/out_of_core/autodiff_lbm.py; here the backward pass is hand-written HIP, pinned by the NumPy restatement
 * tests/_adjoint_ref.py)  One forward step is f_{n+1} = S(f_n; omega): pull streaming, the streaming-step BCs, BGK, the fullway bounce.
 * An adjoint step takes the forward state f_n and the cotangent lam_{n+1} = dL/df_{n+1} and gives lam_n = (dS/df_n)^T lam_{n+1}; its
 * omega term sum_cells sum_l lam_l (feq_l - f*_l) is added, widened to fp64 and in a fixed order, to a device scalar of the object.
 * The Jacobian is that of the exact-arithmetic map (casts count as the identity).  BGK without a force; fields without ghost planes;
 * FP32FP32 / FP64FP64 / FP64FP32; bcs: as for xlbhip_stepper_create, kinds 1..4 only (equilibrium, halfway bounce-back with a constant
 * wall velocity or none, fullway bounce-back, do-nothing).  State and cotangent fields have the lattice's cardinality and the store
 * dtype. */
int xlbhip_adjoint_create(xlbhip_ctx* ctx, int lattice, int compute_dtype, int store_dtype, int n_bc, const xlbhip_bc_desc* bcs, xlbhip_adjoint** out);
int xlbhip_adjoint_destroy(xlbhip_adjoint* a);
/* lam_out = (dS/df_n)^T lam_in; two launches through a scratch field of the object (the local transpose, the transposed streaming) */
int xlbhip_adjoint_step(xlbhip_adjoint* a, const xlbhip_field* f_n, const xlbhip_field* lam_in, xlbhip_field* lam_out, const xlbhip_field* bc_mask,
                        const xlbhip_field* missing_mask, double omega);
/* The adjoint steps over states[0 .. n_states-1] = f_0 .. f_{N-1}, last first, enqueued without a host wait: lam_a holds lam_N on
 * entry; one fused launch per step (the carried state is mu = dL/df*, in the store dtype) and one closing launch, ping-ponging
 * between lam_a and lam_b (both overwritten); *result_in_b: lam_0 is in lam_b.  The bits are those of n_states chained
 * xlbhip_adjoint_step calls. */
int xlbhip_adjoint_run(xlbhip_adjoint* a, int64_t n_states, const xlbhip_field* const* states, xlbhip_field* lam_a, xlbhip_field* lam_b,
                       const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega, int* result_in_b);
/* dL/domega accumulated by every step since the last reset (waits for the compute stream) / sets it to zero (enqueued) */
int xlbhip_adjoint_omega_gradient(xlbhip_adjoint* a, double* out);
int xlbhip_adjoint_reset(xlbhip_adjoint* a);
/* MacroscopicAdjoint()(f, rho_bar, u_bar, lam): lam_l = rho_bar + sum_d u_bar_d (c_dl - u_d) / rho, the transpose of Macroscopic at f
 * applied to (dL/drho, dL/du); rho_bar (cardinality 1) or u_bar (cardinality d) may be NULL for zero */
int xlbhip_macroscopic_adjoint(xlbhip_ctx* ctx, int lattice, int compute_dtype, const xlbhip_field* f, const xlbhip_field* rho_bar, const xlbhip_field* u_bar,
                               xlbhip_field* lam);

/* ---- porous BGK step and its discrete adjoint -----------------------------------------------------------------------------------
 * (geometry as a continuous field: a per-cell solidity alpha in [0, 1], after Pingen, Evgrafov and Maute, Struct. Multidisc. Optim. 34,
 * 507 (2007); pinned by the NumPy restatement tests/_porous_ref.py)  The step is the fused BGK step with the equilibrium taken at the
 * damped velocity (1 - alpha) u; alpha == 0 is the plain BGK step bit for bit.  Values outside [0, 1] are the caller's business and are
 * not checked.  Scope as the adjoint's: BGK without a force; fields without ghost planes; FP32FP32 / FP64FP64 / FP64FP32; bc kinds 1..4.
 * The solidity field has one value per cell in the COMPUTE dtype; it is bound by ADDRESS: destroying the field while it is bound and
 * then stepping or reading the gradient is undefined (the library cannot tell), so bind another field first or keep it alive.  The adjoint
 * step is xlbhip_adjoint_step's with the porous transpose; beside dL/domega it accumulates dL/dalpha in an fp64 field of the object,
 * each cell by its own thread, in the order of the steps. */
typedef struct xlbhip_porous xlbhip_porous;
int xlbhip_porous_create(xlbhip_ctx* ctx, int lattice, int compute_dtype, int store_dtype, int n_bc, const xlbhip_bc_desc* bcs, xlbhip_porous** out);
int xlbhip_porous_destroy(xlbhip_porous* p);
/* binds alpha; a field whose grid (nx, ny, nz) differs from the last one's starts a new (zero) gradient field */
int xlbhip_porous_set_solidity(xlbhip_porous* p, const xlbhip_field* alpha);
int xlbhip_porous_step(xlbhip_porous* p, const xlbhip_field* f_src, xlbhip_field* f_dst, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask,
                       double omega, int64_t timestep);
int xlbhip_porous_run(xlbhip_porous* p, xlbhip_field* f_a, xlbhip_field* f_b, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega,
                      int64_t first_timestep, int64_t n_steps, int* result_in_b);
/* as xlbhip_adjoint_step / xlbhip_adjoint_run, at the bound alpha */
int xlbhip_porous_adjoint_step(xlbhip_porous* p, const xlbhip_field* f_n, const xlbhip_field* lam_in, xlbhip_field* lam_out, const xlbhip_field* bc_mask,
                               const xlbhip_field* missing_mask, double omega);
int xlbhip_porous_adjoint_run(xlbhip_porous* p, int64_t n_states, const xlbhip_field* const* states, xlbhip_field* lam_a, xlbhip_field* lam_b,
                              const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega, int* result_in_b);
/* zeroes dL/domega and dL/dalpha (enqueued) / dL/domega (waits for the compute stream) / copies dL/dalpha into `out`, an fp64 field of
 * one value per cell on alpha's grid (enqueued) */
int xlbhip_porous_adjoint_reset(xlbhip_porous* p);
int xlbhip_porous_omega_gradient(xlbhip_porous* p, double* out);
int xlbhip_porous_solidity_gradient(xlbhip_porous* p, xlbhip_field* out);

/* ---- Shan-Chen pseudopotential flow (single component, liquid-vapour) ----------------------------------------------------------
 * (no counterpart in the reference; the interaction force is Shan and Chen's, Phys. Rev. E 47, 1815 (1993), applied through the
 * exact-difference forcing the reference has for a constant force, xlb/operator/force/exact_difference_force.py; the Carnahan-Starling
 * pseudopotential follows Yuan and Schaefer, Phys. Fluids 18, 042101 (2006); pinned by the NumPy restatement tests/_multiphase_ref.py)
 * One step on the post-streaming populations (pull, then the streaming-step boundary rules): rho, u = moments; psi = Psi(rho);
 * F_a = (-G psi(x)) sum_{i >= 1} (w_i psi(x + c_i)) c_ai with the fluid lattice's weights; the cell collides by BGK with the
 * exact-difference acceleration force_a + F_a / rho.  A neighbour behind a missing direction (bit opp(i) of the cell's missing mask)
 * counts with the wall value Psi(rho_w) of the cell's own bc id; fullway bounce-back cells and solid cells (bc id 255) carry their
 * Psi(rho_w) as psi and feel no force.  The bulk pressure is cs^2 rho + (G cs^2 / 2) psi^2, cs^2 = 1/3.  Two launches per step (psi, then
 * the step that reads the neighbours' psi); the psi field is the object's.  Fields without ghost planes, FP32FP32 / FP64FP64 /
 * FP64FP32.  bcs: as for xlbhip_stepper_create, kinds 2 and 3 only (halfway bounce-back with a constant wall velocity or none, fullway
 * bounce-back). */
int xlbhip_multiphase_create(xlbhip_ctx* ctx, int lattice, int compute_dtype, int store_dtype, int n_bc, const xlbhip_bc_desc* bcs, xlbhip_multiphase** out);
int xlbhip_multiphase_destroy(xlbhip_multiphase* m);
/* form 0: psi = rho0 (1 - exp(-rho / rho0)), params = {rho0};  1: psi = rho, no params;  2: Carnahan-Starling, params = {T, a, b, R}:
 * p = rho R T (1 + eta + eta^2 - eta^3) / (1 - eta)^3 - a rho^2, eta = b rho / 4, psi = sqrt(2 (p - cs^2 rho) / (G cs^2)), g must be -1.
 * force: 3 doubles (internal 3-component form) or NULL, the constant acceleration added to F / rho */
int xlbhip_multiphase_set_model(xlbhip_multiphase* m, int form, double g, int n_params, const double* params, const double* force);
/* The wall densities: rho_w[i] for bc id bc_ids[i] (one of this object's BCs, or 255 for solid cells), with psi_w[i] = Psi(rho_w[i]) as
 * the caller evaluates its model in the compute dtype: these bits go into the table, so that a host restatement shares them.  Every
 * other id has Psi = 0 (a wall that neither attracts nor repels beyond the missing neighbour).  Replaces all values set before. */
int xlbhip_multiphase_set_wall_density(xlbhip_multiphase* m, int n, const int32_t* bc_ids, const double* rho_w, const double* psi_w);
/* one step f(t) -> f(t + 1); omega in (0, 2] */
int xlbhip_multiphase_step(xlbhip_multiphase* m, const xlbhip_field* f_src, xlbhip_field* f_dst, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask,
                           double omega, int64_t timestep);
/* n_steps x (step, swap) enqueued without a host wait; *result_in_b: the result is in f_b */
int xlbhip_multiphase_run(xlbhip_multiphase* m, xlbhip_field* f_a, xlbhip_field* f_b, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega,
                          int64_t first_timestep, int64_t n_steps, int* result_in_b);
/* Outputs of the post-streaming state of the stored field f, in the compute dtype: psi (cardinality 1); the interaction force F without
 * the force vector (cardinality d; zero at wall cells); rho (cardinality 1) and the physical velocity u = u_bare + F / (2 rho)
 * (cardinality d) */
int xlbhip_multiphase_psi(xlbhip_multiphase* m, const xlbhip_field* f, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, xlbhip_field* psi);
int xlbhip_multiphase_force(xlbhip_multiphase* m, const xlbhip_field* f, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, xlbhip_field* force);
int xlbhip_multiphase_macroscopic(xlbhip_multiphase* m, const xlbhip_field* f, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, xlbhip_field* rho,
                                  xlbhip_field* u);

/* ---- Shan-Chen flow of two immiscible components A and B ------------------------------------------------------------------------------
 * (no counterpart in the reference; Shan and Chen, Phys. Rev. E 47, 1815 (1993); Shan and Doolen, J. Stat. Phys. 81, 379 (1995); walls
 * after Martys and Chen, Phys. Rev. E 53, 743 (1996); applied through the exact-difference forcing the reference has for a constant
 * force, xlb/operator/force/exact_difference_force.py; pinned by the NumPy restatement tests/_multicomponent_ref.py)
 * Each component s has its populations f^s on the same lattice and its relaxation rate omega_s.  One step on the post-streaming
 * populations (pull, then the streaming-step boundary rules, per component): rho_s, u_s = moments; psi_s = rho_s;
 * u' = (omega_A rho_A u_A + omega_B rho_B u_B) / (omega_A rho_A + omega_B rho_B); S^s_a = sum_{i >= 1} (w_i psi_s(x + c_i)) c_ai with the
 * lattice's weights; F^A = (-psi_A) (G_AA S^A + G_AB S^B), F^B = (-psi_B) (G_AB S^A + G_BB S^B); each component collides by BGK towards
 * feq(rho_s, u') with the exact-difference acceleration force + F^s / rho_s.  A neighbour behind a missing direction counts with the wall
 * densities of the cell's own bc id; fullway bounce-back cells and solid cells (bc id 255) carry their wall densities and feel no force.
 * The bulk pressure is cs^2 (rho_A + rho_B) + cs^2 (G_AA rho_A^2 / 2 + G_AB rho_A rho_B + G_BB rho_B^2 / 2).  Two launches per step (both
 * densities, then the step that reads the neighbours'); the density fields are the object's.  Fields without ghost planes, FP32FP32 /
 * FP64FP64 / FP64FP32.  bcs: as for xlbhip_stepper_create, kinds 2 and 3 only, and a halfway wall at rest (all values zero: the
 * moving-wall constant assumes density 1). */
int xlbhip_multicomponent_create(xlbhip_ctx* ctx, int lattice, int compute_dtype, int store_dtype, int n_bc, const xlbhip_bc_desc* bcs,
                                 xlbhip_multicomponent** out);
int xlbhip_multicomponent_destroy(xlbhip_multicomponent* m);
/* force: 3 doubles (internal 3-component form) or NULL, the constant acceleration added to F^s / rho_s of both components */
int xlbhip_multicomponent_set_model(xlbhip_multicomponent* m, double g_aa, double g_ab, double g_bb, const double* force);
/* The wall densities: rho_w_a[i], rho_w_b[i] for bc id bc_ids[i] (one of this object's BCs, or 255 for solid cells), rounded to the
 * compute dtype.  Every other id has 0 for both.  Replaces all values set before. */
int xlbhip_multicomponent_set_wall_density(xlbhip_multicomponent* m, int n, const int32_t* bc_ids, const double* rho_w_a, const double* rho_w_b);
/* one step (f^A, f^B)(t) -> (t + 1); omega_a, omega_b in (0, 2] */
int xlbhip_multicomponent_step(xlbhip_multicomponent* m, const xlbhip_field* fa_src, xlbhip_field* fa_dst, const xlbhip_field* fb_src, xlbhip_field* fb_dst,
                               const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega_a, double omega_b, int64_t timestep);
/* n_steps x (step, swap of both pairs) enqueued without a host wait; *result_in_1: the result is in fa_1 and fb_1 */
int xlbhip_multicomponent_run(xlbhip_multicomponent* m, xlbhip_field* fa_0, xlbhip_field* fa_1, xlbhip_field* fb_0, xlbhip_field* fb_1,
                              const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega_a, double omega_b, int64_t first_timestep,
                              int64_t n_steps, int* result_in_1);
/* Outputs of the post-streaming state of the stored fields fa, fb, in the compute dtype.  densities: psi_A, psi_B as the force reads them
 * (cardinality 1 each; the wall densities at wall cells).  force: F^A and F^B without the force vector (cardinality d each; zero at wall
 * cells).  macroscopic: rho_A, rho_B (the moments, cardinality 1 each) and the barycentric velocity
 * u = (rho_A u_A + rho_B u_B + (F^A + F^B) / 2) / (rho_A + rho_B) (cardinality d). */
int xlbhip_multicomponent_densities(xlbhip_multicomponent* m, const xlbhip_field* fa, const xlbhip_field* fb, const xlbhip_field* bc_mask,
                                    const xlbhip_field* missing_mask, xlbhip_field* rho_a, xlbhip_field* rho_b);
int xlbhip_multicomponent_force(xlbhip_multicomponent* m, const xlbhip_field* fa, const xlbhip_field* fb, const xlbhip_field* bc_mask,
                                const xlbhip_field* missing_mask, xlbhip_field* force_a, xlbhip_field* force_b);
int xlbhip_multicomponent_macroscopic(xlbhip_multicomponent* m, const xlbhip_field* fa, const xlbhip_field* fb, const xlbhip_field* bc_mask,
                                      const xlbhip_field* missing_mask, xlbhip_field* rho_a, xlbhip_field* rho_b, xlbhip_field* u);

#ifdef __cplusplus
}
#endif
#endif /* XLBHIP_H */
