// libxlbhip: the porous BGK step (a per-cell solidity alpha in the fused step) and its discrete adjoint.  The object owns the boundary
// tables (a BcTables like a stepper's, stepper_tables.hpp), the binding of the caller's solidity field and what a backward sweep keeps:
// the carried-state scratch field of a single adjoint step, the per-block partial sums, the device scalar dL/domega and the fp64 field
// dL/dalpha.  Everything is enqueued on the context's compute stream; only omega_gradient waits for the device.
#include "porous_launch.hpp"
#include "stepper_tables.hpp"

using namespace xlb;

struct xlbhip_porous : RowStepper {
  const xlbhip_field* alpha = nullptr;  // the bound solidity field: the caller's, held by address; destroying it while bound is the
                                        // caller's error (nothing here can tell), so it is rebound or outlives this object
  DeviceBuf mu;                         // the carried state between the two launches of a single adjoint step (store dtype, q planes)
  size_t mu_elems = 0;
  DeviceBuf partial;  // fp64 [blocks], then [chunks of blocks]: the two levels below the device scalar
  size_t partial_n = 0;
  DeviceBuf domega;  // fp64 [1]: the omega terms of every adjoint step since the last reset, summed in step order
  DeviceBuf galpha;  // fp64 [cells of alpha]: dL/dalpha of every adjoint step since the last reset
  size_t galpha_cells = 0;
  int galpha_nx = 0, galpha_ny = 0, galpha_nz = 0;  // the grid the gradient field belongs to
  // gather bits of the transposed streaming (adjoint_kernels.hpp: k_adjoint_gather_mask), valid for these contents of the two masks
  DeviceBuf gmask;
  const void *gmask_bc = nullptr, *gmask_miss = nullptr;
  uint64_t gmask_bc_version = 0, gmask_miss_version = 0;
  size_t gmask_cells = 0;
};

namespace xlb {

// KEEP IN STEP WITH adjoint.hip: k_porous_reduce, POROUS_CHUNK, ensure_partials, ensure_gather_mask and the two-level omega sum of
// porous_adjoint_launch_once restate k_adjoint_reduce, ADJ_CHUNK and the same functions there (that unit is left as it is, so they are
// copies): the order of the omega sum is defined in both places, and a change to one has to be made in the other.
//
// Sums of chunks of POROUS_CHUNK partials, in an order fixed by their number (the adjoint's two levels, adjoint.hip): block b adds up
// in[b * POROUS_CHUNK ..] (strided sequential sums of its ADJ_BLOCK threads, then the tree).  accumulate == 0: out[b] = the chunk's
// sum; else (one block) *out += the sum.
constexpr unsigned POROUS_CHUNK = 16 * ADJ_BLOCK;
__global__ void __launch_bounds__(ADJ_BLOCK) k_porous_reduce(const double* in, unsigned n, double* out, int accumulate) {
  const unsigned begin = blockIdx.x * POROUS_CHUNK, end = begin + POROUS_CHUNK < n ? begin + POROUS_CHUNK : n;
  double s = 0.0;
  for (unsigned i = begin + threadIdx.x; i < end; i += ADJ_BLOCK) s += in[i];
  const double total = block_sum_fixed(s);
  if (threadIdx.x == 0) {
    if (accumulate)
      *out = *out + total;
    else
      out[blockIdx.x] = total;
  }
}

// the bound solidity field against the grid `g` of a step's fields
static int check_solidity(const xlbhip_porous* s, const char* who, const xlbhip_field* g) {
  XLB_REQUIRE(s->alpha, "%s: no solidity field is bound (xlbhip_porous_set_solidity)", who);
  XLB_REQUIRE(same_grid(s->alpha, g), "%s: the solidity field is on a %d x %d x %d grid, the step's fields on %d x %d x %d", who, s->alpha->nx, s->alpha->ny,
              s->alpha->nz, g->nx, g->ny, g->nz);
  return 0;
}

static int check_forward_fields(const xlbhip_porous* s, const xlbhip_field* fa, const xlbhip_field* fb, const xlbhip_field* bcm, const xlbhip_field* miss) {
  XLB_REQUIRE(s && fa && fb, "null argument");
  XLB_REQUIRE(fa != fb && fa->data != fb->data, "f_0 and f_1 must be different fields (double buffering)");
  if (int rc = check_row_fields("porous step", "population fields", lattice_q(s->lattice), s->sdt, {fa, fb}, true)) return rc;
  if (int rc = check_single_rank_grid("porous step", "step kernel", s->lattice, s->bc.n_bc, fa, bcm, miss)) return rc;
  return check_solidity(s, "porous step", fa);
}

static int check_adjoint_fields(const xlbhip_porous* s, const xlbhip_field* f_n, const xlbhip_field* lin, const xlbhip_field* lout, const xlbhip_field* bcm,
                                const xlbhip_field* miss) {
  XLB_REQUIRE(s && lin && lout, "null argument");
  XLB_REQUIRE(lin != lout && lin->data != lout->data, "lam_in and lam_out must be different fields");
  if (int rc = check_row_fields("porous adjoint step", "state and cotangent fields", lattice_q(s->lattice), s->sdt, {f_n, lin, lout}, false)) return rc;
  if (int rc = check_single_rank_grid("porous adjoint step", "kernel", s->lattice, s->bc.n_bc, lin, bcm, miss)) return rc;
  return check_solidity(s, "porous adjoint step", lin);
}

static int porous_step_once(xlbhip_porous* s, const xlbhip_field* fs, xlbhip_field* fd, const xlbhip_field* bcm, const xlbhip_field* miss, double omega) {
  touch(fd);
  PorousLaunch q = {};
  StepLaunch& p = q.f;
  p = bc_launch(s->ctx, s->bc, s->cdt, s->sdt, bcm, miss, fs);
  p.src = fs->data;
  p.dst = fd->data;
  p.plane_stride = fs->plane_stride;
  p.omega = omega;
  p.has_bc = s->bc.n_bc > 0 ? 1 : 0;
  q.alpha = s->alpha->data;
  return launch_for_lattice(s->lattice, launch_porous_d2q9, launch_porous_d3q19, launch_porous_d3q27, q);
}

static int ensure_partials(xlbhip_porous* s, const xlbhip_field* f) {
  const size_t n = adjoint_blocks(f->nx, f->ny, f->nz);
  if (n > s->partial_n) {
    XLB_HIP(s->partial.alloc((n + (n + POROUS_CHUNK - 1) / POROUS_CHUNK) * sizeof(double)));  // (hipFree inside waits for launches that still write the old one)
    s->partial_n = n;
  }
  return 0;
}

// the gather bits for this pair of masks: built on first use and again when either mask was written since
static int ensure_gather_mask(xlbhip_porous* s, const xlbhip_field* bcm, const xlbhip_field* miss) {
  if (s->bc.n_bc == 0) return 0;
  const size_t n = bcm->cells();
  if (s->gmask && s->gmask_bc == bcm->data && s->gmask_miss == miss->data && s->gmask_bc_version == bcm->version &&
      s->gmask_miss_version == miss->version && s->gmask_cells == n)
    return 0;
  if (s->gmask_cells != n || !s->gmask) XLB_HIP(s->gmask.alloc(n * sizeof(uint32_t)));
  s->gmask_cells = n;
  const int rc = by_lattice(s->lattice, [&](auto L) {
    hipLaunchKernelGGL((k_adjoint_gather_mask<decltype(L)>), blocks_for(n), 256, 0, s->ctx->stream, static_cast<const uint8_t*>(bcm->data),
                       static_cast<const uint32_t*>(miss->data), s->bc.tab_kind.get<const uint8_t>(), s->gmask.get<uint32_t>(), dims(bcm));
    XLB_HIP(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  s->gmask_bc = bcm->data;
  s->gmask_miss = miss->data;
  s->gmask_bc_version = bcm->version;
  s->gmask_miss_version = miss->version;
  return 0;
}

// one launch: `in` (lam or mu, by in_mode) -> `out` (mu or lam, by out_mode), f_n for the launches that leave mu.  A launch that
// leaves mu is the porous kernel: it adds its omega terms to the device scalar and its alpha terms to the gradient field.  The launch
// that leaves lam is the plain adjoint's closing instantiation.
static int porous_adjoint_launch_once(xlbhip_porous* s, const xlbhip_field* f_n, const void* in, size_t in_stride, void* out, size_t out_stride,
                                      const xlbhip_field* grid_of, const xlbhip_field* bcm, const xlbhip_field* miss, double omega, int in_mode, int out_mode) {
  xlbhip_ctx* c = s->ctx;
  PorousAdjointLaunch pq = {};
  AdjointLaunch& q = pq.a;
  StepLaunch& p = q.f;
  p = bc_launch(c, s->bc, s->cdt, s->sdt, bcm, miss, grid_of);
  p.src = f_n ? f_n->data : nullptr;  // (no dst: the launch writes q.out)
  p.plane_stride = f_n ? f_n->plane_stride : 0;
  p.omega = omega;
  p.has_bc = s->bc.n_bc > 0 ? 1 : 0;
  q.in = in;
  q.out = out;
  q.in_stride = in_stride;
  q.out_stride = out_stride;
  q.in_mode = in_mode;
  q.out_mode = out_mode;
  q.partial = s->partial.get<double>();
  q.gmask = s->gmask.get<const uint32_t>();
  if (out_mode != ADJ_OUT_MU) return launch_for_lattice(s->lattice, launch_adjoint_d2q9, launch_adjoint_d3q19, launch_adjoint_d3q27, q);
  pq.alpha = s->alpha->data;
  pq.galpha = s->galpha.get<double>();
  if (int rc = launch_for_lattice(s->lattice, launch_porous_adjoint_d2q9, launch_porous_adjoint_d3q19, launch_porous_adjoint_d3q27, pq)) return rc;
  // the step's omega terms: per-block partials -> per-chunk sums -> the device scalar (a chunk per block; one block at the end)
  const unsigned n = (unsigned)adjoint_blocks(p.nx, p.ny, p.nz), chunks = (n + POROUS_CHUNK - 1) / POROUS_CHUNK;
  double* part = s->partial.get<double>();
  if (chunks > 1) {
    XLB_REQUIRE(chunks <= POROUS_CHUNK, "porous adjoint step: %u blocks are more than the omega sum's two levels take", n);
    hipLaunchKernelGGL(k_porous_reduce, chunks, ADJ_BLOCK, 0, c->stream, part, n, part + n, 0);
    XLB_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_porous_reduce, 1, ADJ_BLOCK, 0, c->stream, part + n, chunks, s->domega.get<double>(), 1);
  } else {
    hipLaunchKernelGGL(k_porous_reduce, 1, ADJ_BLOCK, 0, c->stream, part, n, s->domega.get<double>(), 1);
  }
  XLB_HIP(hipGetLastError());
  return 0;
}

}  // namespace xlb

extern "C" {

int xlbhip_porous_create(xlbhip_ctx* c, int lattice, int cdt, int sdt, int n_bc, const xlbhip_bc_desc* bcs, xlbhip_porous** out) {
  const auto refusal = [](int kind) {
    return bc_adjoint_accepts(kind) ? nullptr
                                    : "porous step: bc kind %d is not supported (equilibrium, halfway and fullway bounce-back and do-nothing only)";
  };
  const auto own = [](xlbhip_porous& s) {
    XLB_HIP(s.domega.alloc(sizeof(double)));
    XLB_HIP(hipMemset(s.domega.get(), 0, sizeof(double)));
    return 0;
  };
  return create_row_stepper(c, lattice, cdt, sdt, n_bc, bcs, POROUS_POLICY_SUBJECT, refusal, own, out);
}

int xlbhip_porous_destroy(xlbhip_porous* s) { return destroy_drained(s); }

int xlbhip_porous_set_solidity(xlbhip_porous* s, const xlbhip_field* alpha) {
  XLB_REQUIRE(s && alpha, "null argument");
  XLB_REQUIRE(alpha->dtype == s->cdt, "porous step: the solidity field must have the compute dtype %d (got %d)", s->cdt, alpha->dtype);
  XLB_REQUIRE(alpha->card == 1 && alpha->halo == 0, "porous step: the solidity field has one value per cell and no ghost planes");
  XLB_REQUIRE(s->lattice != XLBHIP_D2Q9 || alpha->nx == 1, "a 2-D grid is stored as one x plane (%d given)", alpha->nx);
  XLB_HIP(hipSetDevice(s->ctx->device));
  const size_t n = alpha->cells();
  if (alpha->nx != s->galpha_nx || alpha->ny != s->galpha_ny || alpha->nz != s->galpha_nz) {
    // a new grid starts a new gradient (hipFree inside alloc waits for launches that still write the old one)
    if (n != s->galpha_cells) XLB_HIP(s->galpha.alloc(n * sizeof(double)));
    XLB_HIP(hipMemsetAsync(s->galpha.get(), 0, n * sizeof(double), s->ctx->stream));
    s->galpha_cells = n;
    s->galpha_nx = alpha->nx;
    s->galpha_ny = alpha->ny;
    s->galpha_nz = alpha->nz;
  }
  s->alpha = alpha;
  return 0;
}

int xlbhip_porous_step(xlbhip_porous* s, const xlbhip_field* f_src, xlbhip_field* f_dst, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask,
                       double omega, int64_t timestep) {
  (void)timestep;  // (no time-dependent walls in the porous step)
  if (int rc = check_forward_fields(s, f_src, f_dst, bc_mask, missing_mask)) return rc;
  if (int rc = check_relaxation("omega", omega)) return rc;
  XLB_HIP(hipSetDevice(s->ctx->device));
  return porous_step_once(s, f_src, f_dst, bc_mask, missing_mask, omega);
}

int xlbhip_porous_run(xlbhip_porous* s, xlbhip_field* f_a, xlbhip_field* f_b, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega,
                      int64_t first_timestep, int64_t n_steps, int* result_in_b) {
  (void)first_timestep;
  XLB_REQUIRE(result_in_b && n_steps >= 0, "bad argument");
  if (int rc = check_forward_fields(s, f_a, f_b, bc_mask, missing_mask)) return rc;
  if (int rc = check_relaxation("omega", omega)) return rc;
  XLB_HIP(hipSetDevice(s->ctx->device));
  return run_alternating(n_steps, result_in_b, [&](int64_t, bool odd) {
    return odd ? porous_step_once(s, f_b, f_a, bc_mask, missing_mask, omega) : porous_step_once(s, f_a, f_b, bc_mask, missing_mask, omega);
  });
}

int xlbhip_porous_adjoint_step(xlbhip_porous* s, const xlbhip_field* f_n, const xlbhip_field* lam_in, xlbhip_field* lam_out, const xlbhip_field* bc_mask,
                               const xlbhip_field* missing_mask, double omega) {
  XLB_REQUIRE(f_n, "null argument");
  if (int rc = check_adjoint_fields(s, f_n, lam_in, lam_out, bc_mask, missing_mask)) return rc;
  if (int rc = check_relaxation("omega", omega)) return rc;
  XLB_HIP(hipSetDevice(s->ctx->device));
  if (int rc = ensure_partials(s, f_n)) return rc;
  if (int rc = ensure_gather_mask(s, bc_mask, missing_mask)) return rc;
  const size_t stride = lam_out->plane_stride, elems = stride * (size_t)lattice_q(s->lattice);
  if (elems > s->mu_elems) {
    XLB_HIP(s->mu.alloc(elems * dtype_size(s->sdt)));
    s->mu_elems = elems;
  }
  touch(lam_out);
  if (int rc = porous_adjoint_launch_once(s, f_n, lam_in->data, lam_in->plane_stride, s->mu.get(), stride, f_n, bc_mask, missing_mask, omega, ADJ_IN_LAMBDA,
                                          ADJ_OUT_MU))
    return rc;
  return porous_adjoint_launch_once(s, nullptr, s->mu.get(), stride, lam_out->data, stride, lam_out, bc_mask, missing_mask, omega, ADJ_IN_MU, ADJ_OUT_LAMBDA);
}

int xlbhip_porous_adjoint_run(xlbhip_porous* s, int64_t n_states, const xlbhip_field* const* states, xlbhip_field* lam_a, xlbhip_field* lam_b,
                              const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega, int* result_in_b) {
  XLB_REQUIRE(result_in_b && n_states >= 0 && (n_states == 0 || states), "bad argument");
  if (int rc = check_adjoint_fields(s, nullptr, lam_a, lam_b, bc_mask, missing_mask)) return rc;
  for (int64_t i = 0; i < n_states; ++i) {
    XLB_REQUIRE(states[i] && states[i] != lam_a && states[i] != lam_b, "porous adjoint run: state %lld is null or one of the cotangent fields", (long long)i);
    if (int rc = check_adjoint_fields(s, states[i], lam_a, lam_b, bc_mask, missing_mask)) return rc;
  }
  if (int rc = check_relaxation("omega", omega)) return rc;
  *result_in_b = 0;
  if (n_states == 0) return 0;
  XLB_HIP(hipSetDevice(s->ctx->device));
  if (int rc = ensure_partials(s, lam_a)) return rc;
  if (int rc = ensure_gather_mask(s, bc_mask, missing_mask)) return rc;
  touch(lam_a);
  touch(lam_b);
  // lam_N -> mu_{N-1} -> ... -> mu_0 -> lam_0: n_states launches that read a forward state, then the transposed streaming alone
  xlbhip_field *cur = lam_a, *oth = lam_b;
  for (int64_t i = n_states - 1; i >= 0; --i) {
    const int in_mode = i == n_states - 1 ? ADJ_IN_LAMBDA : ADJ_IN_MU;
    if (int rc = porous_adjoint_launch_once(s, states[i], cur->data, cur->plane_stride, oth->data, oth->plane_stride, cur, bc_mask, missing_mask, omega, in_mode,
                                            ADJ_OUT_MU))
      return rc;
    std::swap(cur, oth);
  }
  if (int rc = porous_adjoint_launch_once(s, nullptr, cur->data, cur->plane_stride, oth->data, oth->plane_stride, cur, bc_mask, missing_mask, omega, ADJ_IN_MU,
                                          ADJ_OUT_LAMBDA))
    return rc;
  std::swap(cur, oth);
  *result_in_b = cur == lam_b ? 1 : 0;
  return 0;
}

int xlbhip_porous_adjoint_reset(xlbhip_porous* s) {
  XLB_REQUIRE(s, "null argument");
  XLB_HIP(hipSetDevice(s->ctx->device));
  XLB_HIP(hipMemsetAsync(s->domega.get(), 0, sizeof(double), s->ctx->stream));
  if (s->galpha_cells) XLB_HIP(hipMemsetAsync(s->galpha.get(), 0, s->galpha_cells * sizeof(double), s->ctx->stream));
  return 0;
}

int xlbhip_porous_omega_gradient(xlbhip_porous* s, double* out) {
  XLB_REQUIRE(s && out, "null argument");
  XLB_HIP(hipSetDevice(s->ctx->device));
  XLB_HIP(hipMemcpyAsync(out, s->domega.get(), sizeof(double), hipMemcpyDeviceToHost, s->ctx->stream));
  XLB_HIP(hipStreamSynchronize(s->ctx->stream));
  return 0;
}

int xlbhip_porous_solidity_gradient(xlbhip_porous* s, xlbhip_field* out) {
  XLB_REQUIRE(s && out, "null argument");
  XLB_REQUIRE(s->alpha, "porous adjoint: no solidity field is bound (xlbhip_porous_set_solidity)");
  XLB_REQUIRE(out->dtype == XLBHIP_F64 && out->card == 1 && out->halo == 0 && same_grid(out, s->alpha),
              "porous adjoint: the solidity gradient goes to an fp64 field of one value per cell on the solidity's grid, without ghost planes");
  XLB_HIP(hipSetDevice(s->ctx->device));
  touch(out);
  XLB_HIP(hipMemcpyAsync(out->data, s->galpha.get(), s->galpha_cells * sizeof(double), hipMemcpyDeviceToDevice, s->ctx->stream));
  return 0;
}

}  // extern "C"
