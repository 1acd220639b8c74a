// libxlbhip: the discrete adjoint of the fused BGK step.  The object owns the boundary tables (a BcTables like a stepper's,
// stepper_tables.hpp), the carried-state scratch field of a single adjoint step, the per-block partial sums and the device scalar dL/domega;
// a step enqueues its kernels on the context's compute stream, and only omega_gradient waits for the device.
#include "adjoint_launch.hpp"
#include "stepper_tables.hpp"

using namespace xlb;

struct xlbhip_adjoint : RowStepper {
  DeviceBuf mu;          // the carried state between the two launches of a single step (store dtype, q planes)
  size_t mu_elems = 0;
  DeviceBuf partial;     // fp64 [blocks], then [chunks of blocks]: the two levels below the device scalar
  size_t partial_n = 0;
  DeviceBuf domega;      // fp64 [1]: the omega terms of every step since the last reset, summed in step order
  // gather bits of the transposed streaming (adjoint_kernels.hpp: k_adjoint_gather_mask), valid for these contents of the two masks
  DeviceBuf gmask;
  const void *gmask_bc = nullptr, *gmask_miss = nullptr;
  uint64_t gmask_bc_version = 0, gmask_miss_version = 0;
  size_t gmask_cells = 0;
};

namespace xlb {

// Sums of chunks of ADJ_CHUNK partials, in an order fixed by their number: block b adds up in[b * ADJ_CHUNK ..] (strided sequential
// sums of its ADJ_BLOCK threads, then the tree).  accumulate == 0: out[b] = the chunk's sum; else (one block) *out += the sum.
constexpr unsigned ADJ_CHUNK = 16 * ADJ_BLOCK;
__global__ void __launch_bounds__(ADJ_BLOCK) k_adjoint_reduce(const double* in, unsigned n, double* out, int accumulate) {
  const unsigned begin = blockIdx.x * ADJ_CHUNK, end = begin + ADJ_CHUNK < n ? begin + ADJ_CHUNK : n;
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

static int check_adjoint_fields(const xlbhip_adjoint* s, const xlbhip_field* f_n, const xlbhip_field* lin, const xlbhip_field* lout, const xlbhip_field* bcm,
                                const xlbhip_field* miss) {
  XLB_REQUIRE(s && lin && lout, "null argument");
  XLB_REQUIRE(lin != lout && lin->data != lout->data, "lam_in and lam_out must be different fields");
  // (f_n may be null: a launch that leaves lam reads no forward state; every field's stride goes to the kernel, so they may differ)
  if (int rc = check_row_fields("adjoint step", "state and cotangent fields", lattice_q(s->lattice), s->sdt, {f_n, lin, lout}, false)) return rc;
  return check_single_rank_grid("adjoint step", "kernel", s->lattice, s->bc.n_bc, lin, bcm, miss);
}

static int ensure_partials(xlbhip_adjoint* s, const xlbhip_field* f) {
  const size_t n = adjoint_blocks(f->nx, f->ny, f->nz);
  if (n > s->partial_n) {
    XLB_HIP(s->partial.alloc((n + (n + ADJ_CHUNK - 1) / ADJ_CHUNK) * sizeof(double)));  // (hipFree inside waits for launches that still write the old one)
    s->partial_n = n;
  }
  return 0;
}

// the gather bits for this pair of masks: built on first use and again when either mask was written since
static int ensure_gather_mask(xlbhip_adjoint* s, const xlbhip_field* bcm, const xlbhip_field* miss) {
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

// one launch: `in` (lam or mu, by in_mode) -> `out` (mu or lam, by out_mode), f_n for the launches that leave mu; a launch that
// leaves mu adds its omega terms to the device scalar
static int adjoint_launch_once(xlbhip_adjoint* s, const xlbhip_field* f_n, const void* in, size_t in_stride, void* out, size_t out_stride,
                               const xlbhip_field* grid_of, const xlbhip_field* bcm, const xlbhip_field* miss, double omega, int in_mode, int out_mode) {
  xlbhip_ctx* c = s->ctx;
  AdjointLaunch q = {};
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
  const int rc = launch_for_lattice(s->lattice, launch_adjoint_d2q9, launch_adjoint_d3q19, launch_adjoint_d3q27, q);
  if (rc || out_mode != ADJ_OUT_MU) return rc;
  // the step's omega terms: per-block partials -> per-chunk sums -> the device scalar (a chunk per block; one block at the end)
  const unsigned n = (unsigned)adjoint_blocks(p.nx, p.ny, p.nz), chunks = (n + ADJ_CHUNK - 1) / ADJ_CHUNK;
  double* part = s->partial.get<double>();
  if (chunks > 1) {
    XLB_REQUIRE(chunks <= ADJ_CHUNK, "adjoint step: %u blocks are more than the omega sum's two levels take", n);
    hipLaunchKernelGGL(k_adjoint_reduce, chunks, ADJ_BLOCK, 0, c->stream, part, n, part + n, 0);
    XLB_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_adjoint_reduce, 1, ADJ_BLOCK, 0, c->stream, part + n, chunks, s->domega.get<double>(), 1);
  } else {
    hipLaunchKernelGGL(k_adjoint_reduce, 1, ADJ_BLOCK, 0, c->stream, part, n, s->domega.get<double>(), 1);
  }
  XLB_HIP(hipGetLastError());
  return 0;
}

}  // namespace xlb

extern "C" {

int xlbhip_adjoint_create(xlbhip_ctx* c, int lattice, int cdt, int sdt, int n_bc, const xlbhip_bc_desc* bcs, xlbhip_adjoint** out) {
  const auto refusal = [](int kind) {
    return bc_adjoint_accepts(kind) ? nullptr
                                    : "adjoint step: bc kind %d is not supported (equilibrium, halfway and fullway bounce-back and do-nothing only)";
  };
  const auto own = [](xlbhip_adjoint& s) {
    XLB_HIP(s.domega.alloc(sizeof(double)));
    XLB_HIP(hipMemset(s.domega.get(), 0, sizeof(double)));
    return 0;
  };
  return create_row_stepper(c, lattice, cdt, sdt, n_bc, bcs, ADJOINT_POLICY_SUBJECT, refusal, own, out);
}

int xlbhip_adjoint_destroy(xlbhip_adjoint* s) { return destroy_drained(s); }

int xlbhip_adjoint_step(xlbhip_adjoint* s, const xlbhip_field* f_n, const xlbhip_field* lam_in, xlbhip_field* lam_out, const xlbhip_field* bc_mask,
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
  if (int rc = adjoint_launch_once(s, f_n, lam_in->data, lam_in->plane_stride, s->mu.get(), stride, f_n, bc_mask, missing_mask, omega, ADJ_IN_LAMBDA, ADJ_OUT_MU))
    return rc;
  return adjoint_launch_once(s, nullptr, s->mu.get(), stride, lam_out->data, stride, lam_out, bc_mask, missing_mask, omega, ADJ_IN_MU, ADJ_OUT_LAMBDA);
}

int xlbhip_adjoint_run(xlbhip_adjoint* s, int64_t n_states, const xlbhip_field* const* states, xlbhip_field* lam_a, xlbhip_field* lam_b,
                       const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega, int* result_in_b) {
  XLB_REQUIRE(result_in_b && n_states >= 0 && (n_states == 0 || states), "bad argument");
  if (int rc = check_adjoint_fields(s, nullptr, lam_a, lam_b, bc_mask, missing_mask)) return rc;
  for (int64_t i = 0; i < n_states; ++i) {
    XLB_REQUIRE(states[i] && states[i] != lam_a && states[i] != lam_b, "adjoint run: state %lld is null or one of the cotangent fields", (long long)i);
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
    if (int rc = adjoint_launch_once(s, states[i], cur->data, cur->plane_stride, oth->data, oth->plane_stride, cur, bc_mask, missing_mask, omega, in_mode, ADJ_OUT_MU))
      return rc;
    std::swap(cur, oth);
  }
  if (int rc = adjoint_launch_once(s, nullptr, cur->data, cur->plane_stride, oth->data, oth->plane_stride, cur, bc_mask, missing_mask, omega, ADJ_IN_MU, ADJ_OUT_LAMBDA))
    return rc;
  std::swap(cur, oth);
  *result_in_b = cur == lam_b ? 1 : 0;
  return 0;
}

int xlbhip_adjoint_omega_gradient(xlbhip_adjoint* s, double* out) {
  XLB_REQUIRE(s && out, "null argument");
  XLB_HIP(hipSetDevice(s->ctx->device));
  XLB_HIP(hipMemcpyAsync(out, s->domega.get(), sizeof(double), hipMemcpyDeviceToHost, s->ctx->stream));
  XLB_HIP(hipStreamSynchronize(s->ctx->stream));
  return 0;
}

int xlbhip_adjoint_reset(xlbhip_adjoint* s) {
  XLB_REQUIRE(s, "null argument");
  XLB_HIP(hipSetDevice(s->ctx->device));
  XLB_HIP(hipMemsetAsync(s->domega.get(), 0, sizeof(double), s->ctx->stream));
  return 0;
}

int xlbhip_macroscopic_adjoint(xlbhip_ctx* c, int lattice, int compute_dtype, const xlbhip_field* f, const xlbhip_field* rho_bar, const xlbhip_field* u_bar,
                               xlbhip_field* lam) {
  XLB_REQUIRE(c && f && lam, "null argument");
  XLB_REQUIRE(lattice_q(lattice) > 0, "unknown lattice %d", lattice);
  XLB_REQUIRE(compute_dtype == XLBHIP_F32 || compute_dtype == XLBHIP_F64, "bad compute dtype %d", compute_dtype);
  XLB_CHECK_POP(f, lattice, "macroscopic_adjoint(f)");
  XLB_CHECK_POP(lam, lattice, "macroscopic_adjoint(lam)");
  XLB_REQUIRE(same_grid(lam, f) && lam->halo == 0 && f->halo == 0 && lam != f, "macroscopic_adjoint: lam must be another field on f's grid, without ghost planes");
  XLB_REQUIRE(!rho_bar || (is_float(rho_bar->dtype) && rho_bar->card == 1 && same_grid(rho_bar, f) && rho_bar->halo == 0), "macroscopic_adjoint: bad dL/drho field");
  XLB_REQUIRE(!u_bar || (is_float(u_bar->dtype) && u_bar->card == lattice_d(lattice) && same_grid(u_bar, f) && u_bar->halo == 0),
              "macroscopic_adjoint: bad dL/du field");
  XLB_HIP(hipSetDevice(c->device));
  touch(lam);
  const size_t n = f->cells();
  return by_lattice(lattice, [&](auto L) {
    return by_compute(compute_dtype, [&](auto T) {
      using TT = decltype(T);
      hipLaunchKernelGGL((k_macroscopic_adjoint<decltype(L), TT>), blocks_for(n), 256, 0, c->stream, view(f), view(rho_bar), view(u_bar), view(lam), dims(f));
      XLB_HIP(hipGetLastError());
      return 0;
    });
  });
}

}  // extern "C"
