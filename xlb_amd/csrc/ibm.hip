// libxlbhip: the immersed-boundary stepper (reference: xlb/operator/stepper/ibm_stepper.py).  One call = the ordinary step of a
// stepper, then the coupling of ibm_kernels.hpp on the field the step wrote.  The object owns the markers, their footprint and the
// per-footprint-cell scratch; everything it enqueues goes to the context's compute stream and nothing in a call waits for the device.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>

#include "api_internal.hpp"
#include "ibm_dynamics_kernels.hpp"
#include "ibm_kernels.hpp"
#include "ibm_motion_kernels.hpp"
#include "ibm_state.hpp"
#include "stepper_tables.hpp"

using namespace xlb;

struct xlbhip_ibm {
  xlbhip_ctx* ctx = nullptr;
  xlbhip_stepper* stepper = nullptr;
  int lattice = 0, cdt = 0, sdt = 0;
  int nx = 0, ny = 0, nz = 0;
  int max_sweeps = 0;
  double tolerance = 0.0, relaxation = 1.0;
  IbmMarkers markers;
  IbmFootprint fp;
  IbmBodies bodies;
  size_t csize() const { return cdt == XLBHIP_F32 ? 4 : 8; }
  size_t cells() const { return (size_t)nx * ny * nz; }
};

namespace xlb {

// f(L{}, T{}, S{}) for the object's lattice, compute and store dtypes (3-D lattices; fp32 / fp64 stores)
template <class Fn>
static int ibm_dispatch(const xlbhip_ibm* b, Fn&& f) {
  auto by_types = [&](auto L) {
    if (b->cdt == XLBHIP_F32) return f(L, float{}, float{});
    if (b->sdt == XLBHIP_F32) return f(L, double{}, float{});
    return f(L, double{}, double{});
  };
  return b->lattice == XLBHIP_D3Q19 ? by_types(D3Q19{}) : by_types(D3Q27{});
}

static int ibm_clear_footprint(xlbhip_ibm* b) {
  IbmFootprint& fp = b->fp;
  if (fp.cap == 0) return 0;
  hipLaunchKernelGGL(k_ibm_clear, blocks_for((size_t)fp.cap), 256, 0, b->ctx->stream, fp.map.get<int32_t>(), fp.list.get<uint32_t>(), fp.count.get<int>(), fp.cap);
  XLB_HIP(hipGetLastError());
  XLB_HIP(hipMemsetAsync(fp.count.get(), 0, sizeof(int), b->ctx->stream));
  return 0;
}

// buffers for n markers (the old footprint has been cleared out of the map)
static int ibm_resize(xlbhip_ibm* b, int64_t n) {
  IbmMarkers& m = b->markers;
  IbmFootprint& fp = b->fp;
  m.n = 0;
  fp.cap = 0;
  m.host_pos.clear();
  b->bodies.pos0_valid = false;
  if (n == 0) return 0;
  const int64_t cap = (int64_t)std::min<size_t>((size_t)n * 64, b->cells());
  const size_t cs = b->csize();
  hipStream_t st = b->ctx->stream;
  XLB_HIP(m.pos.alloc((size_t)n * 3 * sizeof(float)));
  if (int rc = alloc_zeroed(m.area, (size_t)n * sizeof(float), st)) return rc;
  if (int rc = alloc_zeroed(m.vel, (size_t)n * 3 * sizeof(float), st)) return rc;
  XLB_HIP(m.stage.buf.alloc((size_t)n * 7 * sizeof(float)));
  XLB_HIP(fp.list.alloc((size_t)cap * sizeof(uint32_t)));
  XLB_HIP(fp.wbits.alloc((size_t)cap * 4));
  XLB_HIP(fp.W.alloc((size_t)cap * 8));
  XLB_HIP(fp.acc.alloc((size_t)cap * 3 * 8));
  XLB_HIP(fp.u.alloc((size_t)cap * 3 * cs));
  if (int rc = alloc_zeroed(fp.G, (size_t)cap * 3 * cs, st)) return rc;
  XLB_HIP(fp.dk.alloc((size_t)n * 3 * cs));
  if (int rc = alloc_zeroed(fp.F, (size_t)n * 3 * cs, st)) return rc;
  m.n = n;
  fp.cap = cap;
  return 0;
}

// cell <-> slot mapping and weight sums of the markers' current positions
static int ibm_build_footprint(xlbhip_ibm* b) {
  hipStream_t st = b->ctx->stream;
  IbmFootprint& fp = b->fp;
  if (int rc = ibm_clear_footprint(b)) return rc;
  XLB_HIP(hipMemsetAsync(fp.wbits.get(), 0, (size_t)fp.cap * 4, st));
  XLB_HIP(hipMemsetAsync(fp.W.get(), 0, (size_t)fp.cap * 8, st));
  XLB_HIP(hipMemsetAsync(fp.acc.get(), 0, (size_t)fp.cap * 3 * 8, st));
  const Dims d{b->nx, b->ny, b->nz};
  const float* pos = b->markers.pos.get<float>();
  const int64_t n = b->markers.n;
  return by_compute(b->cdt, [&](auto T) {
    using TT = decltype(T);
    hipLaunchKernelGGL((k_ibm_mark<TT>), blocks_for((size_t)n * 64), 256, 0, st, pos, n, d, fp.map.get<int32_t>(), fp.list.get<uint32_t>(), fp.count.get<int>(),
                       fp.cap);
    XLB_HIP(hipGetLastError());
    hipLaunchKernelGGL((k_ibm_wmax<TT>), blocks_for((size_t)n * 64), 256, 0, st, pos, n, d, fp.map.get<int32_t>(), fp.wbits.get<unsigned>(), fp.cap);
    XLB_HIP(hipGetLastError());
    hipLaunchKernelGGL((k_ibm_weights<TT>), blocks_for((size_t)n * 64), 256, 0, st, pos, n, d, fp.map.get<int32_t>(), fp.wbits.get<unsigned>(),
                       fp.W.get<unsigned long long>(), fp.cap);
    XLB_HIP(hipGetLastError());
    return 0;
  });
}

// the coupling on f (the field a step has just written)
static int ibm_couple(xlbhip_ibm* b, xlbhip_field* f) {
  hipStream_t st = b->ctx->stream;
  IbmFootprint& fp = b->fp;
  const int64_t n = b->markers.n;
  XLB_HIP(hipMemsetAsync(fp.ctl.get(), 0, sizeof(IbmControl), st));
  if (n == 0 || b->max_sweeps == 0) return 0;
  const Dims d{b->nx, b->ny, b->nz};
  const unsigned slot_blocks = blocks_for((size_t)fp.cap), marker_blocks = blocks_for((size_t)n), pair_blocks = blocks_for((size_t)n * 64);
  const int residual_on = b->tolerance > 0.0 ? 1 : 0;
  IbmControl* ctl = fp.ctl.get<IbmControl>();
  const int rc = ibm_dispatch(b, [&](auto L, auto T, auto S) {
    using LL = decltype(L);
    using TT = decltype(T);
    using SS = decltype(S);
    const float* pos = b->markers.pos.get<float>();
    const int32_t* map = fp.map.get<int32_t>();
    const int* count = fp.count.get<int>();
    unsigned long long* acc = fp.acc.get<unsigned long long>();
    TT* u = fp.u.get<TT>();
    TT* G = fp.G.get<TT>();
    TT* F = fp.F.get<TT>();
    TT* dk = fp.dk.get<TT>();
    hipLaunchKernelGGL((k_ibm_moments<LL, TT, SS>), slot_blocks, 256, 0, st, static_cast<const SS*>(f->data), f->plane_stride, fp.list.get<uint32_t>(), count,
                       fp.cap, u);
    XLB_HIP(hipGetLastError());
    hipLaunchKernelGGL((k_ibm_interp<TT>), marker_blocks, 256, 0, st, pos, b->markers.vel.get<float>(), n, d, map, fp.cap, u, dk, F);
    XLB_HIP(hipGetLastError());
    for (int it = 0; it < b->max_sweeps; ++it) {
      if (it > 0) {  // (the forces are zero in the first sweep: nothing to spread, acc is zero already)
        hipLaunchKernelGGL((k_ibm_spread<TT>), pair_blocks, 256, 0, st, it, residual_on, ctl, pos, b->markers.area.get<float>(), F, n, d, map, fp.cap,
                           fp.wbits.get<unsigned>(), acc);
        XLB_HIP(hipGetLastError());
      }
      hipLaunchKernelGGL((k_ibm_correct<TT>), slot_blocks, 256, 0, st, it, residual_on, ctl, count, fp.cap, fp.wbits.get<unsigned>(), fp.W.get<unsigned long long>(), acc,
                         u, (TT)b->relaxation, G);
      XLB_HIP(hipGetLastError());
      hipLaunchKernelGGL((k_ibm_update<TT>), marker_blocks, 256, 0, st, it, residual_on, ctl, n, dk, F, (TT)(b->tolerance * b->tolerance));
      XLB_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL((k_ibm_apply<LL, TT, SS>), slot_blocks, 256, 0, st, static_cast<SS*>(f->data), f->plane_stride, fp.list.get<uint32_t>(), count, fp.cap, G);
    XLB_HIP(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  touch(f);
  return 0;
}

// ---- rigid bodies ---------------------------------------------------------------------------------------------------------------
// the live pose table of a timestep (and the next row of a recorded pose history); staged == nullptr outside a step
static int ibm_live_pose(xlbhip_ibm* b, const double* staged, bool record) {
  IbmBodies& bd = b->bodies;
  double* row = record ? bd.pose_hist.next_row() : nullptr;
  hipLaunchKernelGGL(k_ibm_pose, 1, IBM_MAX_BODIES, 0, b->ctx->stream, bd.kind.get<int32_t>(), bd.rotate.get<int32_t>(), bd.dyn_state.get<double>(),
                     bd.dyn_params.get<double>(), staged, bd.rest_pose.get<double>(), bd.n, bd.live_pose.get<double>(), row);
  XLB_HIP(hipGetLastError());
  return 0;
}

// the dynamic bodies from the state of timestep t to that of t + 1, with the loads the step has just left
static int ibm_integrate(xlbhip_ibm* b) {
  IbmBodies& bd = b->bodies;
  const IbmIntegrator which = bd.plan.integrator();
  if (which == IbmIntegrator::NONE) return 0;
  if (which == IbmIntegrator::CONTACT)
    hipLaunchKernelGGL(k_ibm_integrate_contact, 1, IBM_MAX_BODIES, 0, b->ctx->stream, bd.kind.get<int32_t>(), bd.rotate.get<int32_t>(),
                       bd.dyn_params.get<double>(), bd.loads.get<double>(), bd.n, bd.dyn_state.get<double>(), bd.status.get<unsigned long long>(),
                       bd.virt.get<double>(), bd.prev.get<double>(), bd.plan.passes_radius() ? bd.radius.get<double>() : nullptr, bd.contact_model,
                       bd.live_pose.get<double>(), bd.contact.get<double>());
  else
    hipLaunchKernelGGL(k_ibm_integrate, 1, IBM_MAX_BODIES, 0, b->ctx->stream, bd.kind.get<int32_t>(), bd.rotate.get<int32_t>(), bd.dyn_params.get<double>(),
                       bd.loads.get<double>(), bd.n, bd.dyn_state.get<double>(), bd.status.get<unsigned long long>());
  XLB_HIP(hipGetLastError());
  return 0;
}

// the markers of the moving bodies to their place at timestep t, then the footprint of the new positions
static int ibm_move(xlbhip_ibm* b, int64_t t) {
  IbmBodies& bd = b->bodies;
  IbmMarkers& m = b->markers;
  if (!bd.plan.moves()) return 0;
  hipLaunchKernelGGL(k_ibm_move, blocks_for((size_t)m.n), 256, 0, b->ctx->stream, bd.pos0.get<float>(), bd.move_id.get<int32_t>(), bd.pose_at(t),
                     bd.centre0.get<double>(), m.n, m.pos.get<float>(), m.vel.get<float>());
  XLB_HIP(hipGetLastError());
  m.host_pos.clear();  // the device holds other positions than the caller passed last: the next ones are never "the same"
  return ibm_build_footprint(b);
}

// force and torque on every body from the forces the coupling left, to `loads` and to the next row of a recorded history
static int ibm_body_loads(xlbhip_ibm* b, int64_t t) {
  IbmBodies& bd = b->bodies;
  if (bd.n == 0) return 0;
  hipStream_t st = b->ctx->stream;
  const double* pose = bd.pose_at(t);
  double* row = bd.loads_hist.next_row();
  return by_compute(b->cdt, [&](auto T) {
    using TT = decltype(T);
    if (bd.n_chunks > 0) {
      hipLaunchKernelGGL((k_ibm_loads<TT>), (unsigned)bd.n_chunks, IBM_LOADS_CHUNK, 0, st, bd.chunks.get<IbmLoadChunk>(), b->fp.F.get<TT>(),
                         b->markers.area.get<float>(), b->markers.pos.get<float>(), pose, bd.partial.get<double>());
      XLB_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ibm_loads_combine, blocks_for((size_t)bd.n * 6), 256, 0, st, bd.chunk0.get<int32_t>(), bd.partial.get<double>(), bd.n,
                       bd.loads.get<double>(), row);
    XLB_HIP(hipGetLastError());
    return 0;
  });
}

static int ibm_check_field(const xlbhip_ibm* b, const xlbhip_field* f) {
  XLB_REQUIRE(f, "null field");
  XLB_REQUIRE(f->halo == 0, "the immersed-boundary stepper does not run on slab-decomposed fields (ghost planes)");
  XLB_REQUIRE(f->nx == b->nx && f->ny == b->ny && f->nz == b->nz, "field of %d x %d x %d cells, the immersed-boundary stepper was made for %d x %d x %d", f->nx,
              f->ny, f->nz, b->nx, b->ny, b->nz);
  XLB_REQUIRE(f->dtype == b->sdt && f->card == lattice_q(b->lattice), "population field does not match the immersed-boundary stepper's lattice / store dtype");
  return 0;
}

// what the setters of the bodies do once their arguments are checked: queued steps read the tables they replace
static int ibm_drain(xlbhip_ibm* b) {
  XLB_HIP(hipSetDevice(b->ctx->device));
  XLB_HIP(hipStreamSynchronize(b->ctx->stream));
  return 0;
}

}  // namespace xlb

extern "C" {

int xlbhip_ibm_create(xlbhip_ctx* c, xlbhip_stepper* stepper, int lattice, int compute_dtype, int store_dtype, int nx, int ny, int nz,
                      int max_iterations, double tolerance, double relaxation, xlbhip_ibm** out) {
  XLB_REQUIRE(c && stepper && out, "null argument");
  XLB_REQUIRE(lattice == XLBHIP_D3Q19 || lattice == XLBHIP_D3Q27, "the immersed-boundary stepper needs a 3-D lattice (2-D grids are not supported)");
  XLB_REQUIRE(compute_dtype == XLBHIP_F32 || compute_dtype == XLBHIP_F64, "bad compute dtype %d", compute_dtype);
  XLB_REQUIRE(store_dtype == XLBHIP_F32 || store_dtype == XLBHIP_F64, "the immersed-boundary stepper does not support fp16 storage");
  XLB_REQUIRE(dtype_size(store_dtype) <= dtype_size(compute_dtype), "bad store dtype %d for compute dtype %d", store_dtype, compute_dtype);
  XLB_REQUIRE(nx > 0 && ny > 0 && nz > 0 && (size_t)nx * ny * nz < ((size_t)1 << 31), "bad grid %d x %d x %d", nx, ny, nz);
  XLB_REQUIRE(max_iterations >= 0 && max_iterations <= IBM_MAX_SWEEPS, "ibm_max_iterations must be 0 .. %d", IBM_MAX_SWEEPS);
  XLB_REQUIRE(tolerance >= 0.0, "ibm_tolerance must not be negative");
  XLB_HIP(hipSetDevice(c->device));
  auto b = std::make_unique<xlbhip_ibm>();
  b->ctx = c;
  b->stepper = stepper;
  b->lattice = lattice;
  b->cdt = compute_dtype;
  b->sdt = store_dtype;
  b->nx = nx;
  b->ny = ny;
  b->nz = nz;
  b->max_sweeps = max_iterations;
  b->tolerance = tolerance;
  b->relaxation = relaxation;
  XLB_HIP(b->fp.map.alloc(b->cells() * sizeof(int32_t)));
  XLB_HIP(hipMemsetAsync(b->fp.map.get(), 0xff, b->cells() * sizeof(int32_t), c->stream));  // every cell: no slot (-1)
  if (int rc = alloc_zeroed(b->fp.count, sizeof(int), c->stream)) return rc;
  if (int rc = alloc_zeroed(b->fp.ctl, sizeof(IbmControl), c->stream)) return rc;
  if (int rc = b->markers.stage.create(c->stream)) return rc;
  if (int rc = b->bodies.pose_stage.create(c->stream)) return rc;
  *out = b.release();
  return 0;
}

int xlbhip_ibm_destroy(xlbhip_ibm* b) {
  return destroy_drained(b);  // (the drain: copies may still read the pinned buffers)
}

int xlbhip_ibm_set_markers(xlbhip_ibm* b, int64_t n, const float* positions, const float* areas, const float* velocities) {
  XLB_REQUIRE(b && n >= 0, "bad argument");
  XLB_REQUIRE((size_t)n < ((size_t)1 << 25), "too many markers (%lld)", (long long)n);
  xlbhip_ctx* c = b->ctx;
  IbmMarkers& m = b->markers;
  IbmBodies& bd = b->bodies;
  XLB_HIP(hipSetDevice(c->device));
  if (n != m.n) {
    XLB_REQUIRE(bd.n == 0, "the number of markers (%lld -> %lld) cannot change while bodies are declared: clear them first", (long long)m.n, (long long)n);
    XLB_REQUIRE(n == 0 || (positions && areas && velocities), "a new number of markers needs positions, areas and velocities");
    if (int rc = ibm_clear_footprint(b)) return rc;
    XLB_HIP(hipStreamSynchronize(c->stream));
    if (int rc = ibm_resize(b, n)) return rc;
  }
  if (n == 0) return 0;
  if (int rc = m.stage.wait()) return rc;
  float* pin = m.stage.buf.get<float>();
  const size_t n3 = m.bytes3();
  bool moved = false;
  if (positions) {
    // (k_ibm_move empties host_pos: after the device has moved the markers, no array the caller passes counts as "the same")
    moved = m.host_pos.size() != (size_t)n * 3 || std::memcmp(m.host_pos.data(), positions, n3) != 0;
    if (moved) {
      m.host_pos.assign(positions, positions + (size_t)n * 3);
      std::memcpy(pin, positions, n3);
      XLB_HIP(hipMemcpyAsync(m.pos.get(), pin, n3, hipMemcpyHostToDevice, c->stream));
      // they are the new reference positions of the bodies
      if (bd.plan.moves()) XLB_HIP(hipMemcpyAsync(bd.pos0.get(), pin, n3, hipMemcpyHostToDevice, c->stream));
      bd.pos0_valid = bd.plan.moves();
    }
  }
  if (areas) {
    std::memcpy(pin + 3 * n, areas, (size_t)n * sizeof(float));
    XLB_HIP(hipMemcpyAsync(m.area.get(), pin + 3 * n, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  }
  if (velocities) {
    std::memcpy(pin + 4 * n, velocities, n3);
    XLB_HIP(hipMemcpyAsync(m.vel.get(), pin + 4 * n, n3, hipMemcpyHostToDevice, c->stream));
  }
  if (int rc = m.stage.record(c->stream)) return rc;
  if (moved) return ibm_build_footprint(b);
  return 0;
}

int xlbhip_ibm_step(xlbhip_ibm* b, const xlbhip_field* f_src, xlbhip_field* f_dst, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask,
                    double omega, int64_t timestep) {
  XLB_REQUIRE(b, "null argument");
  const IbmBodies& bd = b->bodies;
  if (int rc = ibm_check_field(b, f_src)) return rc;
  if (int rc = ibm_check_field(b, f_dst)) return rc;
  if (int rc = bd.require_poses(timestep, 1)) return rc;
  if (bd.plan.use_live())
    if (int rc = ibm_live_pose(b, bd.plan.needs_staged() ? bd.staged_at(timestep) : nullptr, true)) return rc;
  if (int rc = ibm_move(b, timestep)) return rc;
  if (int rc = xlbhip_step(b->stepper, f_src, f_dst, bc_mask, missing_mask, omega, timestep)) return rc;
  if (int rc = ibm_couple(b, f_dst)) return rc;
  if (int rc = ibm_body_loads(b, timestep)) return rc;
  return ibm_integrate(b);
}

int xlbhip_ibm_run(xlbhip_ibm* b, xlbhip_field* f_a, xlbhip_field* f_b, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega,
                   int64_t first_timestep, int64_t n_steps, int* result_in_b) {
  XLB_REQUIRE(b && result_in_b && n_steps >= 0, "bad argument");
  if (int rc = b->bodies.require_poses(first_timestep, n_steps)) return rc;  // (before anything is enqueued)
  return run_alternating(n_steps, result_in_b, [&](int64_t i, bool odd) {
    return xlbhip_ibm_step(b, odd ? f_b : f_a, odd ? f_a : f_b, bc_mask, missing_mask, omega, first_timestep + i);
  });
}

int xlbhip_ibm_forces(xlbhip_ibm* b, int64_t n, double* forces) {
  XLB_REQUIRE(b && n == b->markers.n && (n == 0 || forces), "xlbhip_ibm_forces: expected room for %lld markers", b ? (long long)b->markers.n : 0LL);
  if (n == 0) return 0;
  std::vector<char> host((size_t)n * 3 * b->csize());
  if (int rc = read_back(b->ctx, {{host.data(), b->fp.F.get(), host.size()}})) return rc;
  by_compute(b->cdt, [&](auto T) {
    const auto* v = reinterpret_cast<const decltype(T)*>(host.data());
    for (size_t i = 0; i < (size_t)n * 3; ++i) forces[i] = (double)v[i];
    return 0;
  });
  return 0;
}

int xlbhip_ibm_iterations(xlbhip_ibm* b, int* sweeps) {
  XLB_REQUIRE(b && sweeps, "null argument");
  return read_back(b->ctx, {{sweeps, b->fp.ctl.get<char>() + offsetof(IbmControl, sweeps), sizeof(int)}});
}

int xlbhip_ibm_footprint(xlbhip_ibm* b, int64_t* n_cells, int64_t capacity, uint32_t* cells) {
  XLB_REQUIRE(b && n_cells, "null argument");
  int count = 0;
  if (int rc = read_back(b->ctx, {{&count, b->fp.count.get(), sizeof(int)}})) return rc;
  *n_cells = count;
  if (cells && count > 0) {
    XLB_REQUIRE(capacity >= count, "xlbhip_ibm_footprint: room for %lld cells, the footprint has %d", (long long)capacity, count);
    return read_back(b->ctx, {{cells, b->fp.list.get(), (size_t)count * sizeof(uint32_t)}});
  }
  return 0;
}

int xlbhip_ibm_set_bodies(xlbhip_ibm* b, int n_bodies, const int64_t* first, const int64_t* count, const int* moving, const double* centre0) {
  XLB_REQUIRE(b && n_bodies >= 0, "bad argument");
  const std::string bad = ibm_check_bodies(b->markers.n, n_bodies, first, count, moving, centre0);
  XLB_REQUIRE(bad.empty(), "%s", bad.c_str());
  if (int rc = ibm_drain(b)) return rc;
  b->bodies.forget();
  if (n_bodies == 0) return 0;
  const IbmBodyTables tables = ibm_body_tables(b->markers.n, n_bodies, first, count, moving, centre0);  // (the moving flags are checked here)
  XLB_REQUIRE(tables.error.empty(), "%s", tables.error.c_str());
  return b->bodies.declare(b->ctx->stream, tables, n_bodies, centre0, b->markers);
}

int xlbhip_ibm_set_dynamics(xlbhip_ibm* b, int n_bodies, const int* rotate, const double* params, const double* state) {
  XLB_REQUIRE(b && rotate && params && state, "null argument");
  IbmBodies& bd = b->bodies;
  XLB_REQUIRE(n_bodies == bd.n && n_bodies > 0, "xlbhip_ibm_set_dynamics: %d bodies, %d are declared (xlbhip_ibm_set_bodies)", n_bodies, bd.n);
  XLB_REQUIRE(bd.plan.any_dynamic, "xlbhip_ibm_set_dynamics: no body is declared dynamic (moving flag 2 of xlbhip_ibm_set_bodies)");
  std::vector<int32_t> modes(rotate, rotate + n_bodies);
  for (int i = 0; i < n_bodies; ++i)
    XLB_REQUIRE(modes[i] >= IBM_ROTATE_LOCKED && modes[i] <= IBM_ROTATE_FREE, "body %d: bad rotation mode %d (0 locked, 1 axis, 2 free)", i, modes[i]);
  if (int rc = ibm_drain(b)) return rc;
  if (int rc = upload_bytes(modes.data(), modes.size() * sizeof(int32_t), bd.rotate)) return rc;
  if (int rc = upload_bytes(params, bd.doubles(IBM_DYN_PARAM_DOUBLES), bd.dyn_params)) return rc;
  if (int rc = upload_bytes(state, bd.doubles(IBM_DYN_STATE_DOUBLES), bd.dyn_state)) return rc;
  if (int rc = bd.reset_extras(n_bodies, b->ctx->stream)) return rc;
  bd.plan.dynamics_set = true;
  return 0;
}

int xlbhip_ibm_set_virtual_mass(xlbhip_ibm* b, int n_bodies, const double* virtual_mass, const double* virtual_inertia) {
  XLB_REQUIRE(b && virtual_mass && virtual_inertia, "null argument");
  IbmBodies& bd = b->bodies;
  XLB_REQUIRE(n_bodies == bd.n && n_bodies > 0, "xlbhip_ibm_set_virtual_mass: %d bodies, %d are declared (xlbhip_ibm_set_bodies)", n_bodies, bd.n);
  XLB_REQUIRE(bd.plan.dynamics_set, "xlbhip_ibm_set_virtual_mass: call xlbhip_ibm_set_dynamics first");
  std::vector<double> virt((size_t)n_bodies * 2);
  bool any = false;
  for (int i = 0; i < n_bodies; ++i) {
    const double mv = virtual_mass[i], iv = virtual_inertia[i];
    XLB_REQUIRE(mv >= 0.0 && mv <= 1.7976931348623157e308, "body %d: virtual_mass %g must be finite and not negative", i, mv);
    XLB_REQUIRE(iv >= 0.0 && iv <= 1.7976931348623157e308, "body %d: virtual_inertia %g must be finite and not negative", i, iv);
    virt[2 * (size_t)i] = mv;
    virt[2 * (size_t)i + 1] = iv;
    any = any || mv > 0.0 || iv > 0.0;
  }
  if (int rc = ibm_drain(b)) return rc;
  if (int rc = upload_bytes(virt.data(), virt.size() * sizeof(double), bd.virt)) return rc;
  XLB_HIP(hipMemsetAsync(bd.prev.get(), 0, bd.doubles(6), b->ctx->stream));
  bd.plan.virtual_on = any;
  return 0;
}

int xlbhip_ibm_set_contact(xlbhip_ibm* b, int n_bodies, const double* radius, double range, double stiffness, double wall_stiffness, const double* lo,
                           const double* hi) {
  XLB_REQUIRE(b && radius, "null argument");
  IbmBodies& bd = b->bodies;
  XLB_REQUIRE(n_bodies == bd.n && n_bodies > 0, "xlbhip_ibm_set_contact: %d bodies, %d are declared (xlbhip_ibm_set_bodies)", n_bodies, bd.n);
  XLB_REQUIRE(bd.plan.dynamics_set, "xlbhip_ibm_set_contact: call xlbhip_ibm_set_dynamics first");
  XLB_REQUIRE((lo == nullptr) == (hi == nullptr), "xlbhip_ibm_set_contact: lo and hi are given together or not at all");
  const double big = 1.7976931348623157e308, inf = HUGE_VAL;
  XLB_REQUIRE(range >= 0.0 && range <= big, "xlbhip_ibm_set_contact: range %g must be finite and not negative", range);
  XLB_REQUIRE(stiffness >= 0.0 && stiffness <= big, "xlbhip_ibm_set_contact: stiffness %g must be finite and not negative", stiffness);
  XLB_REQUIRE(wall_stiffness >= 0.0 && wall_stiffness <= big, "xlbhip_ibm_set_contact: wall_stiffness %g must be finite and not negative", wall_stiffness);
  bool any = false;
  for (int i = 0; i < n_bodies; ++i) {
    XLB_REQUIRE(radius[i] >= 0.0 && radius[i] <= big, "body %d: radius %g must be finite and not negative", i, radius[i]);
    any = any || radius[i] > 0.0;
  }
  IbmContactModel model{range, stiffness, wall_stiffness, {-inf, -inf, -inf}, {inf, inf, inf}};
  for (int a = 0; lo && a < 3; ++a) {
    XLB_REQUIRE(lo[a] < hi[a], "xlbhip_ibm_set_contact: lo[%d] = %g must be below hi[%d] = %g", a, lo[a], a, hi[a]);  // (false for a NaN)
    model.lo[a] = lo[a];
    model.hi[a] = hi[a];
  }
  if (int rc = ibm_drain(b)) return rc;
  if (int rc = upload_bytes(radius, bd.doubles(1), bd.radius)) return rc;
  XLB_HIP(hipMemsetAsync(bd.contact.get(), 0, bd.doubles(3), b->ctx->stream));
  bd.contact_model = model;
  bd.plan.contact_on = any && bd.plan.any_dynamic;
  return 0;
}

int xlbhip_ibm_contact_forces(xlbhip_ibm* b, int n_bodies, double* forces) {
  XLB_REQUIRE(b && n_bodies == b->bodies.n && (n_bodies == 0 || forces), "xlbhip_ibm_contact_forces: expected room for %d bodies", b ? b->bodies.n : 0);
  if (n_bodies == 0) return 0;
  return read_back(b->ctx, {{forces, b->bodies.contact.get(), b->bodies.doubles(3)}});
}

int xlbhip_ibm_body_poses(xlbhip_ibm* b, int n_bodies, double* poses, uint64_t* status) {
  XLB_REQUIRE(b && n_bodies == b->bodies.n && status && (n_bodies == 0 || poses), "xlbhip_ibm_body_poses: expected room for %d bodies", b ? b->bodies.n : 0);
  *status = 0;
  if (n_bodies == 0) return 0;
  const IbmBodies& bd = b->bodies;
  if (int rc = bd.require_dynamics()) return rc;
  XLB_HIP(hipSetDevice(b->ctx->device));
  if (int rc = ibm_live_pose(b, nullptr, false)) return rc;
  return read_back(b->ctx, {{poses, bd.live_pose.get(), bd.doubles(IBM_POSE_DOUBLES)}, {status, bd.status.get(), sizeof(uint64_t)}});
}

int xlbhip_ibm_record_poses(xlbhip_ibm* b, int64_t n_rows) {
  XLB_REQUIRE(b && n_rows >= 0, "bad argument");
  IbmBodies& bd = b->bodies;
  XLB_REQUIRE(n_rows == 0 || bd.n > 0, "xlbhip_ibm_record_poses: no bodies are declared");
  XLB_HIP(hipSetDevice(b->ctx->device));
  const int rc = bd.pose_hist.arm(n_rows, bd.n);
  bd.plan.recording_poses = bd.pose_hist.rows > 0;
  return rc;
}

int xlbhip_ibm_poses_history(xlbhip_ibm* b, int64_t n_rows, double* poses) {
  XLB_REQUIRE(b && n_rows >= 0 && (n_rows == 0 || poses), "bad argument");
  const auto& hist = b->bodies.pose_hist;
  XLB_REQUIRE(n_rows <= hist.next, "xlbhip_ibm_poses_history: %lld rows asked for, %lld were recorded", (long long)n_rows, (long long)hist.next);
  if (n_rows == 0) return 0;
  return hist.read(b->ctx, n_rows, poses);
}

int xlbhip_ibm_stage_poses(xlbhip_ibm* b, int64_t first_timestep, int64_t n_steps, const double* poses) {
  XLB_REQUIRE(b && n_steps >= 0 && (n_steps == 0 || poses), "bad argument");
  IbmBodies& bd = b->bodies;
  XLB_REQUIRE(bd.plan.needs_staged(), "xlbhip_ibm_stage_poses: no body with prescribed motion moves (xlbhip_ibm_set_bodies)");
  const size_t bytes = (size_t)n_steps * bd.doubles(IBM_POSE_DOUBLES);
  XLB_REQUIRE(bytes <= XLBHIP_IBM_POSE_BYTES, "%lld steps x %d bodies of poses are %zu bytes, at most %d are staged at once", (long long)n_steps, bd.n, bytes,
              XLBHIP_IBM_POSE_BYTES);
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  bd.pose_count = 0;
  if (n_steps == 0) return 0;
  if (int rc = bd.pose_stage.wait()) return rc;
  std::memcpy(bd.pose_stage.buf.get(), poses, bytes);
  // (in stream order behind the steps that read the rows staged before)
  XLB_HIP(hipMemcpyAsync(bd.pose.get(), bd.pose_stage.buf.get(), bytes, hipMemcpyHostToDevice, c->stream));
  if (int rc = bd.pose_stage.record(c->stream)) return rc;
  bd.pose_first = first_timestep;
  bd.pose_count = n_steps;
  return 0;
}

int xlbhip_ibm_loads(xlbhip_ibm* b, int n_bodies, double* loads) {
  XLB_REQUIRE(b && n_bodies == b->bodies.n && (n_bodies == 0 || loads), "xlbhip_ibm_loads: expected room for %d bodies", b ? b->bodies.n : 0);
  if (n_bodies == 0) return 0;
  return read_back(b->ctx, {{loads, b->bodies.loads.get(), b->bodies.doubles(6)}});
}

int xlbhip_ibm_record_loads(xlbhip_ibm* b, int64_t n_rows) {
  XLB_REQUIRE(b && n_rows >= 0, "bad argument");
  XLB_REQUIRE(n_rows == 0 || b->bodies.n > 0, "xlbhip_ibm_record_loads: no bodies are declared");
  XLB_HIP(hipSetDevice(b->ctx->device));
  return b->bodies.loads_hist.arm(n_rows, b->bodies.n);
}

int xlbhip_ibm_loads_history(xlbhip_ibm* b, int64_t n_rows, double* loads) {
  XLB_REQUIRE(b && n_rows >= 0 && (n_rows == 0 || loads), "bad argument");
  const auto& hist = b->bodies.loads_hist;
  XLB_REQUIRE(n_rows <= hist.next, "xlbhip_ibm_loads_history: %lld rows asked for, %lld were recorded", (long long)n_rows, (long long)hist.next);
  if (n_rows == 0) return 0;
  return hist.read(b->ctx, n_rows, loads);
}

int xlbhip_ibm_download_markers(xlbhip_ibm* b, int64_t n, float* positions, float* velocities) {
  XLB_REQUIRE(b && n == b->markers.n, "xlbhip_ibm_download_markers: expected room for %lld markers", b ? (long long)b->markers.n : 0LL);
  if (n == 0) return 0;
  const IbmMarkers& m = b->markers;
  return read_back(b->ctx, {{positions, m.pos.get(), m.bytes3()}, {velocities, m.vel.get(), m.bytes3()}});
}

}  // extern "C"
