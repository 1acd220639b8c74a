// libxlbhip: the immersed-boundary stepper (reference: xlb/operator/stepper/ibm_stepper.py).  One call = the ordinary step of a
// stepper, then the coupling of ibm_kernels.hpp on the field the step wrote.  The object owns the markers, their footprint and the
// per-footprint-cell scratch; everything it enqueues goes to the context's compute stream and nothing in a call waits for the device.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <vector>

#include "api_internal.hpp"
#include "ibm_dynamics_kernels.hpp"
#include "ibm_kernels.hpp"
#include "ibm_motion_kernels.hpp"

using namespace xlb;

struct xlbhip_ibm {
  xlbhip_ctx* ctx = nullptr;
  xlbhip_stepper* stepper = nullptr;
  int lattice = 0, cdt = 0, sdt = 0;
  int nx = 0, ny = 0, nz = 0;
  int max_sweeps = 0;
  double tolerance = 0.0, relaxation = 1.0;
  int64_t n = 0;    // markers
  int64_t cap = 0;  // slots the footprint arrays hold: min(64 n, cells)
  // markers: float32 as the caller passes them; staged through ONE pinned buffer [positions 3n | areas n | velocities 3n], guarded
  // by the event of the last copy out of it
  DeviceBuf pos, area, vel;
  PinnedBuf pin;
  hipEvent_t pin_ev = nullptr;
  std::vector<float> host_pos;  // what the footprint was built from
  // footprint
  DeviceBuf map;    // int32 per grid cell: slot, or -1
  DeviceBuf list;   // uint32 [cap]: slot -> cell
  DeviceBuf count;  // int: slots in use
  DeviceBuf wbits;  // uint32 [cap]: fp32 bit pattern of the slot's largest weight (sets the slot's fixed-point quantum)
  DeviceBuf W;      // fixed point [cap]
  DeviceBuf acc;    // fixed point [cap][3]; zero between uses
  DeviceBuf u, G;   // compute dtype [cap][3]
  // per marker, compute dtype [n][3]
  DeviceBuf dk, F;
  DeviceBuf ctl;  // IbmControl
  // rigid bodies (xlbhip_ibm_set_bodies): disjoint ranges of the markers; the ones that move are placed by k_ibm_move before every step
  int n_bodies = 0;
  bool any_moving = false;
  DeviceBuf pos0;       // float [n][3]: the reference positions X0 the poses are applied to
  bool pos0_valid = false;  // false: `pos` still holds them (nothing has moved the markers since they were uploaded)
  DeviceBuf move_id;    // int32 [n]: body of the marker when that body moves, else -1
  DeviceBuf centre0;    // double [n_bodies][3]
  DeviceBuf rest_pose;  // double [n_bodies][18]: R = 1, c = centre0, w = v = 0 — what the loads read while no body moves
  // poses of the staged timesteps pose_first .. pose_first + pose_count - 1, [step][body][18]; staged through pose_pin, which pose_ev guards
  DeviceBuf pose;
  PinnedBuf pose_pin;
  hipEvent_t pose_ev = nullptr;
  int64_t pose_first = 0, pose_count = 0;
  // loads
  int64_t n_chunks = 0;
  DeviceBuf chunks;   // IbmLoadChunk [n_chunks], body after body
  DeviceBuf chunk0;   // int32 [n_bodies + 1]: first chunk of every body
  DeviceBuf partial;  // double [n_chunks][6]
  DeviceBuf loads;    // double [n_bodies][6]
  DeviceBuf hist;     // double [hist_rows][n_bodies][6], row hist_next is the next step's
  int64_t hist_rows = 0, hist_next = 0;
  // free bodies (xlbhip_ibm_set_dynamics): integrated on the device from the loads of every step (ibm_dynamics_kernels.hpp)
  bool any_prescribed = false;  // some body with markers follows staged poses
  bool any_dynamic = false;
  bool dynamics_set = false;    // the parameters and the initial state of the dynamic bodies have been uploaded
  DeviceBuf kind;        // int32 [n_bodies]: IBM_BODY_*
  DeviceBuf rotate;      // int32 [n_bodies]: IBM_ROTATE_*
  DeviceBuf dyn_state;   // double [n_bodies][16]
  DeviceBuf dyn_params;  // double [n_bodies][32]
  DeviceBuf status;      // uint64: bit b set = body b met a state that was not finite (sticky)
  DeviceBuf live_pose;   // double [n_bodies][18]: what k_ibm_pose wrote for the step under way
  DeviceBuf pose_hist;   // double [pose_hist_rows][n_bodies][18], row pose_hist_next is the next step's
  int64_t pose_hist_rows = 0, pose_hist_next = 0;
  // virtual mass and contact (xlbhip_ibm_set_virtual_mass / _set_contact): with either on, k_ibm_integrate_contact takes the place of
  // k_ibm_integrate; with neither the launches are those of a stepper that has neither
  bool virtual_on = false, contact_on = false;
  DeviceBuf virt;      // double [n_bodies][2]: m_v, I_v
  DeviceBuf prev;      // double [n_bodies][6]: a_prev | alpha_prev
  DeviceBuf radius;    // double [n_bodies]: contact radius, 0 = takes no part
  DeviceBuf contact;   // double [n_bodies][3]: the contact force of the last step
  IbmContactModel contact_model{};
  // the move and the loads read the live table (else the staged / rest rows directly: the launches of a run without free bodies and
  // without a recorded pose history are exactly those of a stepper that has neither)
  bool use_live() const { return any_dynamic || pose_hist_rows > 0; }
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
  if (b->cap == 0) return 0;
  hipLaunchKernelGGL(k_ibm_clear, blocks_for((size_t)b->cap), 256, 0, b->ctx->stream, b->map.get<int32_t>(), b->list.get<uint32_t>(), b->count.get<int>(),
                     b->cap);
  XLB_HIP(hipGetLastError());
  XLB_HIP(hipMemsetAsync(b->count.get(), 0, sizeof(int), b->ctx->stream));
  return 0;
}

// buffers for n markers (the old footprint has been cleared out of the map)
static int ibm_resize(xlbhip_ibm* b, int64_t n) {
  b->n = 0;
  b->cap = 0;
  b->host_pos.clear();
  b->pos0_valid = false;
  if (n == 0) return 0;
  const int64_t cap = (int64_t)std::min<size_t>((size_t)n * 64, b->cells());
  const size_t cs = b->csize();
  XLB_HIP(b->pos.alloc((size_t)n * 3 * sizeof(float)));
  XLB_HIP(b->area.alloc((size_t)n * sizeof(float)));
  XLB_HIP(b->vel.alloc((size_t)n * 3 * sizeof(float)));
  XLB_HIP(b->pin.alloc((size_t)n * 7 * sizeof(float)));
  XLB_HIP(b->list.alloc((size_t)cap * sizeof(uint32_t)));
  XLB_HIP(b->wbits.alloc((size_t)cap * 4));
  XLB_HIP(b->W.alloc((size_t)cap * 8));
  XLB_HIP(b->acc.alloc((size_t)cap * 3 * 8));
  XLB_HIP(b->u.alloc((size_t)cap * 3 * cs));
  XLB_HIP(b->G.alloc((size_t)cap * 3 * cs));
  XLB_HIP(b->dk.alloc((size_t)n * 3 * cs));
  XLB_HIP(b->F.alloc((size_t)n * 3 * cs));
  hipStream_t st = b->ctx->stream;
  XLB_HIP(hipMemsetAsync(b->area.get(), 0, (size_t)n * sizeof(float), st));
  XLB_HIP(hipMemsetAsync(b->vel.get(), 0, (size_t)n * 3 * sizeof(float), st));
  XLB_HIP(hipMemsetAsync(b->G.get(), 0, (size_t)cap * 3 * cs, st));
  XLB_HIP(hipMemsetAsync(b->F.get(), 0, (size_t)n * 3 * cs, st));
  b->n = n;
  b->cap = cap;
  return 0;
}

// cell <-> slot mapping and weight sums of the markers' current positions
static int ibm_build_footprint(xlbhip_ibm* b) {
  hipStream_t st = b->ctx->stream;
  if (int rc = ibm_clear_footprint(b)) return rc;
  XLB_HIP(hipMemsetAsync(b->wbits.get(), 0, (size_t)b->cap * 4, st));
  XLB_HIP(hipMemsetAsync(b->W.get(), 0, (size_t)b->cap * 8, st));
  XLB_HIP(hipMemsetAsync(b->acc.get(), 0, (size_t)b->cap * 3 * 8, st));
  const Dims d{b->nx, b->ny, b->nz};
  return by_compute(b->cdt, [&](auto T) {
    using TT = decltype(T);
    hipLaunchKernelGGL((k_ibm_mark<TT>), blocks_for((size_t)b->n * 64), 256, 0, st, b->pos.get<float>(), b->n, d, b->map.get<int32_t>(),
                       b->list.get<uint32_t>(), b->count.get<int>(), b->cap);
    XLB_HIP(hipGetLastError());
    hipLaunchKernelGGL((k_ibm_wmax<TT>), blocks_for((size_t)b->n * 64), 256, 0, st, b->pos.get<float>(), b->n, d, b->map.get<int32_t>(),
                       b->wbits.get<unsigned>(), b->cap);
    XLB_HIP(hipGetLastError());
    hipLaunchKernelGGL((k_ibm_weights<TT>), blocks_for((size_t)b->n * 64), 256, 0, st, b->pos.get<float>(), b->n, d, b->map.get<int32_t>(),
                       b->wbits.get<unsigned>(), b->W.get<unsigned long long>(), b->cap);
    XLB_HIP(hipGetLastError());
    return 0;
  });
}

// the coupling on f (the field a step has just written)
static int ibm_couple(xlbhip_ibm* b, xlbhip_field* f) {
  hipStream_t st = b->ctx->stream;
  XLB_HIP(hipMemsetAsync(b->ctl.get(), 0, sizeof(IbmControl), st));
  if (b->n == 0 || b->max_sweeps == 0) return 0;
  const Dims d{b->nx, b->ny, b->nz};
  const unsigned slot_blocks = blocks_for((size_t)b->cap), marker_blocks = blocks_for((size_t)b->n), pair_blocks = blocks_for((size_t)b->n * 64);
  const int residual_on = b->tolerance > 0.0 ? 1 : 0;
  IbmControl* ctl = b->ctl.get<IbmControl>();
  const int rc = ibm_dispatch(b, [&](auto L, auto T, auto S) {
    using LL = decltype(L);
    using TT = decltype(T);
    using SS = decltype(S);
    const float* pos = b->pos.get<float>();
    const int32_t* map = b->map.get<int32_t>();
    const int* count = b->count.get<int>();
    unsigned long long* acc = b->acc.get<unsigned long long>();
    TT* u = b->u.get<TT>();
    TT* G = b->G.get<TT>();
    TT* F = b->F.get<TT>();
    TT* dk = b->dk.get<TT>();
    hipLaunchKernelGGL((k_ibm_moments<LL, TT, SS>), slot_blocks, 256, 0, st, static_cast<const SS*>(f->data), f->plane_stride, b->list.get<uint32_t>(), count,
                       b->cap, u);
    XLB_HIP(hipGetLastError());
    hipLaunchKernelGGL((k_ibm_interp<TT>), marker_blocks, 256, 0, st, pos, b->vel.get<float>(), b->n, d, map, b->cap, u, dk, F);
    XLB_HIP(hipGetLastError());
    for (int it = 0; it < b->max_sweeps; ++it) {
      if (it > 0) {  // (the forces are zero in the first sweep: nothing to spread, acc is zero already)
        hipLaunchKernelGGL((k_ibm_spread<TT>), pair_blocks, 256, 0, st, it, residual_on, ctl, pos, b->area.get<float>(), F, b->n, d, map, b->cap,
                           b->wbits.get<unsigned>(), acc);
        XLB_HIP(hipGetLastError());
      }
      hipLaunchKernelGGL((k_ibm_correct<TT>), slot_blocks, 256, 0, st, it, residual_on, ctl, count, b->cap, b->wbits.get<unsigned>(), b->W.get<unsigned long long>(), acc, u,
                         (TT)b->relaxation, G);
      XLB_HIP(hipGetLastError());
      hipLaunchKernelGGL((k_ibm_update<TT>), marker_blocks, 256, 0, st, it, residual_on, ctl, b->n, dk, F, (TT)(b->tolerance * b->tolerance));
      XLB_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL((k_ibm_apply<LL, TT, SS>), slot_blocks, 256, 0, st, static_cast<SS*>(f->data), f->plane_stride, b->list.get<uint32_t>(), count, b->cap,
                       G);
    XLB_HIP(hipGetLastError());
    return 0;
  });
  if (rc) return rc;
  touch(f);
  return 0;
}

// ---- rigid bodies ---------------------------------------------------------------------------------------------------------------
// the staged row [body][18] of timestep t (nullptr: not staged)
static const double* ibm_staged_at(const xlbhip_ibm* b, int64_t t) {
  if (t < b->pose_first || t >= b->pose_first + b->pose_count) return nullptr;
  return b->pose.get<double>() + (size_t)(t - b->pose_first) * b->n_bodies * IBM_POSE_DOUBLES;
}

// the poses [body][18] the move and the loads of timestep t read: the table k_ibm_pose has written for t when there is one, else the
// rest poses while no body moves, else t's staged row
static const double* ibm_pose_at(const xlbhip_ibm* b, int64_t t) {
  if (b->use_live()) return b->live_pose.get<double>();
  if (!b->any_prescribed) return b->rest_pose.get<double>();
  return ibm_staged_at(b, t);
}

// staged rows are demanded only while some prescribed body moves
static int ibm_require_poses(const xlbhip_ibm* b, int64_t t0, int64_t n) {
  XLB_REQUIRE(!b->any_dynamic || b->dynamics_set, "bodies are declared dynamic but their parameters and state were never set (xlbhip_ibm_set_dynamics)");
  if (!b->any_prescribed) return 0;
  for (int64_t k = 0; k < n; ++k)
    XLB_REQUIRE(ibm_staged_at(b, t0 + k), "the poses of the bodies at timestep %lld are not staged (xlbhip_ibm_stage_poses)", (long long)(t0 + k));
  return 0;
}

// the live pose table of timestep t (and the next row of a recorded pose history); staged == nullptr outside a step
static int ibm_live_pose(xlbhip_ibm* b, const double* staged, bool record) {
  double* row = nullptr;
  if (record && b->pose_hist_next < b->pose_hist_rows) row = b->pose_hist.get<double>() + (size_t)b->pose_hist_next++ * b->n_bodies * IBM_POSE_DOUBLES;
  hipLaunchKernelGGL(k_ibm_pose, 1, IBM_MAX_BODIES, 0, b->ctx->stream, b->kind.get<int32_t>(), b->rotate.get<int32_t>(), b->dyn_state.get<double>(),
                     b->dyn_params.get<double>(), staged, b->rest_pose.get<double>(), b->n_bodies, b->live_pose.get<double>(), row);
  XLB_HIP(hipGetLastError());
  return 0;
}

// the dynamic bodies from the state of timestep t to that of t + 1, with the loads the step has just left
static int ibm_integrate(xlbhip_ibm* b) {
  if (!b->any_dynamic) return 0;
  if (b->virtual_on || b->contact_on) {
    hipLaunchKernelGGL(k_ibm_integrate_contact, 1, IBM_MAX_BODIES, 0, b->ctx->stream, b->kind.get<int32_t>(), b->rotate.get<int32_t>(),
                       b->dyn_params.get<double>(), b->loads.get<double>(), b->n_bodies, b->dyn_state.get<double>(), b->status.get<unsigned long long>(),
                       b->virt.get<double>(), b->prev.get<double>(), b->contact_on ? b->radius.get<double>() : nullptr, b->contact_model,
                       b->live_pose.get<double>(), b->contact.get<double>());
    XLB_HIP(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(k_ibm_integrate, 1, IBM_MAX_BODIES, 0, b->ctx->stream, b->kind.get<int32_t>(), b->rotate.get<int32_t>(), b->dyn_params.get<double>(),
                     b->loads.get<double>(), b->n_bodies, b->dyn_state.get<double>(), b->status.get<unsigned long long>());
  XLB_HIP(hipGetLastError());
  return 0;
}

// the markers of the moving bodies to their place at timestep t, then the footprint of the new positions
static int ibm_move(xlbhip_ibm* b, int64_t t) {
  if (!b->any_moving) return 0;
  hipLaunchKernelGGL(k_ibm_move, blocks_for((size_t)b->n), 256, 0, b->ctx->stream, b->pos0.get<float>(), b->move_id.get<int32_t>(), ibm_pose_at(b, t),
                     b->centre0.get<double>(), b->n, b->pos.get<float>(), b->vel.get<float>());
  XLB_HIP(hipGetLastError());
  b->host_pos.clear();  // the device holds other positions than the caller passed last: the next ones are never "the same"
  return ibm_build_footprint(b);
}

// force and torque on every body from the forces the coupling left, to `loads` and to the next row of a recorded history
static int ibm_body_loads(xlbhip_ibm* b, int64_t t) {
  if (b->n_bodies == 0) return 0;
  hipStream_t st = b->ctx->stream;
  const double* pose = ibm_pose_at(b, t);
  double* row = nullptr;
  if (b->hist_next < b->hist_rows) row = b->hist.get<double>() + (size_t)b->hist_next++ * b->n_bodies * 6;
  return by_compute(b->cdt, [&](auto T) {
    using TT = decltype(T);
    if (b->n_chunks > 0) {
      hipLaunchKernelGGL((k_ibm_loads<TT>), (unsigned)b->n_chunks, IBM_LOADS_CHUNK, 0, st, b->chunks.get<IbmLoadChunk>(), b->F.get<TT>(), b->area.get<float>(),
                         b->pos.get<float>(), pose, b->partial.get<double>());
      XLB_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ibm_loads_combine, blocks_for((size_t)b->n_bodies * 6), 256, 0, st, b->chunk0.get<int32_t>(), b->partial.get<double>(), b->n_bodies,
                       b->loads.get<double>(), row);
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
  XLB_HIP(b->map.alloc(b->cells() * sizeof(int32_t)));
  XLB_HIP(b->count.alloc(sizeof(int)));
  XLB_HIP(b->ctl.alloc(sizeof(IbmControl)));
  XLB_HIP(hipMemsetAsync(b->map.get(), 0xff, b->cells() * sizeof(int32_t), c->stream));  // every cell: no slot (-1)
  XLB_HIP(hipMemsetAsync(b->count.get(), 0, sizeof(int), c->stream));
  XLB_HIP(hipMemsetAsync(b->ctl.get(), 0, sizeof(IbmControl), c->stream));
  XLB_HIP(hipEventCreateWithFlags(&b->pin_ev, hipEventDisableTiming));
  XLB_HIP(hipEventRecord(b->pin_ev, c->stream));
  XLB_HIP(hipEventCreateWithFlags(&b->pose_ev, hipEventDisableTiming));
  XLB_HIP(hipEventRecord(b->pose_ev, c->stream));
  *out = b.release();
  return 0;
}

int xlbhip_ibm_destroy(xlbhip_ibm* b) {
  if (!b) return 0;
  (void)hipSetDevice(b->ctx->device);
  (void)hipStreamSynchronize(b->ctx->stream);  // copies may still read the pinned buffer
  if (b->pin_ev) (void)hipEventDestroy(b->pin_ev);
  if (b->pose_ev) (void)hipEventDestroy(b->pose_ev);
  delete b;
  return 0;
}

int xlbhip_ibm_set_markers(xlbhip_ibm* b, int64_t n, const float* positions, const float* areas, const float* velocities) {
  XLB_REQUIRE(b && n >= 0, "bad argument");
  XLB_REQUIRE((size_t)n < ((size_t)1 << 25), "too many markers (%lld)", (long long)n);
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  if (n != b->n) {
    XLB_REQUIRE(b->n_bodies == 0, "the number of markers (%lld -> %lld) cannot change while bodies are declared: clear them first", (long long)b->n, (long long)n);
    XLB_REQUIRE(n == 0 || (positions && areas && velocities), "a new number of markers needs positions, areas and velocities");
    if (int rc = ibm_clear_footprint(b)) return rc;
    XLB_HIP(hipStreamSynchronize(c->stream));
    if (int rc = ibm_resize(b, n)) return rc;
  }
  if (n == 0) return 0;
  XLB_HIP(hipEventSynchronize(b->pin_ev));  // the previous copy out of the pinned buffer (not the kernels)
  float* pin = b->pin.get<float>();
  const size_t n3 = (size_t)n * 3 * sizeof(float);
  bool moved = false;
  if (positions) {
    // (k_ibm_move empties host_pos: after the device has moved the markers, no array the caller passes counts as "the same")
    moved = b->host_pos.size() != (size_t)n * 3 || std::memcmp(b->host_pos.data(), positions, n3) != 0;
    if (moved) {
      b->host_pos.assign(positions, positions + (size_t)n * 3);
      std::memcpy(pin, positions, n3);
      XLB_HIP(hipMemcpyAsync(b->pos.get(), pin, n3, hipMemcpyHostToDevice, c->stream));
      // they are the new reference positions of the bodies
      if (b->any_moving) XLB_HIP(hipMemcpyAsync(b->pos0.get(), pin, n3, hipMemcpyHostToDevice, c->stream));
      b->pos0_valid = b->any_moving;
    }
  }
  if (areas) {
    std::memcpy(pin + 3 * n, areas, (size_t)n * sizeof(float));
    XLB_HIP(hipMemcpyAsync(b->area.get(), pin + 3 * n, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  }
  if (velocities) {
    std::memcpy(pin + 4 * n, velocities, n3);
    XLB_HIP(hipMemcpyAsync(b->vel.get(), pin + 4 * n, n3, hipMemcpyHostToDevice, c->stream));
  }
  XLB_HIP(hipEventRecord(b->pin_ev, c->stream));
  if (moved) return ibm_build_footprint(b);
  return 0;
}

int xlbhip_ibm_step(xlbhip_ibm* b, const xlbhip_field* f_src, xlbhip_field* f_dst, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask,
                    double omega, int64_t timestep) {
  XLB_REQUIRE(b, "null argument");
  if (int rc = ibm_check_field(b, f_src)) return rc;
  if (int rc = ibm_check_field(b, f_dst)) return rc;
  if (int rc = ibm_require_poses(b, timestep, 1)) return rc;
  if (b->use_live())
    if (int rc = ibm_live_pose(b, b->any_prescribed ? ibm_staged_at(b, timestep) : nullptr, true)) return rc;
  if (int rc = ibm_move(b, timestep)) return rc;
  if (int rc = xlbhip_step(b->stepper, f_src, f_dst, bc_mask, missing_mask, omega, timestep)) return rc;
  if (int rc = ibm_couple(b, f_dst)) return rc;
  if (int rc = ibm_body_loads(b, timestep)) return rc;
  return ibm_integrate(b);
}

int xlbhip_ibm_run(xlbhip_ibm* b, xlbhip_field* f_a, xlbhip_field* f_b, const xlbhip_field* bc_mask, const xlbhip_field* missing_mask, double omega,
                   int64_t first_timestep, int64_t n_steps, int* result_in_b) {
  XLB_REQUIRE(b && result_in_b && n_steps >= 0, "bad argument");
  if (int rc = ibm_require_poses(b, first_timestep, n_steps)) return rc;  // (before anything is enqueued)
  xlbhip_field* cur = f_a;
  xlbhip_field* oth = f_b;
  for (int64_t i = 0; i < n_steps; ++i) {
    if (int rc = xlbhip_ibm_step(b, cur, oth, bc_mask, missing_mask, omega, first_timestep + i)) return rc;
    std::swap(cur, oth);
  }
  *result_in_b = cur == f_b ? 1 : 0;
  return 0;
}

int xlbhip_ibm_forces(xlbhip_ibm* b, int64_t n, double* forces) {
  XLB_REQUIRE(b && n == b->n && (n == 0 || forces), "xlbhip_ibm_forces: expected room for %lld markers", b ? (long long)b->n : 0LL);
  if (n == 0) return 0;
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  std::vector<char> host((size_t)n * 3 * b->csize());
  XLB_HIP(hipMemcpyAsync(host.data(), b->F.get(), host.size(), hipMemcpyDeviceToHost, c->stream));
  XLB_HIP(hipStreamSynchronize(c->stream));
  by_compute(b->cdt, [&](auto T) {
    const auto* v = reinterpret_cast<const decltype(T)*>(host.data());
    for (size_t i = 0; i < (size_t)n * 3; ++i) forces[i] = (double)v[i];
    return 0;
  });
  return 0;
}

int xlbhip_ibm_iterations(xlbhip_ibm* b, int* sweeps) {
  XLB_REQUIRE(b && sweeps, "null argument");
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  XLB_HIP(hipMemcpyAsync(sweeps, b->ctl.get<char>() + offsetof(IbmControl, sweeps), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  XLB_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int xlbhip_ibm_footprint(xlbhip_ibm* b, int64_t* n_cells, int64_t capacity, uint32_t* cells) {
  XLB_REQUIRE(b && n_cells, "null argument");
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  int count = 0;
  XLB_HIP(hipMemcpyAsync(&count, b->count.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  XLB_HIP(hipStreamSynchronize(c->stream));
  *n_cells = count;
  if (cells && count > 0) {
    XLB_REQUIRE(capacity >= count, "xlbhip_ibm_footprint: room for %lld cells, the footprint has %d", (long long)capacity, count);
    XLB_HIP(hipMemcpy(cells, b->list.get(), (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  return 0;
}

int xlbhip_ibm_set_bodies(xlbhip_ibm* b, int n_bodies, const int64_t* first, const int64_t* count, const int* moving, const double* centre0) {
  XLB_REQUIRE(b && n_bodies >= 0, "bad argument");
  XLB_REQUIRE(n_bodies <= IBM_MAX_BODIES, "%d bodies, at most %d are supported", n_bodies, IBM_MAX_BODIES);
  XLB_REQUIRE(n_bodies == 0 || (first && count && moving && centre0), "null argument");
  for (int i = 0; i < n_bodies; ++i) {
    XLB_REQUIRE(first[i] >= 0 && count[i] >= 0 && first[i] + count[i] <= b->n, "body %d: markers %lld .. %lld are out of bounds (%lld markers)", i,
                (long long)first[i], (long long)(first[i] + count[i]), (long long)b->n);
    for (int j = 0; j < i; ++j)
      XLB_REQUIRE(first[i] >= first[j] + count[j] || first[j] >= first[i] + count[i], "bodies %d and %d overlap", j, i);
  }
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  XLB_HIP(hipStreamSynchronize(c->stream));  // queued steps read the tables replaced below
  b->n_bodies = 0;
  b->any_moving = false;
  b->n_chunks = b->pose_count = 0;
  b->hist_rows = b->hist_next = 0;
  b->pose_hist_rows = b->pose_hist_next = 0;
  b->any_prescribed = b->any_dynamic = b->dynamics_set = false;
  b->virtual_on = b->contact_on = false;
  if (n_bodies == 0) return 0;
  for (int i = 0; i < n_bodies; ++i)
    XLB_REQUIRE(moving[i] >= IBM_BODY_REST && moving[i] <= IBM_BODY_DYNAMIC, "body %d: bad moving flag %d (0 at rest, 1 prescribed, 2 dynamic)", i, moving[i]);
  std::vector<int32_t> kind(moving, moving + n_bodies), rotate((size_t)n_bodies, IBM_ROTATE_LOCKED);
  std::vector<int32_t> move_id((size_t)b->n, -1), chunk0((size_t)n_bodies + 1, 0);
  std::vector<IbmLoadChunk> chunks;
  std::vector<double> rest((size_t)n_bodies * IBM_POSE_DOUBLES, 0.0);
  bool any_moving = false, any_prescribed = false, any_dynamic = false;
  for (int i = 0; i < n_bodies; ++i) {
    if (moving[i]) {
      any_moving = any_moving || count[i] > 0;
      any_prescribed = any_prescribed || (moving[i] == IBM_BODY_PRESCRIBED && count[i] > 0);
      any_dynamic = any_dynamic || moving[i] == IBM_BODY_DYNAMIC;
      std::fill(move_id.begin() + first[i], move_id.begin() + first[i] + count[i], (int32_t)i);
    }
    chunk0[i] = (int32_t)chunks.size();
    for (int64_t o = 0; o < count[i]; o += IBM_LOADS_CHUNK)
      chunks.push_back(IbmLoadChunk{(int32_t)i, (int32_t)(first[i] + o), (int32_t)std::min<int64_t>(IBM_LOADS_CHUNK, count[i] - o)});
    double* P = rest.data() + (size_t)i * IBM_POSE_DOUBLES;
    P[0] = P[4] = P[8] = 1.0;
    for (int a = 0; a < 3; ++a) P[9 + a] = centre0[3 * i + a];
  }
  chunk0[n_bodies] = (int32_t)chunks.size();
  if (int rc = upload_bytes(move_id.data(), move_id.size() * sizeof(int32_t), b->move_id)) return rc;
  if (int rc = upload_bytes(chunk0.data(), chunk0.size() * sizeof(int32_t), b->chunk0)) return rc;
  if (int rc = upload_bytes(chunks.data(), chunks.size() * sizeof(IbmLoadChunk), b->chunks)) return rc;
  if (int rc = upload_bytes(centre0, (size_t)n_bodies * 3 * sizeof(double), b->centre0)) return rc;
  if (int rc = upload_bytes(rest.data(), rest.size() * sizeof(double), b->rest_pose)) return rc;
  if (int rc = upload_bytes(kind.data(), kind.size() * sizeof(int32_t), b->kind)) return rc;
  if (int rc = upload_bytes(rotate.data(), rotate.size() * sizeof(int32_t), b->rotate)) return rc;
  XLB_HIP(b->live_pose.alloc((size_t)n_bodies * IBM_POSE_DOUBLES * sizeof(double)));
  XLB_HIP(b->dyn_state.alloc((size_t)n_bodies * IBM_DYN_STATE_DOUBLES * sizeof(double)));
  XLB_HIP(b->dyn_params.alloc((size_t)n_bodies * IBM_DYN_PARAM_DOUBLES * sizeof(double)));
  if (!b->status) XLB_HIP(b->status.alloc(sizeof(unsigned long long)));
  XLB_HIP(hipMemsetAsync(b->dyn_state.get(), 0, (size_t)n_bodies * IBM_DYN_STATE_DOUBLES * sizeof(double), c->stream));
  XLB_HIP(hipMemsetAsync(b->dyn_params.get(), 0, (size_t)n_bodies * IBM_DYN_PARAM_DOUBLES * sizeof(double), c->stream));
  XLB_HIP(hipMemsetAsync(b->status.get(), 0, sizeof(unsigned long long), c->stream));
  XLB_HIP(b->virt.alloc((size_t)n_bodies * 2 * sizeof(double)));
  XLB_HIP(b->prev.alloc((size_t)n_bodies * 6 * sizeof(double)));
  XLB_HIP(b->radius.alloc((size_t)n_bodies * sizeof(double)));
  XLB_HIP(b->contact.alloc((size_t)n_bodies * 3 * sizeof(double)));
  XLB_HIP(hipMemsetAsync(b->virt.get(), 0, (size_t)n_bodies * 2 * sizeof(double), c->stream));
  XLB_HIP(hipMemsetAsync(b->prev.get(), 0, (size_t)n_bodies * 6 * sizeof(double), c->stream));
  XLB_HIP(hipMemsetAsync(b->radius.get(), 0, (size_t)n_bodies * sizeof(double), c->stream));
  XLB_HIP(hipMemsetAsync(b->contact.get(), 0, (size_t)n_bodies * 3 * sizeof(double), c->stream));
  XLB_HIP(b->partial.alloc(std::max<size_t>(chunks.size(), 1) * 6 * sizeof(double)));
  XLB_HIP(b->loads.alloc((size_t)n_bodies * 6 * sizeof(double)));
  XLB_HIP(hipMemsetAsync(b->loads.get(), 0, (size_t)n_bodies * 6 * sizeof(double), c->stream));
  if (any_prescribed) {
    if (!b->pose) XLB_HIP(b->pose.alloc(XLBHIP_IBM_POSE_BYTES));
    if (!b->pose_pin) XLB_HIP(b->pose_pin.alloc(XLBHIP_IBM_POSE_BYTES));
  }
  if (any_moving) {
    if (!b->pos0_valid) {  // nothing has moved the markers since they were uploaded: `pos` holds the reference positions
      XLB_HIP(b->pos0.alloc((size_t)b->n * 3 * sizeof(float)));
      XLB_HIP(hipMemcpyAsync(b->pos0.get(), b->pos.get(), (size_t)b->n * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
      b->pos0_valid = true;
    }
  }
  b->n_bodies = n_bodies;
  b->any_moving = any_moving;
  b->any_prescribed = any_prescribed;
  b->any_dynamic = any_dynamic;
  b->n_chunks = (int64_t)chunks.size();
  return 0;
}

int xlbhip_ibm_set_dynamics(xlbhip_ibm* b, int n_bodies, const int* rotate, const double* params, const double* state) {
  XLB_REQUIRE(b && rotate && params && state, "null argument");
  XLB_REQUIRE(n_bodies == b->n_bodies && n_bodies > 0, "xlbhip_ibm_set_dynamics: %d bodies, %d are declared (xlbhip_ibm_set_bodies)", n_bodies, b->n_bodies);
  XLB_REQUIRE(b->any_dynamic, "xlbhip_ibm_set_dynamics: no body is declared dynamic (moving flag 2 of xlbhip_ibm_set_bodies)");
  std::vector<int32_t> modes(rotate, rotate + n_bodies);
  for (int i = 0; i < n_bodies; ++i)
    XLB_REQUIRE(modes[i] >= IBM_ROTATE_LOCKED && modes[i] <= IBM_ROTATE_FREE, "body %d: bad rotation mode %d (0 locked, 1 axis, 2 free)", i, modes[i]);
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  XLB_HIP(hipStreamSynchronize(c->stream));  // queued steps read the tables replaced below
  if (int rc = upload_bytes(modes.data(), modes.size() * sizeof(int32_t), b->rotate)) return rc;
  if (int rc = upload_bytes(params, (size_t)n_bodies * IBM_DYN_PARAM_DOUBLES * sizeof(double), b->dyn_params)) return rc;
  if (int rc = upload_bytes(state, (size_t)n_bodies * IBM_DYN_STATE_DOUBLES * sizeof(double), b->dyn_state)) return rc;
  XLB_HIP(hipMemsetAsync(b->status.get(), 0, sizeof(unsigned long long), c->stream));
  XLB_HIP(hipMemsetAsync(b->virt.get(), 0, (size_t)n_bodies * 2 * sizeof(double), c->stream));
  XLB_HIP(hipMemsetAsync(b->prev.get(), 0, (size_t)n_bodies * 6 * sizeof(double), c->stream));
  XLB_HIP(hipMemsetAsync(b->radius.get(), 0, (size_t)n_bodies * sizeof(double), c->stream));
  XLB_HIP(hipMemsetAsync(b->contact.get(), 0, (size_t)n_bodies * 3 * sizeof(double), c->stream));
  b->virtual_on = b->contact_on = false;
  b->dynamics_set = true;
  return 0;
}

int xlbhip_ibm_set_virtual_mass(xlbhip_ibm* b, int n_bodies, const double* virtual_mass, const double* virtual_inertia) {
  XLB_REQUIRE(b && virtual_mass && virtual_inertia, "null argument");
  XLB_REQUIRE(n_bodies == b->n_bodies && n_bodies > 0, "xlbhip_ibm_set_virtual_mass: %d bodies, %d are declared (xlbhip_ibm_set_bodies)", n_bodies, b->n_bodies);
  XLB_REQUIRE(b->dynamics_set, "xlbhip_ibm_set_virtual_mass: call xlbhip_ibm_set_dynamics first");
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
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  XLB_HIP(hipStreamSynchronize(c->stream));  // queued steps read the tables replaced below
  if (int rc = upload_bytes(virt.data(), virt.size() * sizeof(double), b->virt)) return rc;
  XLB_HIP(hipMemsetAsync(b->prev.get(), 0, (size_t)n_bodies * 6 * sizeof(double), c->stream));
  b->virtual_on = any;
  return 0;
}

int xlbhip_ibm_set_contact(xlbhip_ibm* b, int n_bodies, const double* radius, double range, double stiffness, double wall_stiffness, const double* lo,
                           const double* hi) {
  XLB_REQUIRE(b && radius, "null argument");
  XLB_REQUIRE(n_bodies == b->n_bodies && n_bodies > 0, "xlbhip_ibm_set_contact: %d bodies, %d are declared (xlbhip_ibm_set_bodies)", n_bodies, b->n_bodies);
  XLB_REQUIRE(b->dynamics_set, "xlbhip_ibm_set_contact: call xlbhip_ibm_set_dynamics first");
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
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  XLB_HIP(hipStreamSynchronize(c->stream));  // queued steps read the tables replaced below
  if (int rc = upload_bytes(radius, (size_t)n_bodies * sizeof(double), b->radius)) return rc;
  XLB_HIP(hipMemsetAsync(b->contact.get(), 0, (size_t)n_bodies * 3 * sizeof(double), c->stream));
  b->contact_model = model;
  b->contact_on = any && b->any_dynamic;
  return 0;
}

int xlbhip_ibm_contact_forces(xlbhip_ibm* b, int n_bodies, double* forces) {
  XLB_REQUIRE(b && n_bodies == b->n_bodies && (n_bodies == 0 || forces), "xlbhip_ibm_contact_forces: expected room for %d bodies", b ? b->n_bodies : 0);
  if (n_bodies == 0) return 0;
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  XLB_HIP(hipMemcpyAsync(forces, b->contact.get(), (size_t)n_bodies * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  XLB_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int xlbhip_ibm_body_poses(xlbhip_ibm* b, int n_bodies, double* poses, uint64_t* status) {
  XLB_REQUIRE(b && n_bodies == b->n_bodies && status && (n_bodies == 0 || poses), "xlbhip_ibm_body_poses: expected room for %d bodies", b ? b->n_bodies : 0);
  *status = 0;
  if (n_bodies == 0) return 0;
  XLB_REQUIRE(!b->any_dynamic || b->dynamics_set, "bodies are declared dynamic but their parameters and state were never set (xlbhip_ibm_set_dynamics)");
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  if (int rc = ibm_live_pose(b, nullptr, false)) return rc;
  XLB_HIP(hipMemcpyAsync(poses, b->live_pose.get(), (size_t)n_bodies * IBM_POSE_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  XLB_HIP(hipMemcpyAsync(status, b->status.get(), sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  XLB_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int xlbhip_ibm_record_poses(xlbhip_ibm* b, int64_t n_rows) {
  XLB_REQUIRE(b && n_rows >= 0, "bad argument");
  XLB_REQUIRE(n_rows == 0 || b->n_bodies > 0, "xlbhip_ibm_record_poses: no bodies are declared");
  XLB_HIP(hipSetDevice(b->ctx->device));
  b->pose_hist_rows = b->pose_hist_next = 0;
  if (n_rows == 0) return 0;
  XLB_HIP(b->pose_hist.alloc((size_t)n_rows * b->n_bodies * IBM_POSE_DOUBLES * sizeof(double)));
  b->pose_hist_rows = n_rows;
  return 0;
}

int xlbhip_ibm_poses_history(xlbhip_ibm* b, int64_t n_rows, double* poses) {
  XLB_REQUIRE(b && n_rows >= 0 && (n_rows == 0 || poses), "bad argument");
  XLB_REQUIRE(n_rows <= b->pose_hist_next, "xlbhip_ibm_poses_history: %lld rows asked for, %lld were recorded", (long long)n_rows, (long long)b->pose_hist_next);
  if (n_rows == 0) return 0;
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  XLB_HIP(hipMemcpyAsync(poses, b->pose_hist.get(), (size_t)n_rows * b->n_bodies * IBM_POSE_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  XLB_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int xlbhip_ibm_stage_poses(xlbhip_ibm* b, int64_t first_timestep, int64_t n_steps, const double* poses) {
  XLB_REQUIRE(b && n_steps >= 0 && (n_steps == 0 || poses), "bad argument");
  XLB_REQUIRE(b->any_prescribed, "xlbhip_ibm_stage_poses: no body with prescribed motion moves (xlbhip_ibm_set_bodies)");
  const size_t bytes = (size_t)n_steps * b->n_bodies * IBM_POSE_DOUBLES * sizeof(double);
  XLB_REQUIRE(bytes <= XLBHIP_IBM_POSE_BYTES, "%lld steps x %d bodies of poses are %zu bytes, at most %d are staged at once", (long long)n_steps, b->n_bodies,
              bytes, XLBHIP_IBM_POSE_BYTES);
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  b->pose_count = 0;
  if (n_steps == 0) return 0;
  XLB_HIP(hipEventSynchronize(b->pose_ev));  // the previous copy out of the pinned buffer (not the kernels)
  std::memcpy(b->pose_pin.get(), poses, bytes);
  // (in stream order behind the steps that read the rows staged before)
  XLB_HIP(hipMemcpyAsync(b->pose.get(), b->pose_pin.get(), bytes, hipMemcpyHostToDevice, c->stream));
  XLB_HIP(hipEventRecord(b->pose_ev, c->stream));
  b->pose_first = first_timestep;
  b->pose_count = n_steps;
  return 0;
}

int xlbhip_ibm_loads(xlbhip_ibm* b, int n_bodies, double* loads) {
  XLB_REQUIRE(b && n_bodies == b->n_bodies && (n_bodies == 0 || loads), "xlbhip_ibm_loads: expected room for %d bodies", b ? b->n_bodies : 0);
  if (n_bodies == 0) return 0;
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  XLB_HIP(hipMemcpyAsync(loads, b->loads.get(), (size_t)n_bodies * 6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  XLB_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int xlbhip_ibm_record_loads(xlbhip_ibm* b, int64_t n_rows) {
  XLB_REQUIRE(b && n_rows >= 0, "bad argument");
  XLB_REQUIRE(n_rows == 0 || b->n_bodies > 0, "xlbhip_ibm_record_loads: no bodies are declared");
  XLB_HIP(hipSetDevice(b->ctx->device));
  b->hist_rows = b->hist_next = 0;
  if (n_rows == 0) return 0;
  XLB_HIP(b->hist.alloc((size_t)n_rows * b->n_bodies * 6 * sizeof(double)));
  b->hist_rows = n_rows;
  return 0;
}

int xlbhip_ibm_loads_history(xlbhip_ibm* b, int64_t n_rows, double* loads) {
  XLB_REQUIRE(b && n_rows >= 0 && (n_rows == 0 || loads), "bad argument");
  XLB_REQUIRE(n_rows <= b->hist_next, "xlbhip_ibm_loads_history: %lld rows asked for, %lld were recorded", (long long)n_rows, (long long)b->hist_next);
  if (n_rows == 0) return 0;
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  XLB_HIP(hipMemcpyAsync(loads, b->hist.get(), (size_t)n_rows * b->n_bodies * 6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  XLB_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int xlbhip_ibm_download_markers(xlbhip_ibm* b, int64_t n, float* positions, float* velocities) {
  XLB_REQUIRE(b && n == b->n, "xlbhip_ibm_download_markers: expected room for %lld markers", b ? (long long)b->n : 0LL);
  if (n == 0) return 0;
  xlbhip_ctx* c = b->ctx;
  XLB_HIP(hipSetDevice(c->device));
  const size_t n3 = (size_t)n * 3 * sizeof(float);
  if (positions) XLB_HIP(hipMemcpyAsync(positions, b->pos.get(), n3, hipMemcpyDeviceToHost, c->stream));
  if (velocities) XLB_HIP(hipMemcpyAsync(velocities, b->vel.get(), n3, hipMemcpyDeviceToHost, c->stream));
  XLB_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
