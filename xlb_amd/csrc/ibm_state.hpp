// The owners of the immersed-boundary stepper's memory (ibm.hip): the markers, their footprint, the rigid bodies with their staged
// poses and recordings.  What the host decides about bodies is ibm_bodies.hpp's; the launches and the C entries are ibm.hip's.
#pragma once
#include <initializer_list>
#include <vector>

#include "api_internal.hpp"
#include "ibm_bodies.hpp"

namespace xlb {

static int alloc_zeroed(DeviceBuf& buf, size_t bytes, hipStream_t st) {
  XLB_HIP(buf.alloc(bytes));
  XLB_HIP(hipMemsetAsync(buf.get(), 0, bytes, st));
  return 0;
}

// blocking read-back of device arrays (a null host pointer: that one is not wanted): in stream order behind everything enqueued
struct ReadBack {
  void* host;
  const void* dev;
  size_t bytes;
};
static int read_back(xlbhip_ctx* c, std::initializer_list<ReadBack> copies) {
  XLB_HIP(hipSetDevice(c->device));
  for (const ReadBack& r : copies)
    if (r.host) XLB_HIP(hipMemcpyAsync(r.host, r.dev, r.bytes, hipMemcpyDeviceToHost, c->stream));
  XLB_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

// A pinned host buffer that uploads are staged through, and the event of the last copy out of it
struct PinnedStage {
  PinnedBuf buf;
  hipEvent_t ev = nullptr;
  ~PinnedStage() {
    if (ev) (void)hipEventDestroy(ev);
  }
  int create(hipStream_t st) {  // (starts out "copied")
    XLB_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return record(st);
  }
  // the previous copy out of the buffer (not the kernels): after this the host may overwrite it
  int wait() {
    XLB_HIP(hipEventSynchronize(ev));
    return 0;
  }
  int record(hipStream_t st) {
    XLB_HIP(hipEventRecord(ev, st));
    return 0;
  }
};

// Rows of WIDTH doubles per body that the steps of a run write on the device, one row per step, read once after the run
template <int WIDTH>
struct Recording {
  DeviceBuf buf;  // double [rows][n_bodies][WIDTH], row `next` is the next step's
  int64_t rows = 0, next = 0;
  size_t row_doubles = 0;
  void off() { rows = next = 0; }
  // n_rows == 0 switches the recording off
  int arm(int64_t n_rows, int n_bodies) {
    off();
    if (n_rows == 0) return 0;
    row_doubles = (size_t)n_bodies * WIDTH;
    XLB_HIP(buf.alloc((size_t)n_rows * row_doubles * sizeof(double)));
    rows = n_rows;
    return 0;
  }
  double* next_row() { return next < rows ? buf.get<double>() + (size_t)next++ * row_doubles : nullptr; }
  int read(xlbhip_ctx* c, int64_t n_rows, double* out) const { return read_back(c, {{out, buf.get(), (size_t)n_rows * row_doubles * sizeof(double)}}); }
};

// The markers: float32 as the caller passes them; staged through ONE pinned buffer [positions 3n | areas n | velocities 3n]
struct IbmMarkers {
  int64_t n = 0;
  DeviceBuf pos, area, vel;
  PinnedStage stage;
  std::vector<float> host_pos;  // what the footprint was built from
  size_t bytes3() const { return (size_t)n * 3 * sizeof(float); }
};

// The footprint of the markers and the per-slot / per-marker scratch of the coupling
struct IbmFootprint {
  int64_t cap = 0;  // slots the arrays hold: min(64 n, cells)
  DeviceBuf map;    // int32 per grid cell: slot, or -1
  DeviceBuf list;   // uint32 [cap]: slot -> cell
  DeviceBuf count;  // int: slots in use
  DeviceBuf wbits;  // uint32 [cap]: fp32 bit pattern of the slot's largest weight (sets the slot's fixed-point quantum)
  DeviceBuf W;      // fixed point [cap]
  DeviceBuf acc;    // fixed point [cap][3]; zero between uses
  DeviceBuf u, G;   // compute dtype [cap][3]
  DeviceBuf dk, F;  // per marker, compute dtype [n][3]
  DeviceBuf ctl;    // IbmControl
};

// The rigid bodies (xlbhip_ibm_set_bodies): disjoint ranges of the markers; the ones that move are placed by k_ibm_move before every step
struct IbmBodies {
  int n = 0;
  IbmStepPlan plan;
  // the tables of ibm_body_tables
  DeviceBuf move_id, chunks, chunk0, kind, rest_pose;
  DeviceBuf centre0;  // double [n][3]
  int64_t n_chunks = 0;
  DeviceBuf pos0;           // float [markers][3]: the reference positions X0 the poses are applied to
  bool pos0_valid = false;  // false: the markers' `pos` still holds them (nothing has moved the markers since they were uploaded)
  // poses of the staged timesteps pose_first .. pose_first + pose_count - 1, [step][body][18]
  DeviceBuf pose;
  PinnedStage pose_stage;
  int64_t pose_first = 0, pose_count = 0;
  DeviceBuf partial;  // double [n_chunks][6]
  DeviceBuf loads;    // double [n][6]
  // free bodies (xlbhip_ibm_set_dynamics): integrated on the device from the loads of every step (ibm_dynamics_kernels.hpp)
  DeviceBuf rotate;      // int32 [n]: IBM_ROTATE_*
  DeviceBuf dyn_state;   // double [n][16]
  DeviceBuf dyn_params;  // double [n][32]
  DeviceBuf status;      // uint64: bit b set = body b met a state that was not finite (sticky)
  DeviceBuf live_pose;   // double [n][18]: what k_ibm_pose wrote for the step under way
  // virtual mass and contact (xlbhip_ibm_set_virtual_mass / _set_contact)
  DeviceBuf virt;     // double [n][2]: m_v, I_v
  DeviceBuf prev;     // double [n][6]: a_prev | alpha_prev
  DeviceBuf radius;   // double [n]: contact radius, 0 = takes no part
  DeviceBuf contact;  // double [n][3]: the contact force of the last step
  IbmContactModel contact_model{};
  Recording<6> loads_hist;
  Recording<IBM_POSE_DOUBLES> pose_hist;

  size_t doubles(int per_body) const { return (size_t)n * per_body * sizeof(double); }

  // the staged row [body][18] of timestep t (nullptr: not staged)
  const double* staged_at(int64_t t) const {
    if (t < pose_first || t >= pose_first + pose_count) return nullptr;
    return pose.get<double>() + (size_t)(t - pose_first) * n * IBM_POSE_DOUBLES;
  }
  // the poses [body][18] the move and the loads of timestep t read
  const double* pose_at(int64_t t) const {
    const IbmPoseSource from = plan.pose_source();
    return from == IbmPoseSource::LIVE ? live_pose.get<double>() : from == IbmPoseSource::REST ? rest_pose.get<double>() : staged_at(t);
  }
  int require_dynamics() const {
    XLB_REQUIRE(!plan.dynamics_missing(), "bodies are declared dynamic but their parameters and state were never set (xlbhip_ibm_set_dynamics)");
    return 0;
  }
  int require_poses(int64_t t0, int64_t count) const {
    if (int rc = require_dynamics()) return rc;
    if (!plan.needs_staged()) return 0;
    for (int64_t k = 0; k < count; ++k)
      XLB_REQUIRE(staged_at(t0 + k), "the poses of the bodies at timestep %lld are not staged (xlbhip_ibm_stage_poses)", (long long)(t0 + k));
    return 0;
  }

  // no bodies (the stream has been drained: queued steps read the tables)
  void forget() {
    n = 0;
    plan = IbmStepPlan{};
    n_chunks = pose_count = 0;
    loads_hist.off();
    pose_hist.off();
  }
  // a new declaration and new dynamics start without virtual mass, without contact and with a clean status word
  int reset_extras(int n_bodies, hipStream_t st) {
    XLB_HIP(hipMemsetAsync(status.get(), 0, sizeof(unsigned long long), st));
    XLB_HIP(hipMemsetAsync(virt.get(), 0, (size_t)n_bodies * 2 * sizeof(double), st));
    XLB_HIP(hipMemsetAsync(prev.get(), 0, (size_t)n_bodies * 6 * sizeof(double), st));
    XLB_HIP(hipMemsetAsync(radius.get(), 0, (size_t)n_bodies * sizeof(double), st));
    XLB_HIP(hipMemsetAsync(contact.get(), 0, (size_t)n_bodies * 3 * sizeof(double), st));
    plan.virtual_on = plan.contact_on = false;
    return 0;
  }
  // uploads the tables of n_bodies > 0 bodies after forget(); markers: the ones the ranges refer to
  int declare(hipStream_t st, const IbmBodyTables& t, int n_bodies, const double* centres, const IbmMarkers& markers) {
    const size_t body = (size_t)n_bodies * sizeof(double);
    if (int rc = upload_bytes(t.move_id.data(), t.move_id.size() * sizeof(int32_t), move_id)) return rc;
    if (int rc = upload_bytes(t.chunk0.data(), t.chunk0.size() * sizeof(int32_t), chunk0)) return rc;
    if (int rc = upload_bytes(t.chunks.data(), t.chunks.size() * sizeof(IbmLoadChunk), chunks)) return rc;
    if (int rc = upload_bytes(centres, 3 * body, centre0)) return rc;
    if (int rc = upload_bytes(t.rest.data(), t.rest.size() * sizeof(double), rest_pose)) return rc;
    if (int rc = upload_bytes(t.kind.data(), t.kind.size() * sizeof(int32_t), kind)) return rc;
    const std::vector<int32_t> locked((size_t)n_bodies, IBM_ROTATE_LOCKED);
    if (int rc = upload_bytes(locked.data(), locked.size() * sizeof(int32_t), rotate)) return rc;
    XLB_HIP(live_pose.alloc(IBM_POSE_DOUBLES * body));
    if (int rc = alloc_zeroed(dyn_state, IBM_DYN_STATE_DOUBLES * body, st)) return rc;
    if (int rc = alloc_zeroed(dyn_params, IBM_DYN_PARAM_DOUBLES * body, st)) return rc;
    if (!status) XLB_HIP(status.alloc(sizeof(unsigned long long)));
    XLB_HIP(virt.alloc(2 * body));
    XLB_HIP(prev.alloc(6 * body));
    XLB_HIP(radius.alloc(body));
    XLB_HIP(contact.alloc(3 * body));
    if (int rc = reset_extras(n_bodies, st)) return rc;
    XLB_HIP(partial.alloc(std::max<size_t>(t.chunks.size(), 1) * 6 * sizeof(double)));
    if (int rc = alloc_zeroed(loads, 6 * body, st)) return rc;
    if (t.any_prescribed) {
      if (!pose) XLB_HIP(pose.alloc(XLBHIP_IBM_POSE_BYTES));
      if (!pose_stage.buf) XLB_HIP(pose_stage.buf.alloc(XLBHIP_IBM_POSE_BYTES));
    }
    if (t.any_moving && !pos0_valid) {  // nothing has moved the markers since they were uploaded: `pos` holds the reference positions
      XLB_HIP(pos0.alloc(markers.bytes3()));
      XLB_HIP(hipMemcpyAsync(pos0.get(), markers.pos.get(), markers.bytes3(), hipMemcpyDeviceToDevice, st));
      pos0_valid = true;
    }
    n = n_bodies;
    plan.any_moving = t.any_moving;
    plan.any_prescribed = t.any_prescribed;
    plan.any_dynamic = t.any_dynamic;
    n_chunks = (int64_t)t.chunks.size();
    return 0;
  }
};

}  // namespace xlb
