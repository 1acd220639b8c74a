// What the host decides about the rigid bodies of the immersed-boundary stepper: the constants and plain structs the kernels and
// ibm.hip share, the tables xlbhip_ibm_set_bodies uploads, and the plan that says which launches a step makes.  Host arithmetic
// only — no HIP type or call, so that tests/test_ibm_bodies.py and tests/ibm_motion_cpu_emulation.cpp compile it for the CPU; the
// device buffers, the copies and the launches are ibm.hip's.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace xlb {

constexpr int IBM_MAX_BODIES = 64;
constexpr int IBM_POSE_DOUBLES = 18;  // R[9] | c[3] | w[3] | v[3]
constexpr int IBM_LOADS_CHUNK = 256;  // markers per partial sum = threads per block of k_ibm_loads
constexpr int IBM_DYN_STATE_DOUBLES = 16;
constexpr int IBM_DYN_PARAM_DOUBLES = 32;
enum : int32_t { IBM_BODY_REST = 0, IBM_BODY_PRESCRIBED = 1, IBM_BODY_DYNAMIC = 2 };  // the `moving` flags of xlbhip_ibm_set_bodies
enum : int32_t { IBM_ROTATE_LOCKED = 0, IBM_ROTATE_AXIS = 1, IBM_ROTATE_FREE = 2 };

// one block of k_ibm_loads: `count` (1 .. 256) markers from `first`, all of body `body`
struct IbmLoadChunk {
  int32_t body, first, count;
};

struct IbmContactModel {
  double range, stiffness, wall_stiffness, lo[3], hi[3];
};

inline std::string ibm_message(const char* fmt, ...) {
  char text[256];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(text, sizeof text, fmt, ap);
  va_end(ap);
  return text;
}

// What is wrong with a declaration of bodies over n_markers markers (empty: nothing), checked in this order: too many bodies, a
// missing array, then body after body its range and its overlap with the bodies before it.
inline std::string ibm_check_bodies(int64_t n_markers, int n_bodies, const int64_t* first, const int64_t* count, const int* moving, const double* centre0) {
  if (n_bodies > IBM_MAX_BODIES) return ibm_message("%d bodies, at most %d are supported", n_bodies, IBM_MAX_BODIES);
  if (n_bodies > 0 && !(first && count && moving && centre0)) return "null argument";
  for (int i = 0; i < n_bodies; ++i) {
    if (!(first[i] >= 0 && count[i] >= 0 && first[i] + count[i] <= n_markers))
      return ibm_message("body %d: markers %lld .. %lld are out of bounds (%lld markers)", i, (long long)first[i], (long long)(first[i] + count[i]),
                         (long long)n_markers);
    for (int j = 0; j < i; ++j)
      if (!(first[i] >= first[j] + count[j] || first[j] >= first[i] + count[i])) return ibm_message("bodies %d and %d overlap", j, i);
  }
  return {};
}

struct IbmBodyTables {
  std::string error;              // not empty: the declaration was refused, the tables are empty
  std::vector<int32_t> move_id;   // [n_markers]: body of the marker when that body moves, else -1
  std::vector<IbmLoadChunk> chunks;  // body after body
  std::vector<int32_t> chunk0;    // [n_bodies + 1]: first chunk of every body
  std::vector<int32_t> kind;      // [n_bodies]: IBM_BODY_*
  std::vector<double> rest;       // [n_bodies][18]: R = 1, c = centre0, w = v = 0
  bool any_moving = false;        // some moving body of either kind has markers: k_ibm_move runs
  bool any_prescribed = false;    // some body with markers follows staged poses
  bool any_dynamic = false;       // some body is free, with markers or without
};

// The tables of a declaration (ibm_check_bodies' checks first, then the moving flags)
inline IbmBodyTables ibm_body_tables(int64_t n_markers, int n_bodies, const int64_t* first, const int64_t* count, const int* moving, const double* centre0) {
  IbmBodyTables t;
  t.error = ibm_check_bodies(n_markers, n_bodies, first, count, moving, centre0);
  for (int i = 0; t.error.empty() && i < n_bodies; ++i)
    if (!(moving[i] >= IBM_BODY_REST && moving[i] <= IBM_BODY_DYNAMIC))
      t.error = ibm_message("body %d: bad moving flag %d (0 at rest, 1 prescribed, 2 dynamic)", i, moving[i]);
  if (!t.error.empty() || n_bodies <= 0) return t;
  t.kind.assign(moving, moving + n_bodies);
  t.move_id.assign((size_t)n_markers, -1);
  t.chunk0.assign((size_t)n_bodies + 1, 0);
  t.rest.assign((size_t)n_bodies * IBM_POSE_DOUBLES, 0.0);
  for (int i = 0; i < n_bodies; ++i) {
    if (moving[i]) {
      t.any_moving = t.any_moving || count[i] > 0;
      t.any_prescribed = t.any_prescribed || (moving[i] == IBM_BODY_PRESCRIBED && count[i] > 0);
      t.any_dynamic = t.any_dynamic || moving[i] == IBM_BODY_DYNAMIC;
      std::fill(t.move_id.begin() + first[i], t.move_id.begin() + first[i] + count[i], (int32_t)i);
    }
    t.chunk0[i] = (int32_t)t.chunks.size();
    for (int64_t o = 0; o < count[i]; o += IBM_LOADS_CHUNK)
      t.chunks.push_back(IbmLoadChunk{(int32_t)i, (int32_t)(first[i] + o), (int32_t)std::min<int64_t>(IBM_LOADS_CHUNK, count[i] - o)});
    double* P = t.rest.data() + (size_t)i * IBM_POSE_DOUBLES;
    P[0] = P[4] = P[8] = 1.0;
    for (int a = 0; a < 3; ++a) P[9 + a] = centre0[3 * i + a];
  }
  t.chunk0[n_bodies] = (int32_t)t.chunks.size();
  return t;
}

enum class IbmPoseSource { LIVE, REST, STAGED };       // the table k_ibm_pose wrote / the rest poses / the timestep's staged row
enum class IbmIntegrator { NONE, PLAIN, CONTACT };     // nothing / k_ibm_integrate / k_ibm_integrate_contact

// Which launches a step makes, from what was declared and switched on.  The launches of a run without free bodies and without a
// recorded pose history are exactly those of a stepper that has neither; so are those of free bodies with neither virtual mass
// nor contact.
struct IbmStepPlan {
  bool any_moving = false, any_prescribed = false, any_dynamic = false;  // of IbmBodyTables
  bool dynamics_set = false;     // the parameters and the initial state of the dynamic bodies have been uploaded
  bool virtual_on = false, contact_on = false;
  bool recording_poses = false;  // a pose history is being recorded

  // k_ibm_pose writes the live table before the move
  bool use_live() const { return any_dynamic || recording_poses; }
  // where the move and the loads read their poses
  IbmPoseSource pose_source() const { return use_live() ? IbmPoseSource::LIVE : any_prescribed ? IbmPoseSource::STAGED : IbmPoseSource::REST; }
  // staged rows are demanded only while some prescribed body moves (then k_ibm_pose is handed the timestep's row too)
  bool needs_staged() const { return any_prescribed; }
  bool moves() const { return any_moving; }
  // dynamic bodies cannot step before xlbhip_ibm_set_dynamics
  bool dynamics_missing() const { return any_dynamic && !dynamics_set; }
  IbmIntegrator integrator() const { return !any_dynamic ? IbmIntegrator::NONE : virtual_on || contact_on ? IbmIntegrator::CONTACT : IbmIntegrator::PLAIN; }
  // the contact kernel gets the radii only with contact on (null: virtual mass alone)
  bool passes_radius() const { return contact_on; }
};

}  // namespace xlb
