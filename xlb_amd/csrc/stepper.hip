// libxlbhip: the stepper.  Its caches, the launches of one step and of a fused pair of steps, the slab halo protocol, the fuse
// decision (step2_plan.hpp), and the stepper's C entry points.  The boundary tables (stepper_tables.hpp: BcTables, parsed by
// bc_tables.hpp) and the profile tables (profile_tables.hpp) have their own owners.
#include <array>
#include <map>
#include <memory>
#include <vector>

#include "api_internal.hpp"
#include "comm.hpp"
#include "profile_tables.hpp"
#include "stepper_tables.hpp"

using namespace xlb;

// what a cache was computed from: a field's address and contents version (versions are globally unique: a new field that
// recycles a freed one's address cannot match).  The empty key matches no field.
struct FieldKey {
  const xlbhip_field* field = nullptr;
  uint64_t version = 0;
  FieldKey() = default;
  FieldKey(const xlbhip_field* f) : field(f), version(f ? f->version : 0) {}
  bool operator==(const FieldKey& o) const { return field == o.field && version == o.version; }
};
struct MetaKey {
  FieldKey bc, miss;
  bool external_halo = false;
  bool operator==(const MetaKey& o) const { return bc == o.bc && miss == o.miss && external_halo == o.external_halo; }
};

// What the two-step kernel needs beyond the fields, cached between pairs (rules: the comment block below)
struct Step2Caches {
  DeviceBuf tile_order;  // uint32 block -> tile, hull tiles first (step2_tile_order)
  int order_ty = 0, order_tz = 0;
  DeviceBuf meta;  // uint32 id | missing << 8 per cell
  size_t meta_cells = 0;
  // the masks the meta words were built from: xlbhip_step2 called per pair (the Python stepper pairing reference-style
  // calls) must not rebuild them every time
  MetaKey meta_key;
  // per launch geometry (x_begin, x_count, segments) the per-block "no boundary cell" flags
  std::map<std::array<int, 3>, DeviceBuf> clean_cache;
  // result of the last "are all edge-kind cells in the x end planes" scan, and the bc_mask it holds for
  FieldKey scan_key;
  int scan_flag = 1;
  // extended BCs on the x end planes only (inlet / outlet): the end planes go through the single-step kernel twice via this
  // third population field
  xlbhip_field* scratch = nullptr;

  // (stream-ordered: the flags' last readers were enqueued before this point and hipFree synchronises)
  void drop_clean() { clean_cache.clear(); }
  // forget the meta words: the buffer (the transports may hold a registration of it), what it was built from, and the flags
  // computed from it
  void forget_meta(xlbhip_ctx* c) {
    if (meta) comm_forget_buffer(c, meta.get());
    (void)meta.reset();
    meta_cells = 0;
    meta_key = MetaKey();
    drop_clean();
  }
};

// The stepper owns its device tables through DeviceBuf members: the destructor releases them, a rebuild re-allocates in place.
// Its caches and when each is rebuilt or dropped:
//   meta words      rebuilt when either mask's address or contents version, or the external_halo option, differs from meta_key,
//                   or the cell count changed (prepare_fuse2, Step2Caches::forget_meta)
//   tile order      rebuilt when the tile counts (tys, tzs) of the (y, z) plane change (prepare_fuse2)
//   clean flags     per launch geometry; all dropped whenever the meta words or the tile order are rebuilt (Step2Caches::drop_clean)
//   edge-kind scan  redone when the bc mask's address or contents version differs from scan_key (can_fuse2)
//   scratch field   re-created when the population fields' shape or dtype differs (can_fuse2)
//   strip buffers   (the fields' own, common.hpp) valid iff strips_version == version && strips_oz == the launch's tile_oz
//   profile ring    dropped whenever the profile table's layout changes (ProfileTables::rebuild)
struct xlbhip_stepper : RowStepper {
  int collision = 0;
  Step2Caches pairs;
  ProfileTables prof;  // per-cell prescribed values and per-timestep wall velocities (profile_tables.hpp)
  bool forced = false;
  double force[3] = {0, 0, 0};
  double smag_cs = 0.17;
  // wall-distance weights of HybridBC cells (mesh maskers): host map (storage cell -> q weights) and its sorted device image
  std::map<uint32_t, std::array<float, 27>> dist_host;
  DeviceBuf dist_keys;  // uint32 [n_dist]
  DeviceBuf dist_vals;  // float [n_dist][q]
  int n_dist = 0;
};

namespace xlb {

static int launch_any(const xlbhip_stepper* s, const StepLaunch& p) {
  XLB_REQUIRE(p.n_prof == 0 || p.prof_vals, "step launch without its profile table (timestep not staged)");
  if (s->collision == XLBHIP_REGULARIZED_BGK || s->collision == XLBHIP_RECURSIVE_REGULARIZED_BGK) {
    const int coll = coll_of_public(s->collision) | (s->forced ? COLL_FORCED : 0);
    return launch_for_lattice(s->lattice, launch_step_d2q9_reg, launch_step_d3q19_reg, launch_step_d3q27_reg, p, coll);
  }
  if (s->forced || s->collision == XLBHIP_SMAGORINSKY_LES_BGK) {
    const int coll = s->collision | (s->forced ? COLL_FORCED : 0);
    return launch_for_lattice(s->lattice, launch_step_d2q9_ext, launch_step_d3q19_ext, launch_step_d3q27_ext, p, coll);
  }
  if (s->lattice == XLBHIP_D2Q9) return s->collision == XLBHIP_BGK ? launch_step_d2q9_bgk(p) : launch_step_d2q9_kbc(p);
  if (s->lattice == XLBHIP_D3Q19) return launch_step_d3q19_bgk(p);
  if (s->collision == XLBHIP_BGK) return launch_step_d3q27_bgk(p);
  return (p.fast_math && p.compute_dtype == XLBHIP_F64) ? launch_step_d3q27_kbc_fast64(p) : launch_step_d3q27_kbc(p);
}

static int check_step_fields(const xlbhip_stepper* s, const xlbhip_field* a, const xlbhip_field* b, const xlbhip_field* bcm,
                             const xlbhip_field* miss) {
  XLB_REQUIRE(s && a && b, "null argument");
  XLB_REQUIRE(a != b, "f_0 and f_1 must be different fields (double buffering)");
  const int q = lattice_q(s->lattice);
  XLB_REQUIRE(a->card == q && b->card == q, "population fields must have cardinality %d", q);
  XLB_REQUIRE(a->dtype == s->sdt && b->dtype == s->sdt, "population fields must have the stepper's store dtype %d", s->sdt);
  XLB_REQUIRE(same_grid(a, b) && a->halo == b->halo && a->plane_stride == b->plane_stride, "f_0 and f_1 layouts differ");
  if (s->bc.n_bc > 0) {
    XLB_REQUIRE(bcm, "this stepper has boundary conditions: bc_mask is required");
  }
  if (bcm) {
    XLB_REQUIRE(bcm->dtype == XLBHIP_U8 && bcm->card == 1 && same_grid(bcm, a) && bcm->halo == a->halo, "bad bc_mask field");
  }
  if (s->bc.needs_missing) {
    XLB_REQUIRE(miss && miss->dtype == XLBHIP_MISSING && same_grid(miss, a) && miss->halo == a->halo,
                "halfway bounce-back needs a missing_mask field on the same grid");
  }
  return 0;
}

// what a single step src -> dst at timestep t needs (a pair adds its own: make_launch2)
static StepLaunch make_launch(xlbhip_stepper* s, const xlbhip_field* src, xlbhip_field* dst, const xlbhip_field* bcm, const xlbhip_field* miss,
                              double omega, int64_t t) {
  xlbhip_ctx* c = s->ctx;
  StepLaunch p = bc_launch(c, s->bc, s->cdt, s->sdt, bcm, miss, src);
  p.src = src->data;
  p.dst = dst->data;
  p.prof_keys = s->prof.keys.get<uint32_t>();
  p.prof_vals = s->prof.table_at(t);  // (time-dependent walls: t's slot of the ring, checked resident by the caller)
  p.n_prof = s->prof.n;
  p.dist_keys = s->dist_keys.get<uint32_t>();
  p.dist_vals = s->dist_vals.get<float>();
  p.n_dist = s->n_dist;
  p.plane_stride = src->plane_stride;
  p.omega = omega;
  p.force[0] = s->force[0];
  p.force[1] = s->force[1];
  p.force[2] = s->force[2];
  p.smag_cs = s->smag_cs;
  p.vec = (int)opt(c, "vec", 0);
  p.has_bc = p.bc != nullptr ? (s->bc.extended_bcs ? 2 : 1) : 0;
  p.flags = (opt(c, "nt_store", 1) ? 1 : 0) | (int)(opt(c, "nt_load", 0) << 1);
  p.block_threads = (int)opt(c, "block_threads", 256);
  p.block_tz = (int)opt(c, "block_tz", 0);
  p.xcd_swizzle = (int)opt(c, "xcd_swizzle", 0);
  p.fast_math = opt(c, "exact_math", 0) ? 0 : 1;
  return p;
}

// the inputs of the two-step plan (step2_plan.hpp) for population fields laid out like f.  has_bc: the launches read a bc mask;
// edge_ext: every edge-kind cell sits in the x end planes (can_fuse2's scan)
static Step2Case plan_case(const xlbhip_stepper* s, const xlbhip_field* f, bool has_bc, bool edge_ext) {
  return {s->lattice, s->collision, s->cdt, s->sdt, opt(s->ctx, "exact_math", 0) ? 0 : 1, f->nx, f->ny, f->nz, f->halo,
          has_bc ? (s->bc.extended_bcs ? 2 : 1) : 0, edge_ext ? 1 : 0, s->bc.n_bc, s->bc.kinds_packed, s->bc.needs_missing ? 1 : 0};
}

// CUs the work items of the two-step kernel are to fill
static long fill_cus(const xlbhip_ctx* c) {
  const int64_t o = opt(c, "fuse2_cus", 0);
  return o > 0 ? (long)o : (c->compute_units > 0 ? c->compute_units : 256);
}

static int fuse2_segments(const xlbhip_stepper* s, const Step2Case& pc, int x_count) {
  return step2_segments(pc, x_count, fill_cus(s->ctx), (int)opt(s->ctx, "fuse2_xseg", 0), opt(s->ctx, "fuse2_clean", 1) != 0);
}

// the launch of a pair of steps src -> dst over all of x: the single step's part plus the two-step kernel's tables and geometry
static Step2Launch make_launch2(xlbhip_stepper* s, const Step2Case& pc, const xlbhip_field* src, xlbhip_field* dst, const xlbhip_field* bcm,
                                const xlbhip_field* miss, double omega, int64_t t) {
  xlbhip_ctx* c = s->ctx;
  Step2Launch p;
  static_cast<StepLaunch&>(p) = make_launch(s, src, dst, bcm, miss, omega, t);
  p.meta = s->pairs.meta.get<uint32_t>();
  // hull tiles first pays when they are much more expensive than fluid tiles (halfway walls: redirected loads) and
  // with clean work items; otherwise (fullway / equilibrium boundaries alone) the XCD-compact patch is faster
  const bool clean_on = p.has_bc && opt(c, "fuse2_clean", 1) != 0;
  p.tile_order = (p.has_bc && (s->bc.needs_missing || clean_on)) ? s->pairs.tile_order.get<uint32_t>() : nullptr;
  p.x_segments = fuse2_segments(s, pc, p.x_count);
  p.x_cap = clean_on ? 8 : 0;  // thin first / last x-segments: with walls on the x faces the inner segments are free of them
  const Step2Tile tile = step2_tile(s->lattice, s->collision, p.has_bc != 0);
  p.tile_ty = tile.ty;
  p.tile_tz = tile.tz;
  if (p.has_bc) {  // half-tile shift: both walls of an axis in one (wrapping) tile row
    p.tile_oy = p.tile_ty / 2;
    p.tile_oz = p.tile_tz / 2;
  }
  p.fast_bgk = (opt(c, "fast_bgk", 0) && !opt(c, "exact_math", 0)) ? 1 : 0;
  p.xcd_swizzle = 1;
  return p;
}

// the stepper's sparse tables for the whole-field kernels; prof_vals: the profile table of the timestep in question
static CellTables cell_tables(const xlbhip_stepper* s, const void* prof_vals) {
  return {s->prof.keys.get<uint32_t>(), prof_vals, s->prof.n, s->dist_keys.get<uint32_t>(), s->dist_vals.get<float>(), s->n_dist};
}

// the outflow pass (stepper_tables.hpp: outflow_aux) after a step src -> dst at timestep t
static int outflow_aux(xlbhip_stepper* s, const xlbhip_field* src, xlbhip_field* dst, const xlbhip_field* bcm, const xlbhip_field* miss,
                       int64_t t) {
  if (!s->bc.has_outflow) return 0;
  const void* pv = s->prof.table_at(t);
  XLB_REQUIRE(s->prof.n == 0 || pv, "outflow pass without its profile table (timestep %lld not staged)", (long long)t);
  return outflow_aux(s->ctx, s->lattice, s->cdt, s->bc, cell_tables(s, pv), src, dst, bcm, miss);
}

// The plan report (xlbhip_step2_plan): step_twice run with a Step2Report takes every decision of a pass and builds the cached tables
// a pass builds, but each two-step launch is written down here instead of being enqueued, and nothing else is launched or touched.
// Words: [0] = launches; per launch x_begin, x_count, effective segments, effective cap, tile_ty, tile_tz, tile_oy, tile_oz,
// strips mode, items, then per item (= block) tile, x_lo, x_hi, clean flag as the kernel reads it (0 where the launch has no flags).
struct Step2Report {
  std::vector<int32_t> words = std::vector<int32_t>(1, 0);
};

static int report_step2(const Step2Launch& p, Step2Report& rep) {
  const int items = step2_items(p);
  DeviceBuf d_items;
  XLB_HIP(d_items.alloc((size_t)items * 3 * sizeof(int32_t)));
  int segments = 0, cap = 0;  // the effective ones, from the launcher's own rules (step2_launch.hpp)
  if (int rc = step2_report_items(p, d_items.get<int32_t>(), &segments, &cap)) return rc;
  std::vector<int32_t> host((size_t)items * 3);
  std::vector<uint8_t> flags((size_t)items, 0);
  XLB_HIP(hipMemcpyAsync(host.data(), d_items.get(), host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, p.stream));
  if (p.clean) XLB_HIP(hipMemcpyAsync(flags.data(), p.clean, flags.size(), hipMemcpyDeviceToHost, p.stream));
  XLB_HIP(hipStreamSynchronize(p.stream));
  for (int v : {p.x_begin, p.x_count, segments, cap, p.tile_ty, p.tile_tz, p.tile_oy, p.tile_oz, (int)p.strips, items})
    rep.words.push_back(v);
  for (int i = 0; i < items; ++i)
    for (int v : {host[3 * i], host[3 * i + 1], host[3 * i + 2], (int)flags[i]}) rep.words.push_back(v);
  rep.words[0] += 1;
  return 0;
}

static int launch_step2(xlbhip_stepper* s, Step2Launch p, Step2Report* rep = nullptr) {
  if (s->lattice == XLBHIP_D3Q27 && s->collision == XLBHIP_KBC) return rep ? report_step2(p, *rep) : launch_step2_d3q27_kbc(p);
  p.clean = nullptr;
  if (p.has_bc && p.meta && opt(s->ctx, "fuse2_clean", 1)) {
    // what the block -> (tile, x-segment) mapping depends on and may differ between the launches of one stepper (tile, shift and
    // order are the stepper's; x_cap follows fuse2_clean): the flags say "no boundary cell in THIS block's item"
    const std::array<int, 3> key = {p.x_begin, p.x_count, p.x_segments};
    auto it = s->pairs.clean_cache.find(key);
    if (it == s->pairs.clean_cache.end()) {
      DeviceBuf flags;
      XLB_HIP(flags.alloc((size_t)step2_items(p)));
      if (int rc = step2_build_clean(p, flags.get<uint8_t>())) return rc;
      it = s->pairs.clean_cache.emplace(key, std::move(flags)).first;
    }
    p.clean = it->second.get<uint8_t>();
  }
  if (rep) return report_step2(p, *rep);
  if (s->lattice == XLBHIP_D3Q27) return launch_step2_d3q27_bgk(p);
  return p.strips != Strips::none ? launch_step2_d3q19_bgk_strips(p) : launch_step2_d3q19_bgk(p);
}

// strip buffer of a population field (1 / 32 of it): allocated on first use; false (and no error) when there is no memory for it
static bool ensure_strips(xlbhip_field* f) {
  if (f->strips) return true;
  const size_t bytes = f->planes * f->plane_stride * dtype_size(f->dtype) / 32 + 512;
  if (hipMalloc(&f->strips, bytes) != hipSuccess) {
    f->strips = nullptr;
    (void)hipGetLastError();
    return false;
  }
  f->strips_version = 0;
  f->strips_oz = -1;
  return true;
}

// Pair of steps for a stepper whose Zou-He / Regularized / outflow cells all sit in the planes x = 0 and x = nx - 1
// (inlet / outlet faces): the two-step kernel updates the planes 2 .. nx-3, whose two-step cone never evaluates such a
// cell (its f(t+1) on the planes 1 and nx-2 only PULLS from the end planes), and the four end planes go through the
// single-step kernel twice with a third population field holding their f(t+1).  The first of those launches reads the
// profile table of timestep t, the second that of t + 1 (time-dependent walls on the end planes).
static int step_twice_edge_ext(xlbhip_stepper* s, const Step2Case& pc, Step2Launch p, const xlbhip_field* src, xlbhip_field* dst, const xlbhip_field* bcm,
                               const xlbhip_field* miss, double omega, int64_t t, Step2Report* rep) {
  XLB_REQUIRE(s->pairs.scratch && s->pairs.scratch->plane_stride == src->plane_stride, "scratch field missing (can_fuse2 allocates it)");
  const int nx = src->nx;
  p.x_begin = 2;
  p.x_count = nx - 4;
  p.x_segments = fuse2_segments(s, pc, p.x_count);
  if (rep) return report_step2(p, *rep);
  if (int rc = launch_step2_d3q19_bgk(p)) return rc;  // (directly: no clean flags, no strips)
  // end planes, step 1: f(t+1) on the planes nx-3 .. nx-1 and 0 .. 2 -> scratch
  StepLaunch q = make_launch(s, src, s->pairs.scratch, bcm, miss, omega, t);
  q.x_begin = nx - 3;
  q.x_count = 3;
  if (int rc = launch_any(s, q)) return rc;
  q.x_begin = 0;
  if (int rc = launch_any(s, q)) return rc;
  if (int rc = outflow_aux(s, src, s->pairs.scratch, bcm, miss, t)) return rc;
  // step 2: f(t+2) on the planes nx-2, nx-1, 0, 1 -> dst
  StepLaunch r = make_launch(s, s->pairs.scratch, dst, bcm, miss, omega, t + 1);
  r.x_begin = nx - 2;
  r.x_count = 2;
  if (int rc = launch_any(s, r)) return rc;
  r.x_begin = 0;
  if (int rc = launch_any(s, r)) return rc;
  return outflow_aux(s, s->pairs.scratch, dst, bcm, miss, t + 1);
}

// the compute stream waits for the halo exchange; with the telemetry on, the wait is bracketed by two timing events
static int wait_for_halo(xlbhip_ctx* c) {
  if (!opt(c, "halo_telemetry", 1)) {
    XLB_HIP(hipStreamWaitEvent(c->stream, c->ev_halo, 0));
    return 0;
  }
  const int slot = c->wait_head;
  c->wait_head = (c->wait_head + 1) % xlbhip_ctx::WAIT_RING;
  if (int rc = harvest_wait(c, slot)) return rc;  // (32 exchanges old: long complete)
  if (!c->ev_w0[slot]) {
    XLB_HIP(hipEventCreate(&c->ev_w0[slot]));
    XLB_HIP(hipEventCreate(&c->ev_w1[slot]));
  }
  XLB_HIP(hipEventRecord(c->ev_w0[slot], c->stream));
  XLB_HIP(hipStreamWaitEvent(c->stream, c->ev_halo, 0));
  XLB_HIP(hipEventRecord(c->ev_w1[slot], c->stream));
  c->wait_used[slot] = true;
  return 0;
}

// One pass over a slab with ghost planes: the ghosts of src are refilled from the ring neighbours on the comm stream (comm.cpp,
// `depth` planes per side) while the planes that need none of them are updated (role interior); the `edge` planes per side
// follow.  Without overlap the whole slab is updated after the exchange (role whole).  launch(x_begin, x_count, role) enqueues
// the kernels of a plane range on the compute stream.
enum class SlabRole { interior, whole, edge };

template <class Launch>
static int slab_pass(xlbhip_ctx* c, int lattice, xlbhip_field* src, int depth, int edge, bool overlap, Launch&& launch) {
  XLB_HIP(hipEventRecord(c->ev_edge, c->stream));  // src complete (previous pass)
  if (overlap) {
    // the interior launch goes out BEFORE the exchange is enqueued: posting an exchange costs host time (dozens of copy /
    // send calls, some of which the runtime may only accept once earlier work of the communication stream has finished —
    // measured with the ipc transport: 1 ms of exposed wait per pair when the launch came second) and the device must
    // already have the interior to work on meanwhile
    if (int rc = launch(edge, src->nx - 2 * edge, SlabRole::interior)) return rc;
  }
  XLB_HIP(hipStreamWaitEvent(c->comm_stream, c->ev_edge, 0));
  if (int rc = halo_exchange_on(c, lattice, src, c->comm_stream, depth)) return rc;
  XLB_HIP(hipEventRecord(c->ev_halo, c->comm_stream));
  if (!overlap) {
    XLB_HIP(hipStreamWaitEvent(c->stream, c->ev_halo, 0));
    return launch(0, src->nx, SlabRole::whole);
  }
  if (int rc = wait_for_halo(c)) return rc;
  if (int rc = launch(0, edge, SlabRole::edge)) return rc;
  return launch(src->nx - edge, edge, SlabRole::edge);
}

// what can_fuse2 decided for a pair of fields: whether pairs of steps go through the two-step kernel, and whether their x end
// planes go through the single-step kernel (step_twice_edge_ext)
struct Fuse2 {
  bool fuse = false, edge_ext = false;
};

// two steps in one pass (a -> scratch-free: src -> dst holds f(t+2)); `how`: the caller's can_fuse2 of these fields (how.fuse)
// rep: write the pass's two-step launches down instead of running it (Step2Report)
static int step_twice(xlbhip_stepper* s, Fuse2 how, const xlbhip_field* src, xlbhip_field* dst, const xlbhip_field* bcm,
                      const xlbhip_field* miss, double omega, int64_t t, Step2Report* rep = nullptr) {
  const Step2Case pc = plan_case(s, src, s->bc.n_bc > 0 && bcm, how.edge_ext);
  Step2Launch p = make_launch2(s, pc, src, dst, bcm, miss, omega, t);
  xlbhip_ctx* c = s->ctx;
  if (!rep) touch(dst);  // (new contents: whatever was cached on the old ones — its strip buffer — is stale)
  if (how.edge_ext) return step_twice_edge_ext(s, pc, p, src, dst, bcm, miss, omega, t, rep);
  // strip buffers (step2_kernel.hpp): phase A's halo columns come from src's strips, phase B writes dst's.  D3Q19, the
  // bit-exact body, (8 x 64) tiles; a field whose strips are not those of its current contents gets them rebuilt first.
  xlbhip_field* srcw = const_cast<xlbhip_field*>(src);
  const bool native_slab = src->halo > 0 && !opt(c, "external_halo", 0);
  // With boundary conditions only: there they buy 1-3 % (cavity 512^3, interleaved A/B: halfway 2.353 -> 2.334, fullway 2.220 -> 2.149
  // ms/step); the BC-free kernel is faster with row-aligned lanes alone (2.12 against 2.18 with strips, 2.29 before: profiles/r03/step2_strips.md).
  // fuse2_strips = 2 forces them for every D3Q19 stepper.
  const int64_t strips_opt = opt(c, "fuse2_strips", 1);
  const bool strips = (strips_opt == 2 || (strips_opt == 1 && p.has_bc)) && s->lattice == XLBHIP_D3Q19 && !p.fast_bgk && p.tile_ty == 8 && p.tile_tz == 64 &&
                      (src->halo == 0 || native_slab) && src->nx >= 8 && (rep || (ensure_strips(srcw) && ensure_strips(dst)));  // (a report allocates none)
  // q writes dst's strips, and reads src's when they are those of src's current contents (all interior planes).  After anything but
  // a strip-writing pass wrote src — a single step, an upload — the first pass only WRITES strips (no separate rebuild pass: at 512^3
  // that would cost 1.5 ms, a third of a pair, inside e.g. the driver's 20-step timed region after its 5 warm-up steps).
  auto read_strips = [&](Step2Launch& q) {
    const bool valid = srcw->strips && srcw->strips_version == srcw->version && srcw->strips_oz == q.tile_oz;
    q.strips = valid ? Strips::read_write : Strips::write;
    q.strips_src = valid ? srcw->strips : nullptr;
    q.strips_dst = dst->strips;
  };
  const bool rowmap_only = !strips && opt(c, "fuse2_rowmap", 0) != 0 && p.has_bc && s->lattice == XLBHIP_D3Q19 && !p.fast_bgk && p.tile_ty == 8 && p.tile_tz == 64;
  if (rowmap_only) p.strips = Strips::rowmap;
  auto dst_strips_done = [&]() {  // every interior plane of dst was written by strip-writing launches
    dst->strips_version = dst->version;
    dst->strips_oz = p.tile_oz;
  };
  if (src->halo == 0 || opt(c, "external_halo", 0)) {
    if (strips) read_strips(p);
    if (int rc = launch_step2(s, p, rep)) return rc;
    if (strips && !rep) dst_strips_done();
    return 0;
  }
  // slab protocol for a PAIR of steps: the two ghost planes per side of src are refilled (depth 2) while the planes whose
  // two-step cone stays inside the slab are updated; the two edge plane pairs follow (each warms its own 3-plane window up
  // from the fresh ghosts).
  const bool overlap = opt(c, "overlap", 1) != 0 && src->nx >= 16;
  auto launch = [&](int x_begin, int x_count, SlabRole role) -> int {
    Step2Launch q = p;
    q.x_begin = x_begin;
    q.x_count = x_count;
    q.x_segments = role == SlabRole::edge ? 1 : fuse2_segments(s, pc, x_count);
    if (strips && role == SlabRole::interior) {
      read_strips(q);
    } else if (strips) {  // launches whose phase A pulls from ghost planes (no strips there) only WRITE strips
      q.strips = Strips::write;
      q.strips_dst = dst->strips;
    }
    return launch_step2(s, q, rep);
  };
  if (rep) {  // slab_pass's launches in its order, without the exchange
    if (!overlap) return launch(0, src->nx, SlabRole::whole);
    if (int rc = launch(2, src->nx - 4, SlabRole::interior)) return rc;
    if (int rc = launch(0, 2, SlabRole::edge)) return rc;
    return launch(src->nx - 2, 2, SlabRole::edge);
  }
  if (int rc = slab_pass(c, s->lattice, srcw, 2, 2, overlap, launch)) return rc;
  if (strips) dst_strips_done();
  return 0;
}

// Whether pairs of steps on these fields go through the two-step kernel.  May run the edge-kind scan of bcm and allocate the
// scratch field; changes nothing else of the stepper.
static Fuse2 can_fuse2(xlbhip_stepper* s, const xlbhip_field* src, const xlbhip_field* bcm) {
  const int64_t mode = opt(s->ctx, "fuse2", 1);
  if (mode == 0 || s->forced) return {};
  bool edge_ext = false;
  if (s->bc.has_edge_kinds) {
    // Zou-He / Regularized / outflow / do-nothing cells: fine when they all sit in the two x end planes (scan of bc_mask, 1 B / cell)
    if (!bcm || src->halo != 0 || src->nx < 16 || s->lattice != XLBHIP_D3Q19) return {};
    xlbhip_ctx* c = s->ctx;
    if (!(s->pairs.scan_key == FieldKey(bcm))) {  // one scan per (stepper, bc_mask contents), not per run
      DeviceBuf dflag;
      int flag = 1;
      if (dflag.alloc(sizeof(int)) != hipSuccess) return {};
      (void)hipMemsetAsync(dflag.get(), 0, sizeof(int), c->stream);
      hipLaunchKernelGGL(k_ext_interior_scan, blocks_for(bcm->cells()), 256, 0, c->stream, view(bcm), s->bc.tab_kind.get<uint8_t>(), dims(bcm),
                         dflag.get<int>());
      if (hipMemcpyAsync(&flag, dflag.get(), sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        flag = 1;
      s->pairs.scan_key = FieldKey(bcm);
      s->pairs.scan_flag = flag;
    }
    if (s->pairs.scan_flag != 0) return {};
    // the end planes need a third population field; without the memory for it the stepper stays on single steps
    if (!s->pairs.scratch || s->pairs.scratch->nx != src->nx || s->pairs.scratch->ny != src->ny || s->pairs.scratch->nz != src->nz || s->pairs.scratch->dtype != src->dtype) {
      if (s->pairs.scratch) xlbhip_field_destroy(s->pairs.scratch);
      s->pairs.scratch = nullptr;
      if (xlbhip_field_create(c, src->card, src->nx, src->ny, src->nz, src->dtype, src->halo, 0.0, &s->pairs.scratch) != 0 ||
          s->pairs.scratch->plane_stride != src->plane_stride) {
        if (s->pairs.scratch) xlbhip_field_destroy(s->pairs.scratch);
        s->pairs.scratch = nullptr;
        (void)hipGetLastError();
        return {};
      }
    }
    edge_ext = true;
  }
  const Step2Case pc = plan_case(s, src, s->bc.n_bc > 0 && bcm, edge_ext);
  const bool fuse = step2_fuse(pc, (int)mode, fill_cus(s->ctx), (int)opt(s->ctx, "fuse2_xseg", 0), opt(s->ctx, "fuse2_clean", 1) != 0);
  return {fuse, fuse && edge_ext};
}

// per-run tables of the two-step kernel: the meta words (bc kind | slot | missing bits per cell, ghost planes
// included) and the hull-first tile order
static int prepare_fuse2(xlbhip_stepper* s, const xlbhip_field* bcm, const xlbhip_field* miss) {
  if (!(s->bc.n_bc > 0 && bcm)) return 0;
  xlbhip_ctx* c = s->ctx;
  const size_t cells = bcm->cells_with_halo();
  if (s->pairs.meta_cells != cells) {
    s->pairs.forget_meta(c);  // (contents gone: rebuilt below)
    XLB_HIP(s->pairs.meta.alloc(cells * sizeof(uint32_t)));
    s->pairs.meta_cells = cells;
  }
  const Step2Tile tile = step2_tile(s->lattice, s->collision, true);
  const int tys = bcm->ny / tile.ty, tzs = bcm->nz / tile.tz;
  if (s->pairs.order_ty != tys || s->pairs.order_tz != tzs) {
    const std::vector<uint32_t> order = step2_tile_order(tys, tzs);
    s->pairs.drop_clean();  // the flags were computed for the old block -> tile mapping
    if (int rc = upload_bytes(order.data(), order.size() * sizeof(uint32_t), s->pairs.tile_order)) return rc;
    s->pairs.order_ty = tys;
    s->pairs.order_tz = tzs;
  }
  const MetaKey key{FieldKey(bcm), FieldKey(miss), opt(c, "external_halo", 0) != 0};
  if (s->pairs.meta_key == key) return 0;  // meta words, tile order and clean flags are those of these very masks
  s->pairs.meta_key = key;
  s->pairs.drop_clean();
  hipLaunchKernelGGL(k_build_meta, blocks_for(cells), 256, 0, c->stream, static_cast<const uint8_t*>(bcm->data),
                     miss ? static_cast<const uint32_t*>(miss->data) : nullptr, s->pairs.meta.get<uint32_t>(), cells, s->bc.ids_packed, s->bc.kinds_packed,
                     s->bc.moving_mask, s->lattice == XLBHIP_D3Q27 ? 1 : 0);
  XLB_HIP(hipGetLastError());
  // slab decomposition: phase A also runs on the ghost planes -1 and nx, so it needs the neighbours' boundary
  // information there.  Host-staged transports (external_halo) fill the ghost planes of the masks themselves.
  if (bcm->halo > 0 && !opt(c, "external_halo", 0))
    return plane_exchange_on(c, s->pairs.meta.get(), sizeof(uint32_t), bcm->nx, bcm->ny, bcm->nz, bcm->halo, c->stream);
  return 0;
}

// the step kernel(s) of one step src -> dst, with the slab halo protocol when the fields carry ghost planes
static int step_kernels(xlbhip_stepper* s, const xlbhip_field* src, xlbhip_field* dst, const xlbhip_field* bcm, const xlbhip_field* miss,
                     double omega, int64_t t) {
  xlbhip_ctx* c = s->ctx;
  StepLaunch p = make_launch(s, src, dst, bcm, miss, omega, t);
  if (src->halo == 0 || opt(c, "external_halo", 0)) return launch_any(s, p);  // (p covers all of x)
  // slab protocol for one step.
  // The launch that runs BEFORE this step's exchange has completed must not write a plane a neighbour may still be pulling
  // (ipc transport: the puller, not the owner, knows when a pull is done; what orders the two is that the owner's edge launches
  // wait for the NEXT exchange, which the neighbour posts after its pulls).  On fields with two ghost planes the previous exchange
  // may have been a fused pair's — planes 0, 1, nx - 2, nx - 1 of `dst` lent out — so their "edge" is two planes wide.
  const int edge = src->halo >= 2 ? 2 : 1;
  const bool overlap = opt(c, "overlap", 1) != 0 && src->nx > 2 * edge;
  return slab_pass(c, s->lattice, const_cast<xlbhip_field*>(src), 1, edge, overlap, [&](int x_begin, int x_count, SlabRole) {
    p.x_begin = x_begin;
    p.x_count = x_count;
    return launch_any(s, p);
  });
}

// one step src -> dst; ExtrapolationOutflowBC cells get their auxiliary data afterwards (nse_stepper.py:270-272)
static int step_once(xlbhip_stepper* s, const xlbhip_field* src, xlbhip_field* dst, const xlbhip_field* bcm, const xlbhip_field* miss,
                     double omega, int64_t t) {
  touch(dst);  // (its strip buffer, if any, no longer matches)
  if (int rc = step_kernels(s, src, dst, bcm, miss, omega, t)) return rc;
  return outflow_aux(s, src, dst, bcm, miss, t);
}

}  // namespace xlb

extern "C" {

int xlbhip_stepper_create(xlbhip_ctx* c, int lattice, int collision, int cdt, int sdt, int n_bc, const xlbhip_bc_desc* bcs,
                          xlbhip_stepper** out) {
  XLB_REQUIRE(collision >= XLBHIP_BGK && collision <= XLBHIP_RECURSIVE_REGULARIZED_BGK, "unknown collision %d", collision);
  XLB_REQUIRE(!(collision == XLBHIP_KBC && lattice == XLBHIP_D3Q19), "Velocity set not supported: D3Q19 has no KBC (reference kbc.py:65-66)");
  XLB_REQUIRE(cdt == XLBHIP_F32 || cdt == XLBHIP_F64, "bad compute dtype %d", cdt);
  XLB_REQUIRE(is_float(sdt) && dtype_size(sdt) <= dtype_size(cdt), "bad store dtype %d for compute dtype %d", sdt, cdt);
  const auto refusal = [&](int kind) { return bc_stepper_refusal(lattice_q(lattice), kind); };
  const auto own = [&](xlbhip_stepper& s) {
    s.collision = collision;
    s.prof.ctx = c;
    s.prof.cdt = cdt;
    return 0;
  };
  return create_row_stepper(c, lattice, cdt, sdt, n_bc, bcs, nullptr, refusal, own, out);  // (all five policies: checked above)
}

}  // extern "C"

// flag the BC: its prescribed values come from the profile table (cell.hpp: PROF_FLAG)
static int flag_profile_bc(xlbhip_stepper* s, int bc_id) {
  const std::vector<char> one = compute_image(s->cdt, {1.0});
  XLB_HIP(hipMemcpy(s->bc.tab_values.get<char>() + ((size_t)bc_id * 27 + PROF_FLAG) * one.size(), one.data(), one.size(), hipMemcpyHostToDevice));
  return 0;
}

extern "C" {

int xlbhip_stepper_set_bc_profile(xlbhip_stepper* s, int bc_id, int64_t n, const uint32_t* storage_cells, const double* values) {
  XLB_REQUIRE(s && bc_id >= 1 && bc_id <= 255, "bad argument");
  XLB_REQUIRE(n == 0 || (storage_cells && values), "null table");
  XLB_HIP(hipSetDevice(s->ctx->device));
  if (int rc = s->prof.add_static(n, storage_cells, values)) return rc;
  return flag_profile_bc(s, bc_id);
}

int xlbhip_stepper_set_bc_profile_cells(xlbhip_stepper* s, int bc_id, int64_t n, const uint32_t* storage_cells) {
  XLB_REQUIRE(s && bc_id >= 1 && bc_id <= 255, "bad argument");
  XLB_REQUIRE(n == 0 || storage_cells, "null cell list");
  XLB_HIP(hipSetDevice(s->ctx->device));
  const uint8_t kind = s->bc.kind_host[bc_id];
  XLB_REQUIRE(bc_has_wall_table(kind),
              "time-dependent wall velocities: bc %d is of kind %d (HybridBC / HalfwayBounceBackBC with a profile)", bc_id, (int)kind);
  if (int rc = s->prof.declare_time_dependent(bc_id, n, storage_cells)) return rc;
  return flag_profile_bc(s, bc_id);
}

int xlbhip_stepper_profile_slots(xlbhip_stepper* s, int* slots) {
  XLB_REQUIRE(s && slots, "null argument");
  *slots = s->prof.slot_count();
  return 0;
}

int xlbhip_stepper_stage_bc_profiles(xlbhip_stepper* s, int64_t t_first, int64_t n_steps, const double* values) {
  XLB_REQUIRE(s, "stepper is null");
  XLB_REQUIRE(s->prof.has_td(), "this stepper has no time-dependent wall velocities (xlbhip_stepper_set_bc_profile_cells)");
  XLB_REQUIRE(n_steps >= 0 && (n_steps == 0 || values), "bad argument");
  XLB_HIP(hipSetDevice(s->ctx->device));
  return s->prof.stage(t_first, n_steps, values);
}

int xlbhip_stepper_momentum_transfer(xlbhip_stepper* s, int bc_id, const xlbhip_field* f_0, const xlbhip_field* bcm, const xlbhip_field* miss,
                                     double force_out[3]) {
  return xlbhip_stepper_momentum_transfer_at(s, bc_id, 0, f_0, bcm, miss, force_out);
}

int xlbhip_stepper_momentum_transfer_at(xlbhip_stepper* s, int bc_id, int64_t timestep, const xlbhip_field* f_0, const xlbhip_field* bcm,
                                        const xlbhip_field* miss, double force_out[3]) {
  XLB_REQUIRE(s && force_out && bc_id >= 1 && bc_id <= 255, "bad argument");
  xlbhip_ctx* c = s->ctx;
  XLB_CHECK_POP(f_0, s->lattice, "momentum_transfer(f_0)");
  XLB_REQUIRE(bcm && bcm->dtype == XLBHIP_U8 && bcm->card == 1 && same_grid(bcm, f_0) && bcm->halo == f_0->halo, "momentum_transfer: bad bc_mask field");
  XLB_REQUIRE(miss && miss->dtype == XLBHIP_MISSING && same_grid(miss, f_0) && miss->halo == f_0->halo, "momentum_transfer: needs the missing_mask field");
  XLB_REQUIRE(f_0->halo == 0, "momentum_transfer through the stepper's tables: fields without ghost planes (mesh / profile BCs live on one rank)");
  const uint8_t kind = s->bc.kind_host[bc_id];
  XLB_HIP(hipSetDevice(c->device));
  XLB_REQUIRE(bc_has_wall_table(kind),
              "momentum_transfer through the stepper: bc %d is of kind %d (HybridBC / profile walls; plain walls use xlbhip_momentum_transfer)", bc_id,
              (int)kind);
  const void* pv = s->prof.table_for(bc_id, timestep);
  XLB_REQUIRE(s->prof.n == 0 || pv, "momentum_transfer: the time-dependent wall velocities of timestep %lld are not staged", (long long)timestep);
  DeviceBuf dforce;
  XLB_HIP(dforce.alloc(3 * sizeof(double)));
  XLB_HIP(hipMemsetAsync(dforce.get(), 0, 3 * sizeof(double), c->stream));
  const size_t n = f_0->cells();
  const int rc = by_lattice(s->lattice, [&](auto L) {
    return by_compute(s->cdt, [&](auto T) {
      using TT = decltype(T);
      hipLaunchKernelGGL((k_momentum_transfer_tab<decltype(L), TT>), blocks_for(n), BC_BLOCK, 0, c->stream, view(f_0), view(bcm), view(miss), dims(f_0), bc_id,
                         bc_view<TT>(s->bc, cell_tables(s, pv)), dforce.get<double>());
      XLB_HIP(hipGetLastError());
      return 0;
    });
  });
  if (rc) return rc;
  hipError_t e = hipMemcpyAsync(force_out, dforce.get(), 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  XLB_REQUIRE(e == hipSuccess, "momentum_transfer: %s", hipGetErrorString(e));
  return 0;
}

int xlbhip_stepper_set_bc_distances(xlbhip_stepper* s, int64_t n, const uint32_t* storage_cells, const float* weights) {
  XLB_REQUIRE(s, "stepper is null");
  XLB_REQUIRE(n == 0 || (storage_cells && weights), "null table");
  xlbhip_ctx* c = s->ctx;
  const int q = lattice_q(s->lattice);
  XLB_HIP(hipSetDevice(c->device));
  XLB_HIP(hipStreamSynchronize(c->stream));
  for (int64_t i = 0; i < n; ++i) {
    std::array<float, 27> w{};
    for (int l = 0; l < q; ++l) w[(size_t)l] = weights[i * q + l];
    s->dist_host[storage_cells[i]] = w;
  }
  std::vector<uint32_t> keys;
  std::vector<float> vals;
  sorted_table(s->dist_host, (size_t)q, keys, vals);
  s->n_dist = (int)keys.size();
  if (int rc = upload_keys(keys, s->dist_keys)) return rc;
  return upload_bytes(vals.data(), vals.size() * sizeof(float), s->dist_vals);
}

int xlbhip_stepper_set_force(xlbhip_stepper* s, const double* force) {
  XLB_REQUIRE(s, "stepper is null");
  s->forced = force != nullptr;
  for (int a = 0; a < 3; ++a) s->force[a] = force ? force[a] : 0.0;
  return 0;
}

int xlbhip_stepper_set_smagorinsky(xlbhip_stepper* s, double coef) {
  XLB_REQUIRE(s, "stepper is null");
  s->smag_cs = coef;
  return 0;
}

int xlbhip_stepper_destroy(xlbhip_stepper* s) {
  return destroy_drained(s, [&] {
    s->prof.release();  // (explicitly here, after the drain: copies may still read the pinned rows)
    s->pairs.forget_meta(s->ctx);
    if (s->pairs.scratch) xlbhip_field_destroy(s->pairs.scratch);
  });  // (the device tables go with their owners)
}

int xlbhip_step(xlbhip_stepper* s, const xlbhip_field* src, xlbhip_field* dst, const xlbhip_field* bcm, const xlbhip_field* miss,
                double omega, int64_t timestep) {
  // the timestep selects the wall velocities of time-dependent profiles (nse_stepper.py:370-378 passes it to every BC functional)
  if (int rc = check_step_fields(s, src, dst, bcm, miss)) return rc;
  if (int rc = s->prof.require_staged(timestep, 1)) return rc;
  return step_once(s, src, dst, bcm, miss, omega, timestep);
}

// n steps; `fixed_placement`: the result must land in f_a for even n and in f_b for odd n (xlbhip_run's contract);
// otherwise every pair of steps is fused and *result_in_b reports where the result is (xlbhip_run_any)
static int run_steps(xlbhip_stepper* s, xlbhip_field* a, xlbhip_field* b, const xlbhip_field* bcm, const xlbhip_field* miss, double omega,
                     int64_t t0, int64_t n, bool fixed_placement, int* result_in_b) {
  XLB_REQUIRE(n >= 0, "n_steps < 0");
  if (int rc = check_step_fields(s, a, b, bcm, miss)) return rc;
  if (int rc = s->prof.require_staged(t0, n)) return rc;
  // With two-step fusion ("fuse2") a pair of steps is ONE pass a -> b: pairs alternate direction (a -> b, b -> a, ...).
  // Under the fixed placement contract a trailing half pair (buffer parity) is fixed up by single steps.
  int64_t i = 0;
  xlbhip_field* cur = a;
  xlbhip_field* oth = b;
  // (a host-staged transport refills the ghosts between calls: it drives pairs through xlbhip_step2 itself)
  const bool caller_fills_ghosts = a->halo > 0 && opt(s->ctx, "external_halo", 0) != 0;
  Fuse2 how = (n >= 2 && !caller_fills_ghosts) ? can_fuse2(s, a, bcm) : Fuse2();
  if (n >= 2 && a->halo > 0 && !caller_fills_ghosts && comm_ranks(s->ctx) > 1) {
    // pairs and single steps post different message sets (depth-2 / depth-1 exchange, meta planes): every rank must take
    // the same decision, and uneven slabs may sit on either side of the chip-filling rule -> MIN over the ranks
    int all = 0;
    if (int rc = comm_all_min(s->ctx, how.fuse ? 1 : 0, &all)) return rc;
    how.fuse = all != 0;
  }
  if (how.fuse) {
    if (int rc = prepare_fuse2(s, bcm, miss)) return rc;
    // choose the number of pairs so that the remaining single steps land the result in the right buffer:
    // after P pairs the data sits in (P odd ? b : a); then r = n - 2P single steps flip r more times.
    // P + r must be congruent to n (mod 2)  <=>  P even.  Use the largest even P with 2P <= n.
    int64_t pairs = fixed_placement ? ((n / 2) & ~int64_t(1)) : n / 2;
    for (int64_t k = 0; k < pairs; ++k) {
      if (int rc = step_twice(s, how, cur, oth, bcm, miss, omega, t0 + 2 * k)) return rc;
      xlbhip_field* tmp = cur;
      cur = oth;
      oth = tmp;
    }
    i = 2 * pairs;
  }
  for (; i < n; ++i) {
    if (int rc = step_once(s, cur, oth, bcm, miss, omega, t0 + i)) return rc;
    xlbhip_field* tmp = cur;
    cur = oth;
    oth = tmp;
  }
  if (result_in_b) *result_in_b = cur == b ? 1 : 0;
  return 0;
}

int xlbhip_run(xlbhip_stepper* s, xlbhip_field* a, xlbhip_field* b, const xlbhip_field* bcm, const xlbhip_field* miss, double omega,
               int64_t t0, int64_t n) {
  return run_steps(s, a, b, bcm, miss, omega, t0, n, true, nullptr);
}

int xlbhip_run_any(xlbhip_stepper* s, xlbhip_field* a, xlbhip_field* b, const xlbhip_field* bcm, const xlbhip_field* miss, double omega,
                   int64_t t0, int64_t n, int* result_in_b) {
  XLB_REQUIRE(result_in_b, "result_in_b is null");
  return run_steps(s, a, b, bcm, miss, omega, t0, n, false, result_in_b);
}

int xlbhip_step2_eligible(xlbhip_stepper* s, const xlbhip_field* src, xlbhip_field* dst, const xlbhip_field* bcm, const xlbhip_field* miss) {
  if (check_step_fields(s, src, dst, bcm, miss)) return 0;
  return can_fuse2(s, src, bcm).fuse ? 1 : 0;
}

int xlbhip_step2(xlbhip_stepper* s, const xlbhip_field* src, xlbhip_field* dst, const xlbhip_field* bcm, const xlbhip_field* miss,
                 double omega, int64_t timestep) {
  if (int rc = check_step_fields(s, src, dst, bcm, miss)) return rc;
  if (int rc = s->prof.require_staged(timestep, 2)) return rc;
  const Fuse2 how = can_fuse2(s, src, bcm);
  XLB_REQUIRE(how.fuse, "this stepper / field layout has no two-step kernel (see xlbhip_step2_eligible)");
  if (int rc = prepare_fuse2(s, bcm, miss)) return rc;
  return step_twice(s, how, src, dst, bcm, miss, omega, timestep);
}

int xlbhip_step2_plan(xlbhip_stepper* s, const xlbhip_field* src, xlbhip_field* dst, const xlbhip_field* bcm, const xlbhip_field* miss,
                      int32_t* out, int64_t capacity, int64_t* n_words) {
  XLB_REQUIRE(n_words && (out || capacity == 0), "null argument");
  if (int rc = check_step_fields(s, src, dst, bcm, miss)) return rc;
  const Fuse2 how = can_fuse2(s, src, bcm);
  XLB_REQUIRE(how.fuse, "this stepper / field layout has no two-step kernel (see xlbhip_step2_eligible)");
  if (int rc = prepare_fuse2(s, bcm, miss)) return rc;
  Step2Report rep;
  if (int rc = step_twice(s, how, src, dst, bcm, miss, 1.0, 0, &rep)) return rc;
  *n_words = (int64_t)rep.words.size();
  if (capacity >= *n_words) std::copy(rep.words.begin(), rep.words.end(), out);
  return 0;
}

int xlbhip_run_timed(xlbhip_stepper* s, xlbhip_field* a, xlbhip_field* b, const xlbhip_field* bcm, const xlbhip_field* miss, double omega,
                     int64_t t0, int64_t n, float* ms, int* result_in_b) {
  XLB_REQUIRE(s && ms, "null argument");
  xlbhip_ctx* c = s->ctx;
  XLB_HIP(hipEventRecord(c->ev_a, c->stream));
  // (result_in_b == NULL: xlbhip_run's fixed placement; else as xlbhip_run_any)
  if (int rc = run_steps(s, a, b, bcm, miss, omega, t0, n, result_in_b == nullptr, result_in_b)) return rc;
  XLB_HIP(hipEventRecord(c->ev_b, c->stream));
  XLB_HIP(hipEventSynchronize(c->ev_b));
  XLB_HIP(hipEventElapsedTime(ms, c->ev_a, c->ev_b));
  return 0;
}

}  // extern "C"
