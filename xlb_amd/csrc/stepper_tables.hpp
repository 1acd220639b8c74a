// What the native objects that launch row kernels share (stepper.hip, scalar.hip, adjoint.hip, multiphase.hip).  The device side of
// their boundary conditions: BcTables owns the uploaded tables and keeps the packed words, the flags and the host kinds of the image
// they came from (bc_tables.hpp parses the descriptors); bc_launch fills the part of a StepLaunch they fill alike; outflow_aux is the
// pass after a step.  Their life: RowStepper is what each carries, create_row_stepper the shared part of its create, destroy_drained
// its destroy, run_alternating its run loop (ibm.hip takes the last two as well), check_row_fields what a step asks of its fields.
#pragma once
#include <initializer_list>
#include <memory>
#include <string>

#include "api_internal.hpp"
#include "bc_tables.hpp"
#include "step_launch.hpp"

namespace xlb {

// The boundary conditions of a stepper: their kinds and values by id, and what the kernels look up in their arguments
struct BcTables : BcWords {
  std::vector<uint8_t> kind_host = std::vector<uint8_t>(256, 0);  // tab_kind's contents
  DeviceBuf tab_kind;                                             // uint8 [256]
  DeviceBuf tab_values;                                           // [256][27] compute dtype

  // the caller's device is current
  int upload(int cdt, const BcImage& image) {
    static_cast<BcWords&>(*this) = image;
    kind_host = image.kind;
    if (int rc = upload_bytes(kind_host.data(), 256, tab_kind)) return rc;
    return upload_values(cdt, image.vals, tab_values);
  }
};

// the image of a stepper's descriptors, or the parser's / the caller's refusal as the library's error (refusal: bc_tables.hpp, bc_parse)
template <class Refusal>
static int bc_image(int lattice, int n_bc, const xlbhip_bc_desc* bcs, Refusal&& refusal, BcImage& out) {
  const std::string err = bc_parse(lattice_q(lattice), n_bc, bcs, refusal, out);
  XLB_REQUIRE(err.empty(), "%s", err.c_str());
  return 0;
}

// What the four native objects that launch row kernels carry (the fluid stepper, scalar transport, the adjoint, the multiphase step)
struct RowStepper {
  xlbhip_ctx* ctx = nullptr;
  int lattice = 0, cdt = 0, sdt = 0;
  BcTables bc;
};

// The shared part of their xlbhip_*_create: the argument checks, the image of the descriptors (`refusal`: bc_image), the object on
// the context's device with its boundary tables uploaded, then own(object) for the caller's own tables, and only then *out.
// policy_subject: in whose name any policy but the three of by_three_policies is refused, or nullptr (the caller checked its dtypes).
template <class Obj, class Refusal, class Own>
static int create_row_stepper(xlbhip_ctx* c, int lattice, int cdt, int sdt, int n_bc, const xlbhip_bc_desc* bcs, const char* policy_subject,
                              Refusal&& refusal, Own&& own, Obj** out) {
  XLB_REQUIRE(c && out, "null argument");
  XLB_REQUIRE(lattice_q(lattice) > 0, "unknown lattice %d", lattice);
  if (policy_subject)  // (the launchers' dispatcher with nothing to launch: its refusal is the check, in the launchers' words)
    if (int rc = by_three_policies(policy_subject, cdt, sdt, [](auto, auto) { return 0; })) return rc;
  XLB_REQUIRE(n_bc == 0 || bcs, "null bc list");
  BcImage image;
  if (int rc = bc_image(lattice, n_bc, bcs, refusal, image)) return rc;
  XLB_HIP(hipSetDevice(c->device));
  auto s = std::make_unique<Obj>();  // (a failure below releases it and the tables uploaded so far)
  s->ctx = c;
  s->lattice = lattice;
  s->cdt = cdt;
  s->sdt = sdt;
  if (int rc = s->bc.upload(cdt, image)) return rc;
  if (int rc = own(*s)) return rc;
  *out = s.release();
  return 0;
}

// xlbhip_*_destroy of an object whose launches run on its context's compute stream: they may still read what it owns, so the stream
// drains first; then release() for what has to go before the members do, then the object
template <class Obj, class Release>
static int destroy_drained(Obj* s, Release&& release) {
  if (!s) return 0;
  (void)hipSetDevice(s->ctx->device);
  (void)hipStreamSynchronize(s->ctx->stream);
  release();
  delete s;
  return 0;
}
template <class Obj>
static int destroy_drained(Obj* s) {
  return destroy_drained(s, [] {});
}

// xlbhip_*_run of a double-buffered step: step(i, odd) for i = 0 .. n_steps - 1, where an even step goes a -> b and an odd one
// b -> a; *result_in_b says where the last one left the result
template <class Step>
static int run_alternating(int64_t n_steps, int* result_in_b, Step&& step) {
  for (int64_t i = 0; i < n_steps; ++i)
    if (int rc = step(i, (i & 1) != 0)) return rc;
  *result_in_b = (int)(n_steps & 1);
  return 0;
}

// What a single-rank row-kernel step asks of a family of its fields (null entries are skipped): `card` planes in the store dtype,
// no ghost planes, one grid and, where the kernel takes one stride for all of them (one_stride), one plane stride
static int check_row_fields(const char* who, const char* fields_name, int card, int sdt, std::initializer_list<const xlbhip_field*> fields, bool one_stride) {
  const xlbhip_field* first = nullptr;
  for (const xlbhip_field* f : fields) {
    if (!f) continue;
    if (!first) first = f;
    XLB_REQUIRE(f->card == card, "%s: %s must have cardinality %d", who, fields_name, card);
    XLB_REQUIRE(f->dtype == sdt, "%s: %s must have the store dtype %d", who, fields_name, sdt);
    XLB_REQUIRE(f->halo == 0, "%s: fields without ghost planes only (single rank)", who);
    XLB_REQUIRE(same_grid(f, first), "%s: the fields of a step must share one grid", who);
    XLB_REQUIRE(!one_stride || f->plane_stride == first->plane_stride, "%s: the layouts of the %s differ", who, fields_name);
  }
  return 0;
}

// What every stepper's launch takes from (context, tables, dtypes, masks, grid): the tables, the masks, the extent and ghost planes of
// `grid_of`, all of x, the dtypes and the compute stream.  The fields, plane_stride, omega, has_bc and the options are the caller's.
static StepLaunch bc_launch(const xlbhip_ctx* c, const BcTables& bc, int cdt, int sdt, const xlbhip_field* bcm, const xlbhip_field* miss,
                            const xlbhip_field* grid_of) {
  StepLaunch p = {};
  p.bc = (bc.n_bc > 0 && bcm) ? static_cast<const uint8_t*>(bcm->data) : nullptr;
  p.miss = miss ? static_cast<const uint32_t*>(miss->data) : nullptr;
  p.tab_kind = bc.tab_kind.get<uint8_t>();
  p.tab_values = bc.tab_values.get();
  p.ids_packed = bc.ids_packed;
  p.kinds_packed = bc.kinds_packed;
  p.n_bc = bc.n_bc;
  p.nx = grid_of->nx;
  p.ny = grid_of->ny;
  p.nz = grid_of->nz;
  p.halo = grid_of->halo;
  p.x_begin = 0;
  p.x_count = grid_of->nx;
  p.compute_dtype = cdt;
  p.store_dtype = sdt;
  p.stream = c->stream;
  return p;
}

// the sparse per-cell tables a stepper may keep beside its boundary tables (the fluid stepper's profile and wall-distance tables)
struct CellTables {
  const uint32_t* prof_keys = nullptr;
  const void* prof_vals = nullptr;  // compute dtype [n_prof][3]
  int n_prof = 0;
  const uint32_t* dist_keys = nullptr;
  const float* dist_vals = nullptr;
  int n_dist = 0;
};

// the tables as the whole-field kernels take them
template <class T>
static BcView<T> bc_view(const BcTables& bc, const CellTables& ct) {
  return {bc.tab_kind.get<uint8_t>(), bc.tab_values.get<const T>(), ct.prof_keys, static_cast<const T*>(ct.prof_vals), ct.n_prof, ct.dist_keys, ct.dist_vals,
          ct.n_dist};
}

// assemble_auxiliary_data of the ExtrapolationOutflowBC cells after a step src -> dst (nse_stepper.py:270-272).  A template only so
// that the units that call it (stepper.hip, scalar.hip), and no other that includes this file, carry the k_outflow_aux kernels.
template <class Tables>
static int outflow_aux(const xlbhip_ctx* c, int lattice, int cdt, const Tables& bc, const CellTables& ct, const xlbhip_field* src, xlbhip_field* dst,
                       const xlbhip_field* bcm, const xlbhip_field* miss) {
  if (!bc.has_outflow) return 0;
  const size_t n = dst->cells();
  return by_lattice(lattice, [&](auto L) {
    return by_compute(cdt, [&](auto T) {
      using TT = decltype(T);
      hipLaunchKernelGGL((k_outflow_aux<decltype(L), TT>), blocks_for(n), BC_BLOCK, 0, c->stream, view(src), view(dst), view(bcm), view(miss), dims(dst),
                         bc_view<TT>(bc, ct));
      XLB_HIP(hipGetLastError());
      return 0;
    });
  });
}

}  // namespace xlb
