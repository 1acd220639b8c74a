// The device side of a stepper's boundary conditions, shared by stepper.hip, scalar.hip and adjoint.hip: BcTables owns the uploaded
// tables and keeps the packed words, the flags and the host kinds of the image they came from (bc_tables.hpp parses the descriptors);
// bc_launch fills the part of a StepLaunch the three steppers fill alike; outflow_aux is the pass after a step.
#pragma once
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
