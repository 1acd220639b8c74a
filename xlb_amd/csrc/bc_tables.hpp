// From the boundary-condition descriptors of a stepper to the host image of its tables: kinds and values by bc id, the packed words
// the kernels look up in their arguments, and the flags the launches ask.  The one parser of the fluid stepper, the scalar-transport
// stepper and the adjoint stepper; each states the kinds it takes through a predicate.  Host arithmetic only — no HIP type or call, so
// that tests/test_bc_tables.py compiles it for the CPU; the device buffers and the upload are the owner's (stepper_tables.hpp).
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "bc_kinds.hpp"

namespace xlb {

// the packed words and the flags: what the host image and the device owner both hold
struct BcWords {
  int n_bc = 0;
  bool needs_missing = false;
  bool extended_bcs = false;
  bool has_outflow = false;     // ExtrapolationOutflowBC present: k_outflow_aux runs after every step
  bool has_edge_kinds = false;  // kinds the two-step kernel does not evaluate itself: Zou-He family, outflow, do-nothing
  unsigned long long ids_packed = 0;  // the first 8 bc ids, one per byte
  unsigned kinds_packed = 0;          // their kinds, one per nibble
  unsigned moving_mask = 0;           // slots (first 8 BCs) whose halfway wall has a non-zero moving-wall term
};

struct BcImage : BcWords {
  std::vector<uint8_t> kind = std::vector<uint8_t>(256, 0);        // [256] XLBHIP_BC_*, 0 = no such id
  std::vector<double> vals = std::vector<double>(256 * 27, 0.0);  // [256][27], the first q of a row used
};

// ---- which kinds a stepper takes ----
// the fluid stepper: nullptr, or the text of its refusal (a format taking the kind); q = 9 is the 2-D lattice
inline const char* bc_stepper_refusal(int q, int kind) {
  if (!bc_is_known(kind)) return "unknown bc kind %d";
  if (bc_is_hybrid(kind) && q == 9) return "This BC is not implemented in 2D!";  // bc_hybrid.py:119-120
  return nullptr;
}
constexpr bool bc_is_basic(int k) { return k >= XLBHIP_BC_EQUILIBRIUM && k <= XLBHIP_BC_DO_NOTHING; }
// the coupled fluid + scalar step: no HybridBC, no profile walls
constexpr bool bc_scalar_accepts(int k) { return bc_is_basic(k) || bc_is_zouhe_family(k) || k == XLBHIP_BC_EXTRAPOLATION_OUTFLOW; }
// the adjoint step: equilibrium, halfway and fullway bounce-back and do-nothing
constexpr bool bc_adjoint_accepts(int k) { return bc_is_basic(k); }
// the Shan-Chen step: walls only, halfway (constant wall velocity or none) and fullway bounce-back — the missing directions of every
// other kind have no agreed neighbour pseudopotential
constexpr bool bc_multiphase_accepts(int k) { return k == XLBHIP_BC_HALFWAY_BB || k == XLBHIP_BC_FULLWAY_BB; }

// The image of `bcs` for a lattice of q populations.  refusal(kind): nullptr for a kind the caller takes, else the format of its message
// (one %d, the kind).  Returns the error text; empty: `out` is complete.
template <class Refusal>
std::string bc_parse(int q, int n_bc, const xlbhip_bc_desc* bcs, Refusal&& refusal, BcImage& out) {
  const auto fail = [](const char* fmt, int arg) {
    char msg[200];
    std::snprintf(msg, sizeof msg, fmt, arg);
    return std::string(msg);
  };
  out = BcImage();
  out.n_bc = n_bc;
  for (int i = 0; i < n_bc; ++i) {
    const xlbhip_bc_desc& b = bcs[i];
    if (b.id < 1 || b.id > 255) return fail("bc id %d out of range 1..255", b.id);
    if (const char* fmt = refusal(b.kind)) return fail(fmt, b.kind);
    if (out.kind[b.id] != 0) return fail("bc id %d used twice", b.id);
    out.kind[b.id] = (uint8_t)b.kind;
    for (int l = 0; l < q; ++l) out.vals[b.id * 27 + l] = b.values[l];
    if (b.kind == XLBHIP_BC_EXTRAPOLATION_OUTFLOW) out.has_outflow = true;
    if (bc_is_edge_kind(b.kind)) out.has_edge_kinds = true;
    if (bc_is_extended(b.kind)) out.extended_bcs = true;
    if (bc_reads_missing(b.kind)) out.needs_missing = true;
  }
  for (int i = 0; i < n_bc && i < 8; ++i) {
    out.ids_packed |= (unsigned long long)(bcs[i].id & 0xff) << (8 * i);
    out.kinds_packed |= (unsigned)(bcs[i].kind & 0xf) << (4 * i);
    if (bcs[i].kind == XLBHIP_BC_HALFWAY_BB)
      for (int l = 0; l < q; ++l)
        if (bcs[i].values[l] != 0.0) out.moving_mask |= 1u << i;
  }
  return std::string();
}

}  // namespace xlb
