// The kind predicates of the boundary conditions, for host and device: every rule "which kinds ..." has its one definition here.
// Needs the public header alone; cell.hpp includes it for the kernels, bc_tables.hpp for the descriptor parser.
#pragma once
#include "../../include/xlbhip.h"

namespace xlb {

constexpr bool bc_is_known(int k) { return k >= XLBHIP_BC_EQUILIBRIUM && k <= XLBHIP_BC_HALFWAY_BB_PROFILE; }
constexpr bool bc_is_zouhe_family(int k) { return k >= XLBHIP_BC_ZOUHE_VELOCITY && k <= XLBHIP_BC_REGULARIZED_PRESSURE; }
constexpr bool bc_is_hybrid(int k) { return k >= XLBHIP_BC_HYBRID_BB_REGULARIZED && k <= XLBHIP_BC_HYBRID_NEQ_REGULARIZED; }
constexpr bool bc_is_extended(int k) { return k >= XLBHIP_BC_ZOUHE_VELOCITY; }  // the extended step-kernel variant's: all but the four basic kinds
constexpr bool bc_reads_missing(int k) { return k == XLBHIP_BC_HALFWAY_BB || bc_is_extended(k); }
constexpr bool bc_is_edge_kind(int k) { return bc_is_extended(k) || k == XLBHIP_BC_DO_NOTHING; }  // not evaluated by the two-step kernel itself
constexpr bool bc_has_wall_table(int k) { return bc_is_hybrid(k) || k == XLBHIP_BC_HALFWAY_BB_PROFILE; }  // cells may sit in the sparse tables

}  // namespace xlb
