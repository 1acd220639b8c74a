// Type-erased launch descriptor + the per-(lattice, collision) dispatcher that each
// step_*.hip translation unit instantiates.  What every launcher of a StepLaunch shares (this file's, scalar_launch.hpp,
// adjoint_launch.hpp, multiphase_launch.hpp; step2_launch.hpp takes step_args) is defined once here: step_args, the one copy
// StepLaunch -> StepArgs; by_three_policies, the precision policies of every kernel family but the plain ones; launch_rows, the launch
// of a row kernel on a block shape of launch_shape.hpp; launch_for_lattice, the choice among a family's three per-lattice units.
#pragma once
#include "common.hpp"
#include "launch_shape.hpp"
#include "step_kernel.hpp"

namespace xlb {

struct StepLaunch {
  const void* src;
  void* dst;
  const uint8_t* bc;
  const uint32_t* miss;
  const uint8_t* tab_kind;
  const void* tab_values;  // compute dtype [256][27]
  const uint32_t* prof_keys;  // profile table of Zou-He / Regularized BCs (sorted storage cell indices), or nullptr
  const void* prof_vals;      // compute dtype [n_prof][3]
  int n_prof;
  const uint32_t* dist_keys;  // wall-distance table of HybridBC cells (sorted storage cell indices), or nullptr
  const float* dist_vals;     // [n_dist][q]
  int n_dist;
  unsigned long long ids_packed;
  unsigned kinds_packed;
  int n_bc;
  size_t plane_stride;
  int nx, ny, nz, halo;
  int x_begin, x_count;
  double omega;
  double force[3];
  double smag_cs;
  int compute_dtype, store_dtype;
  int vec;     // requested cells per thread (1, 2, 4); must divide nz
  int has_bc;  // 0: no BCs; 1: basic kinds; 2: + Zou-He / Regularized
  int flags;   // bit 0: non-temporal stores
  int block_threads;  // 0 = default (256)
  int block_tz;       // threads along z per block, 0 = as many as fit
  int xcd_swizzle;
  int fast_math;  // 1: tolerance-graded fast collision where one is built (fp64 KBC: cell.hpp kbc_fast); 0: bit-exact builds only
  hipStream_t stream;
};

// the strips mode of a two-step launch; the values are those of k_step2's STRIPS template parameter (documented there: step2_kernel.hpp)
enum class Strips : int { none = 0, write = 2, read_write = 3, rowmap = 4 };

// A launch of the two-steps-per-pass kernel: what a single step needs plus the two-step kernel's own geometry and tables
struct Step2Launch : StepLaunch {
  const uint32_t* meta = nullptr;        // id | missing << 8 per cell, or nullptr
  const uint32_t* tile_order = nullptr;  // block -> tile, or nullptr
  const uint8_t* clean = nullptr;        // per-block "no boundary cells" flags for THIS launch geometry, or nullptr
  const void* strips_src = nullptr;      // strip buffers of the source / destination field (storage plane 0), or nullptr
  void* strips_dst = nullptr;
  Strips strips = Strips::none;
  int x_segments = 1;
  int x_cap = 0;                 // thin first / last segment (planes), 0 = uniform cuts
  int tile_oy = 0, tile_oz = 0;  // periodic origin shift of the tiling (0 .. tile - 1)
  int tile_ty = 0, tile_tz = 0;  // tile of the (y, z) plane a block owns
  int fast_bgk = 0;              // 1 = tolerance-graded fast BGK body (opt-in)
};

// which (T, S, VEC) combinations exist: fp32 compute -> VEC in {1, 2, 4}; fp64 compute -> {1, 2}
inline int pick_vec(int compute_dtype, int nz, int requested, int collision) {
  // Measured on MI355X: one cell per thread wins everywhere — D3Q19 fp32 at 512^3 (profiles/r01/sweeps.md: 44-60 VGPRs ->
  // 8 waves/SIMD; 75.9 % of the HBM peak vs 74.5 % for VEC=2 and 72.9 % for VEC=4) and fp64 KBC at 384^3
  // (profiles/r02/d3q27_kbc_384_sweep.txt: 122 VGPRs / 4 waves vs 164 / 3; 0.684 vs 0.618 of peak), so "auto" (0) means 1.
  // Wider variants stay selectable through the "vec" option.
  const int vmax = (compute_dtype == XLBHIP_F32) ? 4 : 2;
  (void)collision;
  int v = requested > 0 ? requested : 1;
  if (v > vmax) v = vmax;
  if (v == 3) v = 2;
  if (nz % v != 0) v = 1;
  return v;
}

// The kernel arguments every launcher of a StepLaunch fills alike (launch_typed, launch_scalar_typed, launch_adjoint_typed, launch2f):
// everything else starts as zero / nullptr, and each launcher sets what is its own.  vec: cells per thread along z.
template <class T, class S>
StepArgs<T, S> step_args(const StepLaunch& p, int vec) {
  StepArgs<T, S> a = {};
  a.src = static_cast<const S*>(p.src);
  a.dst = static_cast<S*>(p.dst);
  a.bc = p.bc;
  a.miss = p.miss;
  a.bc_kind = p.tab_kind;
  a.bc_values = static_cast<const T*>(p.tab_values);
  a.ids_packed = p.ids_packed;
  a.kinds_packed = p.kinds_packed;
  a.n_bc = p.n_bc;
  a.plane_stride = p.plane_stride;
  a.nx = p.nx;
  a.ny = p.ny;
  a.nz = p.nz;
  a.halo = p.halo;
  a.x_begin = p.x_begin;
  a.x_count = p.x_count;
  a.nzq = p.nz / vec;
  a.omega = static_cast<T>(p.omega);
  a.extra.smag_cs = p.smag_cs;
  return a;
}

// The precision policies every kernel family but the plain BGK / KBC steps is built for (to bound build time): FP32FP32, FP64FP64
// and FP64FP32
inline bool three_policies(int compute_dtype, int store_dtype) {
  return (compute_dtype == XLBHIP_F32 && store_dtype == XLBHIP_F32) ||
         (compute_dtype == XLBHIP_F64 && (store_dtype == XLBHIP_F64 || store_dtype == XLBHIP_F32));
}

// f(T{}, S{}) with (T, S) the compute and store types of one of the three policies; any other pair is refused in the name of
// `subject` ("scalar transport is", "... collisions are")
template <class F>
int by_three_policies(const char* subject, int compute_dtype, int store_dtype, F&& f) {
  XLB_REQUIRE(three_policies(compute_dtype, store_dtype), "%s built for FP32FP32, FP64FP64 and FP64FP32 only (got compute=%d store=%d)", subject,
              compute_dtype, store_dtype);
  if (store_dtype == XLBHIP_F64) return f(double{}, double{});
  return compute_dtype == XLBHIP_F64 ? f(double{}, float{}) : f(float{}, float{});
}

// One launch of a row kernel (k_step, k_step_scalar, k_adjoint_step, the multiphase kernels) on `stream`: block and grid of `sh`,
// with the grid's y and z inside what the device takes
template <class Args>
int launch_rows(void (*kernel)(Args), const RowBlockShape& sh, hipStream_t stream, const Args& a) {
  const dim3 block(sh.tz, sh.ty, 1), grid(sh.gx, sh.gy, sh.gz);
  XLB_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "grid too large: ny/ty=%u x_count=%u", grid.y, grid.z);
  hipLaunchKernelGGL(kernel, grid, block, 0, stream, a);
  XLB_HIP(hipGetLastError());
  return 0;
}

// The entry point of `lattice` among the three of a kernel family (each is defined in a translation unit of its own), called with `a`
template <class Entry, class... A>
int launch_for_lattice(int lattice, Entry* d2q9, Entry* d3q19, Entry* d3q27, const A&... a) {
  return (lattice == XLBHIP_D2Q9 ? d2q9 : lattice == XLBHIP_D3Q19 ? d3q19 : d3q27)(a...);
}

template <class L, class T, class S, int VEC, int COLL, int HASBC, int FLAGS>
int launch_typed(const StepLaunch& p) {
  StepArgs<T, S> a = step_args<T, S>(p, VEC);
  a.prof_keys = p.prof_keys;
  a.prof_vals = static_cast<const T*>(p.prof_vals);
  a.n_prof = p.n_prof;
  a.dist_keys = p.dist_keys;
  a.dist_vals = p.dist_vals;
  a.n_dist = p.n_dist;
  a.extra.force[0] = p.force[0];
  a.extra.force[1] = p.force[1];
  a.extra.force[2] = p.force[2];
  const int threads = p.block_threads > 0 ? p.block_threads : 256;
  const RowBlockShape sh = row_block_shape(a.nzq, p.ny, p.x_count, threads, p.block_tz);
  XLB_REQUIRE(threads <= (VEC == 1 ? XLB_LB1 : 256), "block_threads %d exceeds the kernel's launch bound", threads);
  a.xcd_swizzle = (p.xcd_swizzle && sh.gx > 1 && sh.gy % 8 == 0) ? 1 : 0;
  return launch_rows(k_step<L, T, S, VEC, COLL, HASBC, FLAGS>, sh, p.stream, a);
}

template <class L, class T, class S, int VEC, int COLL, int HASBC>
int launch_flags(const StepLaunch& p) {
#ifdef XLB_TUNE_VARIANTS
  switch (p.flags & 7) {
    case 0: return launch_typed<L, T, S, VEC, COLL, HASBC, 0>(p);
    case 1: return launch_typed<L, T, S, VEC, COLL, HASBC, 1>(p);
    case 3: return launch_typed<L, T, S, VEC, COLL, HASBC, 3>(p);
    case 7: return launch_typed<L, T, S, VEC, COLL, HASBC, 7>(p);
    default: XLB_FAIL("flag combination %d not instantiated", p.flags);
  }
#else
  return (p.flags & 2) ? launch_typed<L, T, S, VEC, COLL, HASBC, 3>(p) : launch_typed<L, T, S, VEC, COLL, HASBC, 1>(p);
#endif
}

template <class L, class T, class S, int VEC, int COLL>
int launch_vec(const StepLaunch& p) {
  if (p.has_bc == 2) return launch_flags<L, T, S, VEC, COLL, 2>(p);
  if (p.has_bc == 1) return launch_flags<L, T, S, VEC, COLL, 1>(p);
  return launch_flags<L, T, S, VEC, COLL, 0>(p);
}

template <class L, class T, class S, int COLL>
int launch_policy(const StepLaunch& p) {
  const int v = pick_vec(p.compute_dtype, p.nz, p.vec, COLL & 3);
  if constexpr (sizeof(T) == 4) {
    if (v == 4) return launch_vec<L, T, S, 4, COLL>(p);
  }
  if (v == 2) return launch_vec<L, T, S, 2, COLL>(p);
  return launch_vec<L, T, S, 1, COLL>(p);
}

template <class L, int COLL>
int launch_step(const StepLaunch& p) {
  const int c = p.compute_dtype, s = p.store_dtype;
  if (c == XLBHIP_F32 && s == XLBHIP_F32) return launch_policy<L, float, float, COLL>(p);
  if (c == XLBHIP_F32 && s == XLBHIP_F16) return launch_policy<L, float, _Float16, COLL>(p);
  if (c == XLBHIP_F64 && s == XLBHIP_F64) return launch_policy<L, double, double, COLL>(p);
  if (c == XLBHIP_F64 && s == XLBHIP_F32) return launch_policy<L, double, float, COLL>(p);
  if (c == XLBHIP_F64 && s == XLBHIP_F16) return launch_policy<L, double, _Float16, COLL>(p);
  XLB_FAIL("unsupported precision policy compute=%d store=%d", c, s);
}

// Extended and regularised collisions: three policies only, to bound build time
template <class L, int COLL>
int launch_step_ext(const StepLaunch& p) {
  return by_three_policies("SmagorinskyLESBGK / forced collisions are", p.compute_dtype, p.store_dtype,
                           [&](auto T, auto S) { return launch_policy<L, decltype(T), decltype(S), COLL>(p); });
}

// The variants of a step_<lattice>_ext.hip unit.  coll: XLBHIP_SMAGORINSKY_LES_BGK [| COLL_FORCED], or XLBHIP_BGK / XLBHIP_KBC |
// COLL_FORCED (Smagorinsky LES, exact-difference forcing: SURVEY.md section 8f rank 3)
template <class L>
int launch_step_ext_lattice(const StepLaunch& p, int coll) {
  switch (coll) {
    case XLBHIP_SMAGORINSKY_LES_BGK: return launch_step_ext<L, XLBHIP_SMAGORINSKY_LES_BGK>(p);
    case XLBHIP_SMAGORINSKY_LES_BGK | COLL_FORCED: return launch_step_ext<L, XLBHIP_SMAGORINSKY_LES_BGK | COLL_FORCED>(p);
    case XLBHIP_BGK | COLL_FORCED: return launch_step_ext<L, XLBHIP_BGK | COLL_FORCED>(p);
  }
  if constexpr (L::ID != XLBHIP_D3Q19) {
    if (coll == (XLBHIP_KBC | COLL_FORCED)) return launch_step_ext<L, XLBHIP_KBC | COLL_FORCED>(p);
  }
  XLB_FAIL("collision variant %d not built for D%dQ%d", coll, L::D, L::Q);
}

// The variants of a step_<lattice>_reg.hip unit.  coll: COLL_REGULARIZED [| COLL_RECURSIVE] [| COLL_FORCED] (cell.hpp regularized:
// projected and recursive, each with and without exact-difference forcing)
template <class L>
int launch_step_reg_lattice(const StepLaunch& p, int coll) {
  constexpr int RR = COLL_REGULARIZED | COLL_RECURSIVE;
  switch (coll) {
    case COLL_REGULARIZED: return launch_step_ext<L, COLL_REGULARIZED>(p);
    case COLL_REGULARIZED | COLL_FORCED: return launch_step_ext<L, COLL_REGULARIZED | COLL_FORCED>(p);
    case RR: return launch_step_ext<L, RR>(p);
    case RR | COLL_FORCED: return launch_step_ext<L, RR | COLL_FORCED>(p);
  }
  XLB_FAIL("collision variant %d not built for D%dQ%d", coll, L::D, L::Q);
}

// fp64-compute policies only (the fast KBC variant: cell.hpp kbc_fast)
template <class L, int COLL>
int launch_step_f64(const StepLaunch& p) {
  const int c = p.compute_dtype, s = p.store_dtype;
  // (a store type narrower than the compute type: the gamma reduction of the fast KBC collision runs in fp32, cell.hpp COLL_G32)
  constexpr int NARROW = COLL | (XLB_KBC_GAMMA32 ? COLL_G32 : 0);
  if (c == XLBHIP_F64 && s == XLBHIP_F64) return launch_policy<L, double, double, COLL>(p);
  if (c == XLBHIP_F64 && s == XLBHIP_F32) return launch_policy<L, double, float, NARROW>(p);
  if (c == XLBHIP_F64 && s == XLBHIP_F16) return launch_policy<L, double, _Float16, NARROW>(p);
  XLB_FAIL("fast fp64 variant asked for compute=%d store=%d", c, s);
}

// defined one per translation unit (step_<lattice>_<collision>.hip)
int launch_step_d3q27_kbc_fast64(const StepLaunch& p);
// two steps per pass (step2_kernel.hpp): f(t) in src -> f(t+2) in dst
int launch_step2_d3q19_bgk(const Step2Launch& p);
int launch_step2_d3q19_bgk_strips(const Step2Launch& p);  // p.strips != Strips::none (step2_d3q19_strips.hip)
int launch_step2_d3q27_bgk(const Step2Launch& p);
int launch_step2_d3q27_kbc(const Step2Launch& p);
int step2_build_clean(const Step2Launch& p, uint8_t* out);
int step2_items(const Step2Launch& p);
int step2_report_items(const Step2Launch& p, int32_t* out, int* eff_segments, int* eff_cap);  // out: device memory, 3 words per item
// (the definitions are launch_step_ext_lattice<L> and launch_step_reg_lattice<L>)
int launch_step_d2q9_ext(const StepLaunch& p, int coll);
int launch_step_d3q19_ext(const StepLaunch& p, int coll);
int launch_step_d3q27_ext(const StepLaunch& p, int coll);
int launch_step_d2q9_reg(const StepLaunch& p, int coll);
int launch_step_d3q19_reg(const StepLaunch& p, int coll);
int launch_step_d3q27_reg(const StepLaunch& p, int coll);
int launch_step_d2q9_bgk(const StepLaunch& p);
int launch_step_d2q9_kbc(const StepLaunch& p);
int launch_step_d3q19_bgk(const StepLaunch& p);
int launch_step_d3q27_bgk(const StepLaunch& p);
int launch_step_d3q27_kbc(const StepLaunch& p);

}  // namespace xlb
