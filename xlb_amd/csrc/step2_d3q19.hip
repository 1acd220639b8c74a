// Instantiates the two-steps-per-pass kernel (step2_kernel.hpp) for D3Q19 / BGK / FP32FP32.
#include "step2_launch.hpp"

namespace xlb {

// f(t) in p.src -> f(t+2) in p.dst on (8 x 64) tiles (step2_plan.hpp: step2_tile)
int launch_step2_d3q19_bgk(const Step2Launch& p) {
  XLB_REQUIRE(p.tile_ty == 8 && p.tile_tz == 64, "two-step kernel: only the (8 x 64) tile is built");
  if (p.halo) return p.has_bc ? launch2<D3Q19, 1, 8, 64, true>(p) : launch2<D3Q19, 0, 8, 64, true>(p);
  return p.has_bc ? launch2<D3Q19, 1, 8, 64, false>(p) : launch2<D3Q19, 0, 8, 64, false>(p);
}

// per-block "no boundary cell in this work item" flags for the launch geometry of p (n = tiles x effective segments bytes)
int step2_build_clean(const Step2Launch& p, uint8_t* out) {
  XLB_REQUIRE(p.meta && out && p.tile_ty == 8 && (p.tile_tz == 64 || (p.tile_tz == 48 && p.halo == 0)), "clean flags: (8 x 64) / (8 x 48) tiles with meta words only");
  const size_t ghost = (size_t)p.halo * p.ny * p.nz;
  const unsigned tiles = (unsigned)(p.ny / 8) * (unsigned)(p.nz / p.tile_tz);
  const int segs = step2_eff_segments(p), swz = step2_eff_swizzle(p, tiles);
  if (p.tile_tz == 48)
    hipLaunchKernelGGL((k_step2_clean<8, 48, false>), dim3(tiles * (unsigned)segs), dim3(256), 0, p.stream, p.meta, p.tile_order, swz, segs, step2_eff_cap(p), p.x_begin,
                       p.x_count, p.nx, p.ny, p.nz, p.tile_oy, p.tile_oz, out);
  else if (p.halo)
    hipLaunchKernelGGL((k_step2_clean<8, 64, true>), dim3(tiles * (unsigned)segs), dim3(256), 0, p.stream, p.meta + ghost, p.tile_order, swz, segs, step2_eff_cap(p), p.x_begin,
                       p.x_count, p.nx, p.ny, p.nz, p.tile_oy, p.tile_oz, out);
  else
    hipLaunchKernelGGL((k_step2_clean<8, 64, false>), dim3(tiles * (unsigned)segs), dim3(256), 0, p.stream, p.meta, p.tile_order, swz, segs, step2_eff_cap(p), p.x_begin,
                       p.x_count, p.nx, p.ny, p.nz, p.tile_oy, p.tile_oz, out);
  XLB_HIP(hipGetLastError());
  return 0;
}

// The work item of every block of a launch, for the plan report (stepper.hip: Step2Report): out[3 b ...] = tile, x_lo, x_hi of block b,
// by the block -> (tile, x segment) mapping of k_step2 and k_step2_clean (step2_kernel.hpp) with the device's own step2_seg_range.
template <int TY, int TZ>
__global__ void k_step2_items(const uint32_t* tile_order, int xcd_swizzle, int x_segments, int x_cap, int x_begin, int x_count, int ny, int nz, int n_items,
                              int32_t* out) {
  const unsigned b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= (unsigned)n_items) return;
  const unsigned tiles_z = (unsigned)nz / TZ, tiles_y = (unsigned)ny / TY, n_tiles = tiles_y * tiles_z;
  const unsigned seg = b / n_tiles, slot_in_seg = b % n_tiles;
  unsigned tile = slot_in_seg;
  if (tile_order) {
    tile = tile_order[slot_in_seg];
  } else if (xcd_swizzle) {
    const unsigned per_xcd = n_tiles / 8u;
    tile = (slot_in_seg % 8u) * per_xcd + slot_in_seg / 8u;
  }
  const int n_seg = x_segments > 0 ? x_segments : 1;
  int x_lo, x_hi;
  step2_seg_range(x_begin, x_count, n_seg, x_cap, (int)seg, x_lo, x_hi);
  out[3 * b] = (int32_t)tile;
  out[3 * b + 1] = x_lo;
  out[3 * b + 2] = x_hi;
}

int step2_report_items(const Step2Launch& p, int32_t* out, int* eff_segments, int* eff_cap) {
  XLB_REQUIRE(out && eff_segments && eff_cap && p.tile_ty == 8 && (p.tile_tz == 64 || p.tile_tz == 48), "plan report: (8 x 64) / (8 x 48) tiles only");
  const unsigned tiles = (unsigned)(p.ny / 8) * (unsigned)(p.nz / p.tile_tz);
  const int segs = step2_eff_segments(p), swz = step2_eff_swizzle(p, tiles), n = (int)tiles * segs;
  if (p.tile_tz == 48)
    hipLaunchKernelGGL((k_step2_items<8, 48>), dim3((n + 255) / 256), dim3(256), 0, p.stream, p.tile_order, swz, segs, step2_eff_cap(p), p.x_begin, p.x_count, p.ny, p.nz, n, out);
  else
    hipLaunchKernelGGL((k_step2_items<8, 64>), dim3((n + 255) / 256), dim3(256), 0, p.stream, p.tile_order, swz, segs, step2_eff_cap(p), p.x_begin, p.x_count, p.ny, p.nz, n, out);
  XLB_HIP(hipGetLastError());
  *eff_segments = segs;
  *eff_cap = step2_eff_cap(p);
  return 0;
}

int step2_items(const Step2Launch& p) { return (p.ny / p.tile_ty) * (p.nz / p.tile_tz) * step2_eff_segments(p); }

}  // namespace xlb

#ifdef XLB_STEP2_TRACE
// debug builds only (tools/step2_phase_trace.py): the phase stamps of the last launch
extern "C" int xlbhip_debug_step2_trace(unsigned long long* out, int n) {
  constexpr int N = xlb::TRACE_PLANES * xlb::TRACE_WAVES * xlb::TRACE_EVENTS;
  if (n < N) return N;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(xlb::g_step2_trace), sizeof(unsigned long long) * N) == hipSuccess ? 0 : -1;
}
#endif
