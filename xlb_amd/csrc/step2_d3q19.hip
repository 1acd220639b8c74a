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
