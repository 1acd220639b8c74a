// The strip-buffer instantiations of the two-steps-per-pass kernel (step2_kernel.hpp, "Strip buffers") for D3Q19 / BGK / FP32FP32,
// (8 x 64) tiles, bit-exact body: phase A's halo columns come from the source field's strips (STRIPS & 1), phase B writes the
// destination's (STRIPS & 2).  A pass whose source has no valid strips (a single step or an upload wrote it) only writes them; on
// slab-decomposed fields the two edge launches — whose phase A pulls from ghost planes, which carry no strips — only write, too.
#include "step2_launch.hpp"

namespace xlb {

int launch_step2_d3q19_bgk_strips(const Step2Launch& p) {
  XLB_REQUIRE(p.tile_ty == 8 && p.tile_tz == 64 && !p.fast_bgk && p.strips != Strips::none, "strip buffers: (8 x 64) tiles, bit-exact body");
  if (p.strips == Strips::rowmap) {  // (enum Strips, step2_kernel.hpp; "fuse2_rowmap": measurement option)
    XLB_REQUIRE(p.has_bc, "fuse2_rowmap: the BC-free kernel has row-aligned lanes anyway");
    return p.halo ? launch2f<D3Q19, 1, 8, 64, true, false, float, XLBHIP_BGK, 4>(p) : launch2f<D3Q19, 1, 8, 64, false, false, float, XLBHIP_BGK, 4>(p);
  }
  const bool rw = p.strips == Strips::read_write;
  if (p.halo) {
    if (rw) return p.has_bc ? launch2f<D3Q19, 1, 8, 64, true, false, float, XLBHIP_BGK, 3>(p) : launch2f<D3Q19, 0, 8, 64, true, false, float, XLBHIP_BGK, 3>(p);
    return p.has_bc ? launch2f<D3Q19, 1, 8, 64, true, false, float, XLBHIP_BGK, 2>(p) : launch2f<D3Q19, 0, 8, 64, true, false, float, XLBHIP_BGK, 2>(p);
  }
  if (rw) return p.has_bc ? launch2f<D3Q19, 1, 8, 64, false, false, float, XLBHIP_BGK, 3>(p) : launch2f<D3Q19, 0, 8, 64, false, false, float, XLBHIP_BGK, 3>(p);
  return p.has_bc ? launch2f<D3Q19, 1, 8, 64, false, false, float, XLBHIP_BGK, 2>(p) : launch2f<D3Q19, 0, 8, 64, false, false, float, XLBHIP_BGK, 2>(p);
}

}  // namespace xlb

#ifdef XLB_STEP2_TRACE
// debug builds only (tools/step2_phase_trace.py): the phase stamps of the last launch of THIS translation unit's kernels (the stamp
// buffer is per translation unit; step2_d3q19.hip has the reader of the instantiations without strip buffers)
extern "C" int xlbhip_debug_step2_trace_strips(unsigned long long* out, int n) {
  constexpr int N = xlb::TRACE_PLANES * xlb::TRACE_WAVES * xlb::TRACE_EVENTS;
  if (n < N) return N;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(xlb::g_step2_trace), sizeof(unsigned long long) * N) == hipSuccess ? 0 : -1;
}
#endif
