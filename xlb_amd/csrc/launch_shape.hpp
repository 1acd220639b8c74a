// The block and grid of the row kernels (k_step, k_step_scalar, k_adjoint_step): one definition for their launchers and for the
// adjoint's count of per-block partial sums.  Plain integers — no HIP, so that tests/test_bc_tables.py compiles it for the CPU.
#pragma once

namespace xlb {

struct RowBlockShape {
  int tz, ty;      // block: threads along z, rows stacked along y
  int gx, gy, gz;  // grid: blocks along a row, along y, one per x plane
};

// Threads along z: a row of nzq threads in equal chunks of whole waves (nzq = 384 -> 2 x 192, not 256 + 128), narrowed to block_tz
// when that is set (> 0) and smaller; rows stacked to fill the block of `threads`, at most ny of them.
inline RowBlockShape row_block_shape(int nzq, int ny, int planes, int threads, int block_tz) {
  int tz = nzq;
  if (tz > threads) {
    const int chunks = (nzq + threads - 1) / threads;
    tz = (nzq + chunks - 1) / chunks;
    tz = (tz + 63) / 64 * 64;
    if (tz > threads) tz = threads;
  }
  if (block_tz > 0 && block_tz < tz) tz = block_tz;
  int ty = threads / tz;
  if (ty < 1) ty = 1;
  if (ty > ny) ty = ny;
  return {tz, ty, (nzq + tz - 1) / tz, (ny + ty - 1) / ty, planes};
}

}  // namespace xlb
