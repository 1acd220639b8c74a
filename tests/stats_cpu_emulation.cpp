// The host-compilable half of xlb_amd/csrc/stats_kernels.hpp (the channels of one cell, the cell -> bin map, the item -> cells plan)
// compiled through tests/hip_on_cpu and run item by item, lane by lane, the way k_stats_sample and k_stats_combine of csrc/stats.hip
// walk it.  tests/test_flow_statistics_host.py compares the sums with the NumPy restatement and checks the plan's properties; what it
// cannot show is the GPU's code generation and its wave shuffles.
#include "stats_kernels.hpp"
#include <vector>
thread_local emulated_dim3 threadIdx, blockIdx, blockDim, gridDim;
using namespace xlb;

// one sample added to sums [channels][bins]; watch = {bit pattern of the largest u.u, non-finite cells}
template <class L, class T, class S, int ORDER>
static int sample(const StatsPlan& p, const S* f, size_t plane_stride, int f_halo, const uint8_t* bc, int bc_halo, const StatsExclude& ex, double* sums,
                  unsigned long long* watch) {
  constexpr int C = stats_channels<L, ORDER>();
  const bool kz = p.keep & STATS_KEEP_Z;
  std::vector<double> scratch(p.nj > 1 ? (size_t)p.nj * C * p.bins : 0);
  for (int64_t item = 0; item < p.items; ++item) {
    const StatsItem it = stats_item(p, item);
    std::vector<StatsAcc<L, T, ORDER>> a(STATS_LANES);
    for (int lane = 0; lane < STATS_LANES; ++lane) {
      stats_clear(a[lane]);
      stats_lane<L, T, S, ORDER>(p, it, lane, f, plane_stride, f_halo, bc, bc_halo, ex, a[lane]);
      atomicMax(&watch[0], stats_bits<T>(a[lane].umax));
      watch[1] += a[lane].bad;
    }
    if (!kz)  // the butterfly of the wave: every lane adds its partner's value, six times
      for (int m = 1; m < STATS_LANES; m <<= 1) {
        std::vector<StatsAcc<L, T, ORDER>> b = a;
        for (int lane = 0; lane < STATS_LANES; ++lane)
          for (int c = 0; c < C; ++c) a[lane].c[c] = b[lane].c[c] + b[lane ^ m].c[c];
      }
    for (int lane = 0; lane < STATS_LANES; ++lane) {
      const int z = it.zc * STATS_LANES + lane;
      if (kz ? z >= p.nz : lane != 0) continue;
      const size_t bin = (size_t)stats_bin(p, it.k, z);
      for (int c = 0; c < C; ++c) {
        if (p.nj == 1)
          sums[(size_t)c * p.bins + bin] = sums[(size_t)c * p.bins + bin] + a[lane].c[c];
        else
          scratch[((size_t)it.j * C + c) * p.bins + bin] = a[lane].c[c];
      }
    }
  }
  if (p.nj > 1) {  // k_stats_combine
    const size_t cols = (size_t)C * p.bins;
    int bw, jw;
    stats_combine_shape(cols, bw, jw);
    for (size_t col = 0; col < cols; ++col) {
      double s = 0.0;
      for (int r = 0; r < jw; ++r) {
        double v = 0.0;
        for (int j = r; j < p.nj; j += jw) v = v + scratch[(size_t)j * cols + col];
        s = r == 0 ? v : s + v;
      }
      sums[col] = sums[col] + s;
    }
  }
  return C;
}

// fields as the library lays them out: element (l, x, y, z) at f[l * plane_stride + ((x + halo) * ny + y) * nz + z]
extern "C" int stats_sample_cpu(int lattice, int cdt, int sdt, const void* f, size_t plane_stride, int f_halo, const uint8_t* bc, int bc_halo, int nx, int ny,
                                int nz, int keep, int order, const uint32_t* exclude, double* sums, unsigned long long* watch) {
  const StatsPlan p = stats_plan(nx, ny, nz, keep);
  StatsExclude ex;
  for (int i = 0; i < 8; ++i) ex.bits[i] = exclude[i];
#define GO3(L, T, S) \
  return order == 2 ? sample<L, T, S, 2>(p, (const S*)f, plane_stride, f_halo, bc, bc_halo, ex, sums, watch) \
                    : sample<L, T, S, 1>(p, (const S*)f, plane_stride, f_halo, bc, bc_halo, ex, sums, watch);
#define GO(L)                                                      \
  if (cdt == XLBHIP_F32 && sdt == XLBHIP_F32) { GO3(L, float, float) }     \
  if (cdt == XLBHIP_F32 && sdt == XLBHIP_F16) { GO3(L, float, _Float16) }  \
  if (cdt == XLBHIP_F64 && sdt == XLBHIP_F64) { GO3(L, double, double) }   \
  if (cdt == XLBHIP_F64 && sdt == XLBHIP_F32) { GO3(L, double, float) }    \
  if (cdt == XLBHIP_F64 && sdt == XLBHIP_F16) { GO3(L, double, _Float16) } \
  return -1;
  if (lattice == XLBHIP_D2Q9) { GO(D2Q9) }
  if (lattice == XLBHIP_D3Q19) { GO(D3Q19) }
  GO(D3Q27)
}

// the plan's numbers: nk, ns, nzc, ch, nj, items, bins
extern "C" void stats_plan_cpu(int nx, int ny, int nz, int keep, int64_t out[7]) {
  const StatsPlan p = stats_plan(nx, ny, nz, keep);
  out[0] = p.nk, out[1] = p.ns, out[2] = p.nzc, out[3] = p.ch, out[4] = p.nj, out[5] = p.items, out[6] = p.bins;
}

// every (storage cell, partial = j, bin) the plan visits on a field with `halo` ghost planes, in the plan's order; returns their number
// (room for `capacity` entries)
extern "C" int64_t stats_visit_cpu(int nx, int ny, int nz, int keep, int halo, int64_t capacity, int64_t* cell, int64_t* partial, int64_t* bin) {
  const StatsPlan p = stats_plan(nx, ny, nz, keep);
  int64_t n = 0;
  for (int64_t item = 0; item < p.items; ++item) {
    const StatsItem it = stats_item(p, item);
    for (int lane = 0; lane < STATS_LANES; ++lane)
      stats_lane_cells(p, it, lane, halo, halo, [&](size_t i, size_t) {
        if (n < capacity) {
          cell[n] = (int64_t)i;
          partial[n] = it.j;
          bin[n] = stats_bin(p, it.k, (int)(i % (size_t)nz));
        }
        ++n;
      });
  }
  return n;
}
