// FlowStatistics: running sums of rho, u and their products over the cells of a population field, reduced over any subset of
// the grid axes, plus a blow-up watchdog (largest u.u, number of non-finite cells).  No reference counterpart: its drivers take
// these numbers from host copies of whole fields.
//
// One cell: rho and u from cell.hpp: moments<L, T> in the compute dtype T (the bits Macroscopic writes), promoted to double; every
// product and every sum below is taken in double.  Channels (STATS_ORDER 2): count, rho, rho^2, u_a (D), u_a u_b (n_pi, the order
// of second_moment); order 1: count, rho, u_a.
//
// Plan (a pure function of the local shape, the kept axes and the order — never of the device, the launch size or ghost planes).
// A ROW is one (x, y) with all its z; lanes always run along z, 64 of them per z chunk.  The rows split into the kept part
// k in [0, NK) (the kept ones of x, y) and the summed part s in [0, NS); the summed part is cut into NJ chunks of CH rows.
//   z kept:    item (k, j, zc), lane = one z: the lane adds CH rows of its z column in registers.  No lane meets another.
//   z summed:  item (k, j): the lane adds CH rows x every z chunk, then the 64 lanes are combined by a fixed butterfly.
// One wave works on one item at a time.  With NJ == 1 the item is the only owner of its bins and adds into the running sums itself;
// otherwise it writes partial j of its bins to scratch[j][channel][bin] and k_stats_combine adds the partials in j order.  No
// floating-point atomic anywhere: the sums are bit-identical from run to run.
//
// The first half of this file (everything up to "device only") also compiles for the host (tests/hip_on_cpu), where
// tests/stats_cpu_emulation.cpp runs it lane by lane in the plan's order.
#pragma once
#include "cell.hpp"

namespace xlb {

constexpr int STATS_LANES = 64;            // z positions of one item (one wave)
constexpr int STATS_TARGET_ITEMS = 4096;   // items the plan aims for: 4 waves per SIMD of a 256-CU device, all resident at once
constexpr int STATS_MIN_ROWS = 8;          // rows of a chunk below which splitting further does not pay
constexpr int STATS_KEEP_X = 1, STATS_KEEP_Y = 2, STATS_KEEP_Z = 4;
// scratch of the partial sums: NJ * channels * bins doubles.  NJ > 1 only while NK * z chunks < STATS_TARGET_ITEMS, and then
// NJ * NK * z chunks < 2 * STATS_TARGET_ITEMS, so it never holds more than 12 * 64 * 2 * 4096 doubles = 48 MiB
constexpr size_t STATS_MAX_SCRATCH_BYTES = (size_t)12 * STATS_LANES * 2 * STATS_TARGET_ITEMS * sizeof(double);

template <class L, int ORDER>
constexpr int stats_channels() {
  return ORDER == 2 ? 3 + L::D + n_pi<L>() : 2 + L::D;
}

// position of the product u_d u_e (d <= e) in the order of second_moment: (xx, xy, xz, yy, yz, zz) / (xx, xy, yy)
constexpr int stats_pair(int D, int d, int e) {
  int n = 0;
  for (int i = 0; i < d; ++i) n += D - i;
  return n + (e - d);
}

struct StatsExclude {
  uint32_t bits[8];  // bc_mask values whose cells are not sampled
};

struct StatsPlan {
  int nx, ny, nz, keep;
  int nk, ns, nzc;  // kept row groups, summed rows per group, z chunks
  int ch, nj;       // rows per chunk, chunks
  int64_t items;
  int64_t bins;
};

__host__ __device__ inline StatsPlan stats_plan(int nx, int ny, int nz, int keep) {
  StatsPlan p;
  p.nx = nx;
  p.ny = ny;
  p.nz = nz;
  p.keep = keep;
  const bool kx = keep & STATS_KEEP_X, ky = keep & STATS_KEEP_Y, kz = keep & STATS_KEEP_Z;
  p.nk = (kx ? nx : 1) * (ky ? ny : 1);
  p.ns = (kx ? 1 : nx) * (ky ? 1 : ny);
  p.nzc = (nz + STATS_LANES - 1) / STATS_LANES;
  const int64_t per_chunk = (int64_t)p.nk * (kz ? p.nzc : 1);  // items one chunk of every group makes
  int64_t want = (STATS_TARGET_ITEMS + per_chunk - 1) / per_chunk;
  const int64_t most = (p.ns + STATS_MIN_ROWS - 1) / STATS_MIN_ROWS;
  if (want > most) want = most;
  if (want < 1) want = 1;
  p.ch = (int)((p.ns + want - 1) / want);
  p.nj = (p.ns + p.ch - 1) / p.ch;
  p.items = per_chunk * p.nj;
  p.bins = (int64_t)p.nk * (kz ? nz : 1);
  return p;
}

struct StatsItem {
  int k, j, zc;
};
__host__ __device__ inline StatsItem stats_item(const StatsPlan& p, int64_t item) {
  StatsItem it;
  if (p.keep & STATS_KEEP_Z) {
    it.zc = (int)(item % p.nzc);
    item /= p.nzc;
  } else {
    it.zc = 0;
  }
  it.j = (int)(item % p.nj);
  it.k = (int)(item / p.nj);
  return it;
}
// row s of group k
__host__ __device__ inline void stats_row(const StatsPlan& p, int k, int s, int& x, int& y) {
  const bool kx = p.keep & STATS_KEEP_X, ky = p.keep & STATS_KEEP_Y;
  if (kx && ky) {
    x = k / p.ny;
    y = k % p.ny;
  } else if (kx) {
    x = k;
    y = s;
  } else if (ky) {
    x = s;
    y = k;
  } else {
    x = s / p.ny;
    y = s % p.ny;
  }
}
// bin of a cell of group k
__host__ __device__ inline int64_t stats_bin(const StatsPlan& p, int k, int z) { return (p.keep & STATS_KEEP_Z) ? (int64_t)k * p.nz + z : k; }

// what one lane carries through an item
template <class L, class T, int ORDER>
struct StatsAcc {
  double c[stats_channels<L, ORDER>()];
  T umax;        // largest u.u of the sampled cells
  unsigned bad;  // sampled cells whose rho or u is not finite
};
template <class L, class T, int ORDER>
__device__ __forceinline__ void stats_clear(StatsAcc<L, T, ORDER>& a) {
  static_for<stats_channels<L, ORDER>()>([&](auto cc) { a.c[decltype(cc)::value] = 0.0; });
  a.umax = T(0);
  a.bad = 0u;
}

// the channels of one cell, from its populations (storage index i) and its mask byte.  Written without branches: a cell that is not
// sampled, or not finite, adds 0.0 to every sum (which changes no bit of it), so the accumulators stay in one set of registers.
template <class L, class T, class S, int ORDER>
__device__ __forceinline__ void stats_cell(const S* __restrict__ f, size_t plane_stride, size_t i, const uint8_t* __restrict__ bc, size_t ib,
                                           const StatsExclude& ex, StatsAcc<L, T, ORDER>& a) {
  constexpr int D = L::D, O = 3 - L::D;
  T ff[L::Q];
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    ff[l] = to_compute<T, S>(f[(size_t)l * plane_stride + i]);
  });
  bool sampled = true;
  if (bc) {
    const unsigned id = bc[ib];
    unsigned word = ex.bits[0];  // (a chain of selects over the eight words: no second, dependent load)
    static_for<7>([&](auto kc) {
      constexpr unsigned k = decltype(kc)::value + 1;
      word = (id >> 5) == k ? ex.bits[k] : word;
    });
    sampled = ((word >> (id & 31u)) & 1u) == 0u;
  }
  T rho, u[3];
  moments<L, T>(ff, rho, u);
  bool finite = __builtin_isfinite(rho);
  static_for<D>([&](auto ac) { finite = finite && __builtin_isfinite(u[decltype(ac)::value + O]); });
  const bool good = sampled && finite;
  a.bad += (sampled && !finite) ? 1u : 0u;
  T usq = u[O] * u[O];
  static_for<D - 1>([&](auto ac) {
    constexpr int b = decltype(ac)::value + 1 + O;
    usq = usq + u[b] * u[b];
  });
  a.umax = (good && usq > a.umax) ? usq : a.umax;
  const double r = good ? (double)rho : 0.0;
  double ud[3];
  static_for<D>([&](auto ac) { ud[decltype(ac)::value + O] = good ? (double)u[decltype(ac)::value + O] : 0.0; });
  a.c[0] = a.c[0] + (good ? 1.0 : 0.0);
  a.c[1] = a.c[1] + r;
  if constexpr (ORDER == 2) {
    a.c[2] = a.c[2] + r * r;
    static_for<D>([&](auto ac) {
      constexpr int d = decltype(ac)::value;
      a.c[3 + d] = a.c[3 + d] + ud[d + O];
    });
    static_for<D>([&](auto ac) {
      constexpr int d = decltype(ac)::value;
      static_for<D - d>([&](auto ec) {
        constexpr int e = d + decltype(ec)::value;
        constexpr int n = 3 + D + stats_pair(D, d, e);
        a.c[n] = a.c[n] + ud[d + O] * ud[e + O];
      });
    });
  } else {
    static_for<D>([&](auto ac) {
      constexpr int d = decltype(ac)::value;
      a.c[2 + d] = a.c[2 + d] + ud[d + O];
    });
  }
}

// the cells of one lane of one item, in the plan's order: fn(storage index in f, storage index in bc_mask)
template <class Fn>
__device__ __forceinline__ void stats_lane_cells(const StatsPlan& p, const StatsItem& it, int lane, int f_halo, int bc_halo, Fn&& fn) {
  const int s0 = it.j * p.ch, s1 = min(s0 + p.ch, p.ns);
  const bool kz = p.keep & STATS_KEEP_Z;
  const int zc0 = kz ? it.zc : 0, zc1 = kz ? it.zc + 1 : p.nzc;
  for (int s = s0; s < s1; ++s) {
    int x, y;
    stats_row(p, it.k, s, x, y);
    const size_t row = ((size_t)(x + f_halo) * p.ny + y) * p.nz, brow = ((size_t)(x + bc_halo) * p.ny + y) * p.nz;
    for (int zc = zc0; zc < zc1; ++zc) {
      const int z = zc * STATS_LANES + lane;
      if (z < p.nz) fn(row + z, brow + z);
    }
  }
}
template <class L, class T, class S, int ORDER>
__device__ __forceinline__ void stats_lane(const StatsPlan& p, const StatsItem& it, int lane, const S* __restrict__ f, size_t plane_stride, int f_halo,
                                           const uint8_t* __restrict__ bc, int bc_halo, const StatsExclude& ex, StatsAcc<L, T, ORDER>& a) {
  stats_lane_cells(p, it, lane, f_halo, bc_halo, [&](size_t i, size_t ib) { stats_cell<L, T, S, ORDER>(f, plane_stride, i, bc, ib, ex, a); });
}

// shape of k_stats_combine's blocks for `cols` = channels * bins columns: bw columns x jw partial lanes (bw * jw = 256)
__host__ __device__ inline void stats_combine_shape(size_t cols, int& bw, int& jw) {
  bw = cols <= 64 ? 1 : 16;
  jw = 256 / bw;
}

// what the watchdog keeps on the device
struct StatsWatch {
  unsigned long long umax_bits;  // bit pattern of the largest u.u (compute dtype, low bits) of the last sample
  unsigned long long bad_last;   // non-finite cells of the last sample
  unsigned long long bad_total;  // ... since the last reset
};
template <class T>
__device__ __forceinline__ unsigned long long stats_bits(T v) {
  if constexpr (sizeof(T) == 4) {
    return (unsigned long long)__float_as_uint((float)v);
  } else {
    unsigned long long b;
    __builtin_memcpy(&b, &v, 8);
    return b;
  }
}

#ifdef __HIPCC__
// ---- device only ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double stats_xor_add(double v, int m) { return v + __shfl_xor(v, m, STATS_LANES); }

// 256 threads = 4 waves, one item per wave at a time, items strided over the launch.
template <class L, class T, class S, int ORDER, bool KZ>
__global__ __launch_bounds__(256) void k_stats_sample(StatsPlan p, const S* __restrict__ f, size_t plane_stride, int f_halo, const uint8_t* __restrict__ bc,
                                                      int bc_halo, StatsExclude ex, double* __restrict__ sums, double* __restrict__ scratch,
                                                      StatsWatch* __restrict__ watch) {
  constexpr int C = stats_channels<L, ORDER>();
  const int lane = threadIdx.x % STATS_LANES;
  // (readfirstlane: the wave's number is the same in all its lanes, which lets the row arithmetic and the plane bases live in scalar registers)
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x / STATS_LANES) + __builtin_amdgcn_readfirstlane((int)threadIdx.x / STATS_LANES);
  const int64_t waves = (int64_t)gridDim.x * (blockDim.x / STATS_LANES);
  constexpr bool kz = KZ;  // = p.keep & STATS_KEEP_Z, which the plan's functions read
  T umax = T(0);
  unsigned bad = 0u;
  for (int64_t item = wave; item < p.items; item += waves) {
    const StatsItem it = stats_item(p, item);
    StatsAcc<L, T, ORDER> a;
    stats_clear(a);
    stats_lane<L, T, S, ORDER>(p, it, lane, f, plane_stride, f_halo, bc, bc_halo, ex, a);
    if (a.umax > umax) umax = a.umax;
    bad += a.bad;
    const int z = it.zc * STATS_LANES + lane;
    bool writer = z < p.nz;
    if constexpr (!kz) {
      static_for<C>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        double v = a.c[c];
        v = stats_xor_add(v, 1);
        v = stats_xor_add(v, 2);
        v = stats_xor_add(v, 4);
        v = stats_xor_add(v, 8);
        v = stats_xor_add(v, 16);
        v = stats_xor_add(v, 32);
        a.c[c] = v;
      });
      writer = lane == 0;
    }
    if (writer) {
      const size_t bin = (size_t)stats_bin(p, it.k, z);
      if (p.nj == 1) {
        static_for<C>([&](auto cc) {
          constexpr int c = decltype(cc)::value;
          sums[(size_t)c * p.bins + bin] = sums[(size_t)c * p.bins + bin] + a.c[c];
        });
      } else {
        static_for<C>([&](auto cc) {
          constexpr int c = decltype(cc)::value;
          scratch[((size_t)it.j * C + c) * p.bins + bin] = a.c[c];
        });
      }
    }
  }
  // the watchdog: integer maxima and integer sums, whose result does not depend on the order
  unsigned long long ub = stats_bits<T>(umax);
  for (int m = 1; m < STATS_LANES; m <<= 1) {
    const unsigned long long o = __shfl_xor(ub, m, STATS_LANES);
    ub = o > ub ? o : ub;
    bad += __shfl_xor(bad, m, STATS_LANES);
  }
  if (lane == 0) {
    if (ub != 0ull) atomicMax(&watch->umax_bits, ub);
    if (bad != 0u) {
      atomicAdd(&watch->bad_last, (unsigned long long)bad);
      atomicAdd(&watch->bad_total, (unsigned long long)bad);
    }
  }
}

// sums[col] += scratch[0][col] + scratch[1][col] + ... in a fixed order: 256 threads = bw columns x jw partial lanes; lane r adds the
// partials r, r + jw, ... one after the other, then the jw lane sums are added in lane order.
static __global__ __launch_bounds__(256) void k_stats_combine(const double* __restrict__ scratch, double* __restrict__ sums, size_t cols, int nj, int bw, int jw) {
  __shared__ double part[256];
  const int t = threadIdx.x, b = t % bw, r = t / bw;
  const size_t col = (size_t)blockIdx.x * bw + b;
  double v = 0.0;
  if (col < cols)
    for (int j = r; j < nj; j += jw) v = v + scratch[(size_t)j * cols + col];
  part[t] = v;
  __syncthreads();
  if (r == 0 && col < cols) {
    double s = part[b];
    for (int q = 1; q < jw; ++q) s = s + part[q * bw + b];
    sums[col] = sums[col] + s;
  }
}
#endif  // __HIPCC__

}  // namespace xlb
