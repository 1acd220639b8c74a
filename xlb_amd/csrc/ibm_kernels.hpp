// Immersed-boundary coupling kernels (reference: xlb/operator/stepper/ibm_stepper.py:156-178 and :264-476).
//
// Everything here works on the FOOTPRINT of the markers — the cells inside the 4 x 4 x 4 support of Peskin's kernel around a
// marker, i.e. the cells with a positive weight sum — and on the markers themselves.  No launch scales with the grid.
//
//   k_ibm_mark / _wmax / _weights (positions changed) cell -> slot map, slot -> cell list, largest weight, weight sums W
//   k_ibm_moments                (once per call)      rho, u of f_1 on the listed cells
//   k_ibm_interp                 (once per call)      d_k = U_k - u(X_k): u and the weights do not change between sweeps
//   k_ibm_spread / _correct / _update  (per sweep)    acc = sum_k w A F, G = relaxation (acc / W - u), F += d, residual flag
//   k_ibm_apply                  (once per call)      f_1 += store(feq(rho, u + G) - feq(rho, u)) on the listed cells
//
// Accumulation.  acc and W are sums over the markers that reach a cell, added with atomics.  Floating-point atomic adds would make
// the result depend on the arrival order, so the contributions are converted to 64-bit FIXED POINT and added with integer atomics:
// the sum is exact in the integers, hence independent of the order (and of the order of the markers in the caller's arrays).
// What the coupling uses is the RATIO acc / W, and W can be arbitrarily small (a cell at the very edge of one support), so the
// quantum is per cell: 2^-40 of the power of two above the cell's LARGEST weight, which k_ibm_wmax finds first with an integer
// atomicMax on the fp32 bit pattern of the weights (positive floats order like their bits: order-independent too).  W then carries a
// relative rounding of at most (markers reaching the cell) x 2^-40, acc the same relative to |A F| — far below the fp32 rounding of
// the sums.  The 64-bit word holds |sum| < 2^23 in units of (largest weight x |A F|) with A (a surface element in lattice units) and
// F (a velocity difference, << 1) of order one; a single contribution is clamped to 2^60 quanta (a diverged run), so the
// conversion itself never overflows.
//
// Early exit.  The sweep loop of the reference stops when no marker's force changed by more than the tolerance (:364-368, :413-419).
// Here every sweep's kernels are always enqueued; the kernels of sweep `it` read the residual word of sweep it - 1 and return at
// once when it stayed 0 (a skipped sweep leaves its own word 0, so the following ones are skipped too).  No host read in a call.
#pragma once
#include "ops_kernels.hpp"

namespace xlb {

constexpr int IBM_MAX_SWEEPS = 64;
constexpr double IBM_FIX_CLAMP = 1152921504606846976.0;  // 2^60 quanta

// device control block of one call: residual flag per sweep and the number of sweeps that ran
struct IbmControl {
  int flag[IBM_MAX_SWEEPS];
  int sweeps;
};

// The quantum of a cell whose largest weight has the fp32 bit pattern `wbits`: that weight is m 2^e with m in [1/2, 1) and
// e = E - 126 (E the biased exponent, denormals counted as E = 1); the quantum is 2^(e - 40).
__device__ __forceinline__ int ibm_scale_exp(unsigned wbits) {
  const int E = (int)(wbits >> 23);
  return 166 - (E < 1 ? 1 : E);  // 40 - e
}
__device__ __forceinline__ unsigned long long ibm_to_fixed(double v, unsigned wbits) {
  v = ldexp(v, ibm_scale_exp(wbits));
  v = fmin(fmax(v, -IBM_FIX_CLAMP), IBM_FIX_CLAMP);
  return (unsigned long long)(long long)llrint(v);  // (two's complement: unsigned adds wrap to the signed sum)
}
template <class T>
__device__ __forceinline__ T ibm_from_fixed(unsigned long long v, unsigned wbits) {
  return static_cast<T>(ldexp((double)(long long)v, -ibm_scale_exp(wbits)));
}

// Peskin's 4-point function, ibm_stepper.py:158-173
template <class T>
__device__ __forceinline__ T peskin_weight(T r) {
  const T a = r < T(0) ? -r : r;
  if (a <= T(1)) return T(0.125) * ((T(3) - T(2) * a) + sqrt((T(1) + T(4) * a) - (T(4) * a) * a));
  if (a <= T(2)) return T(0.125) * ((T(5) - T(2) * a) - sqrt((T(-7) + T(12) * a) - (T(4) * a) * a));
  return T(0);
}

// Candidate c (0 .. 63) of marker k: the cell (base + j) per axis, base = floor(X - 1/2) - 1, which covers every cell centre with
// |r| < 2 (r = 2 exactly has weight 0).  False when the cell lies outside the box (no periodic wrap: a marker near a face loses part
// of its support), the position is not a finite number, or the weight is not positive.
template <class T>
__device__ __forceinline__ bool ibm_candidate(const float* __restrict__ pos, int64_t k, int c, const Dims& d, uint32_t& cell, T& w) {
  const int j[3] = {c >> 4, (c >> 2) & 3, c & 3};
  const int n[3] = {d.nx, d.ny, d.nz};
  int i[3];
  T ww[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const T X = static_cast<T>(pos[3 * k + a]);
    if (!(X > T(-4) && X < T(n[a] + 4))) return false;  // (also NaN; keeps the conversion to int defined)
    i[a] = (int)floor(X - T(0.5)) - 1 + j[a];
    if (i[a] < 0 || i[a] >= n[a]) return false;
    ww[a] = peskin_weight<T>((T(i[a]) + T(0.5)) - X);  // cell (i, j, k) sits at (i + 1/2, ...): ibm_stepper.py:105
  }
  w = (ww[0] * ww[1]) * ww[2];  // ibm_stepper.py:176-178
  cell = (uint32_t)(((size_t)i[0] * d.ny + i[1]) * d.nz + i[2]);
  return w > T(0);
}

// sweep `it` does not run: the sweep before it computed a residual (it - 1 > 0, tolerance > 0) and no marker exceeded the tolerance
__device__ __forceinline__ bool ibm_sweep_skipped(const IbmControl* ctl, int it, int residual_on) {
  return residual_on && it >= 2 && ctl->flag[it - 1] == 0;
}

// ---- footprint (rebuilt when the positions change) ----------------------------------------------------------------------------
__global__ void k_ibm_clear(int32_t* __restrict__ map, const uint32_t* __restrict__ list, const int* __restrict__ count, int64_t cap) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= cap || s >= *count) return;
  map[list[s]] = -1;
}

template <class T>
__global__ void k_ibm_mark(const float* __restrict__ pos, int64_t n, Dims d, int32_t* map, uint32_t* __restrict__ list, int* count, int64_t cap) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 64) return;
  uint32_t cell;
  T w;
  if (!ibm_candidate<T>(pos, t >> 6, (int)(t & 63), d, cell, w)) return;
  if (atomicCAS(&map[cell], -1, -2) != -1) return;  // somebody else lists this cell
  const int s = atomicAdd(count, 1);
  if (s < cap) {  // (always: cap = min(64 n, cells) bounds the number of distinct cells)
    list[s] = cell;
    atomicExch(&map[cell], s);
  }
}

// the largest weight per slot, as the fp32 bit pattern (weights are positive: their order is that of the bits)
template <class T>
__global__ void k_ibm_wmax(const float* __restrict__ pos, int64_t n, Dims d, const int32_t* __restrict__ map, unsigned* wbits, int64_t cap) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 64) return;
  uint32_t cell;
  T w;
  if (!ibm_candidate<T>(pos, t >> 6, (int)(t & 63), d, cell, w)) return;
  const int s = map[cell];
  if (s < 0 || s >= cap) return;
  atomicMax(&wbits[s], __float_as_uint(static_cast<float>(w)));
}

template <class T>
__global__ void k_ibm_weights(const float* __restrict__ pos, int64_t n, Dims d, const int32_t* __restrict__ map, const unsigned* __restrict__ wbits,
                              unsigned long long* W, int64_t cap) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 64) return;
  uint32_t cell;
  T w;
  if (!ibm_candidate<T>(pos, t >> 6, (int)(t & 63), d, cell, w)) return;
  const int s = map[cell];
  if (s < 0 || s >= cap) return;
  atomicAdd(&W[s], ibm_to_fixed((double)w, wbits[s]));
}

// ---- once per call ----------------------------------------------------------------------------------------------------------
// rho, u of f_1 on the listed cells (ibm_stepper.py:310-318)
template <class L, class T, class S>
__global__ void k_ibm_moments(const S* __restrict__ f, size_t plane_stride, const uint32_t* __restrict__ list, const int* __restrict__ count, int64_t cap,
                              T* __restrict__ u) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= cap || s >= *count) return;
  const size_t cell = list[s];
  T ff[L::Q];
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    ff[l] = to_compute<T, S>(f[(size_t)l * plane_stride + cell]);
  });
  T r, uu[3];
  moments<L, T>(ff, r, uu);
  u[3 * s] = uu[0];
  u[3 * s + 1] = uu[1];
  u[3 * s + 2] = uu[2];
}

// d_k = U_k - (sum_c w u[c]) / (sum_c w) (0 for an empty support), ibm_stepper.py:341-361; the forces start at zero (:391)
template <class T>
__global__ void k_ibm_interp(const float* __restrict__ pos, const float* __restrict__ vel, int64_t n, Dims d, const int32_t* __restrict__ map, int64_t cap,
                             const T* __restrict__ u, T* __restrict__ dk, T* __restrict__ F) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  T num[3] = {T(0), T(0), T(0)}, den = T(0);
  for (int c = 0; c < 64; ++c) {
    uint32_t cell;
    T w;
    if (!ibm_candidate<T>(pos, k, c, d, cell, w)) continue;
    const int s = map[cell];
    if (s < 0 || s >= cap) continue;
    num[0] = num[0] + u[3 * s] * w;
    num[1] = num[1] + u[3 * s + 1] * w;
    num[2] = num[2] + u[3 * s + 2] * w;
    den = den + w;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const T ui = den > T(0) ? num[a] / den : T(0);
    dk[3 * k + a] = static_cast<T>(vel[3 * k + a]) - ui;
    F[3 * k + a] = T(0);
  }
}

// ---- per sweep --------------------------------------------------------------------------------------------------------------
// acc[c] += (F_k w) A_k, ibm_stepper.py:283-293
template <class T>
__global__ void k_ibm_spread(int it, int residual_on, const IbmControl* __restrict__ ctl, const float* __restrict__ pos, const float* __restrict__ area,
                             const T* __restrict__ F, int64_t n, Dims d, const int32_t* __restrict__ map, int64_t cap, const unsigned* __restrict__ wbits,
                             unsigned long long* acc) {
  if (ibm_sweep_skipped(ctl, it, residual_on)) return;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 64) return;
  const int64_t k = t >> 6;
  uint32_t cell;
  T w;
  if (!ibm_candidate<T>(pos, k, (int)(t & 63), d, cell, w)) return;
  const int s = map[cell];
  if (s < 0 || s >= cap) return;
  const T A = static_cast<T>(area[k]);
#pragma unroll
  for (int a = 0; a < 3; ++a) atomicAdd(&acc[3 * (size_t)s + a], ibm_to_fixed((double)((F[3 * k + a] * w) * A), wbits[s]));
}

// G = relaxation (acc / W - u) where W > 0, else acc (ibm_stepper.py:320-325); acc is left zero for the next sweep
template <class T>
__global__ void k_ibm_correct(int it, int residual_on, const IbmControl* __restrict__ ctl, const int* __restrict__ count, int64_t cap,
                              const unsigned* __restrict__ wbits, const unsigned long long* __restrict__ W, unsigned long long* __restrict__ acc,
                              const T* __restrict__ u, T relaxation, T* __restrict__ G) {
  if (ibm_sweep_skipped(ctl, it, residual_on)) return;
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= cap || s >= *count) return;
  const unsigned wb = wbits[s];
  const T wsum = ibm_from_fixed<T>(W[s], wb);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const T v = ibm_from_fixed<T>(acc[3 * s + a], wb);
    acc[3 * s + a] = 0;
    G[3 * s + a] = wsum > T(0) ? relaxation * (v / wsum - u[3 * s + a]) : v;
  }
}

// F_k += d_k; from the second sweep on, |F_k - prev_k|^2 > tolerance^2 raises the sweep's flag (ibm_stepper.py:361-368)
template <class T>
__global__ void k_ibm_update(int it, int residual_on, IbmControl* ctl, int64_t n, const T* __restrict__ dk, T* __restrict__ F, T tolerance_sq) {
  if (ibm_sweep_skipped(ctl, it, residual_on)) return;
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  T sq = T(0);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const T prev = F[3 * k + a];
    const T next = prev + dk[3 * k + a];
    F[3 * k + a] = next;
    const T diff = next - prev;
    sq = sq + diff * diff;
  }
  if (residual_on && it > 0 && sq > tolerance_sq) atomicMax(&ctl->flag[it], 1);
  if (k == 0) ctl->sweeps = it + 1;
}

// ---- once per call: f_1 += store(feq(rho, u + G) - feq(rho, u)), ibm_stepper.py:238-261 -----------------------------------------
template <class L, class T, class S>
__global__ void k_ibm_apply(S* __restrict__ f, size_t plane_stride, const uint32_t* __restrict__ list, const int* __restrict__ count, int64_t cap,
                            const T* __restrict__ G) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= cap || s >= *count) return;
  const size_t cell = list[s];
  S fs[L::Q];
  T ff[L::Q];
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    fs[l] = f[(size_t)l * plane_stride + cell];
    ff[l] = to_compute<T, S>(fs[l]);
  });
  T r, uu[3];
  moments<L, T>(ff, r, uu);
  T uf[3] = {uu[0] + G[3 * s], uu[1] + G[3 * s + 1], uu[2] + G[3 * s + 2]};
  T feq[L::Q], feq_force[L::Q];
  equilibrium<L, T>(r, uf, feq_force);
  equilibrium<L, T>(r, uu, feq);
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    f[(size_t)l * plane_stride + cell] = fs[l] + to_store<S, T>(feq_force[l] - feq[l]);
  });
}

}  // namespace xlb
