// Stand-in for <hip/hip_runtime.h> that lets kernel headers of xlb_amd/csrc compile for the HOST (tests/ibm_cpu_emulation.cpp): the
// qualifiers vanish, the thread indices are plain variables the driver sets, and atomics are ordinary read-modify-writes (one emulated
// thread runs after the other).  Test infrastructure only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(...)
#define __shared__ static
struct emulated_dim3 {
  unsigned x = 0, y = 0, z = 0;
};
extern thread_local emulated_dim3 threadIdx, blockIdx, blockDim, gridDim;
inline void __syncthreads() {}
template <class T> inline T atomicAdd(T* p, T v) { T o = *p; *p = o + v; return o; }
inline int atomicCAS(int* p, int c, int v) { int o = *p; if (o == c) *p = v; return o; }
inline unsigned atomicCAS(unsigned* p, unsigned c, unsigned v) { unsigned o = *p; if (o == c) *p = v; return o; }
template <class T> inline T atomicExch(T* p, T v) { T o = *p; *p = v; return o; }
template <class T> inline T atomicMax(T* p, T v) { T o = *p; if (v > o) *p = v; return o; }
template <class T> inline T atomicMin(T* p, T v) { T o = *p; if (v < o) *p = v; return o; }
template <class T> inline T atomicOr(T* p, T v) { T o = *p; *p = o | v; return o; }
template <class T> inline T atomicAnd(T* p, T v) { T o = *p; *p = o & v; return o; }
using std::fabs; using std::floor; using std::fmax; using std::fmin; using std::ldexp; using std::llrint; using std::max; using std::min; using std::sqrt;
inline float __builtin_amdgcn_rcpf(float x) { return 1.0f / x; }
inline double __builtin_amdgcn_rcp(double x) { return 1.0 / x; }
inline unsigned __float_as_uint(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
inline float __uint_as_float(unsigned u) { float f; std::memcpy(&f, &u, 4); return f; }
inline int __float_as_int(float f) { int u; std::memcpy(&u, &f, 4); return u; }
inline float __int_as_float(int u) { float f; std::memcpy(&f, &u, 4); return f; }
