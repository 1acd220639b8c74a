// The immersed-boundary coupling kernels (xlb_amd/csrc/ibm_kernels.hpp) compiled for the host through tests/hip_on_cpu: the launches of
// csrc/ibm.hip in the same order, every thread run one after the other.  tests/test_ibm_kernels_on_cpu.py compares the result with the
// NumPy restatement; what it cannot show is the GPU code generation and the behaviour of real atomics.
#include "ibm_kernels.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
thread_local emulated_dim3 threadIdx, blockIdx, blockDim, gridDim;
using namespace xlb;
template <class K, class... A>
static void launch(K k, size_t n, A... a) {
  blockDim.x = 256;
  for (size_t b = 0; b < (n + 255) / 256; ++b)
    for (unsigned t = 0; t < 256; ++t) { blockIdx.x = (unsigned)b; threadIdx.x = t; k(a...); }
}
// C entry: one coupling call on f (q, nx, ny, nz) C-order, plane_stride = cells
template <class L, class T, class S>
static int couple(S* f, int nx, int ny, int nz, int64_t n, const float* pos, const float* area, const float* vel, int sweeps, double tol, double relax,
                  double* F_out, int* sweeps_out, int64_t* fp_out) {
  const size_t cells = (size_t)nx * ny * nz;
  const int64_t cap = (int64_t)std::min<size_t>((size_t)n * 64, cells);
  std::vector<int32_t> map(cells, -1);
  std::vector<uint32_t> list(cap);
  int count = 0;
  std::vector<unsigned long long> W(cap, 0), acc(3 * cap, 0);
  std::vector<unsigned> wbits(cap, 0);
  std::vector<T> u(3 * cap), G(3 * cap, 0), dk(3 * n), F(3 * n, 0);
  IbmControl ctl;
  std::memset(&ctl, 0, sizeof ctl);
  Dims d{nx, ny, nz};
  launch(k_ibm_mark<T>, (size_t)n * 64, pos, n, d, map.data(), list.data(), &count, cap);
  launch(k_ibm_wmax<T>, (size_t)n * 64, pos, n, d, (const int32_t*)map.data(), wbits.data(), cap);
  launch(k_ibm_weights<T>, (size_t)n * 64, pos, n, d, (const int32_t*)map.data(), (const unsigned*)wbits.data(), W.data(), cap);
  launch(k_ibm_moments<L, T, S>, (size_t)cap, (const S*)f, cells, (const uint32_t*)list.data(), (const int*)&count, cap, u.data());
  launch(k_ibm_interp<T>, (size_t)n, pos, vel, n, d, (const int32_t*)map.data(), cap, (const T*)u.data(), dk.data(), F.data());
  const int res = tol > 0 ? 1 : 0;
  for (int it = 0; it < sweeps; ++it) {
    if (it > 0) launch(k_ibm_spread<T>, (size_t)n * 64, it, res, (const IbmControl*)&ctl, pos, area, (const T*)F.data(), n, d, (const int32_t*)map.data(), cap, (const unsigned*)wbits.data(), acc.data());
    launch(k_ibm_correct<T>, (size_t)cap, it, res, (const IbmControl*)&ctl, (const int*)&count, cap, (const unsigned*)wbits.data(), (const unsigned long long*)W.data(), acc.data(), (const T*)u.data(), (T)relax, G.data());
    launch(k_ibm_update<T>, (size_t)n, it, res, &ctl, n, (const T*)dk.data(), F.data(), (T)(tol * tol));
  }
  launch(k_ibm_apply<L, T, S>, (size_t)cap, f, cells, (const uint32_t*)list.data(), (const int*)&count, cap, (const T*)G.data());
  for (int64_t i = 0; i < 3 * n; ++i) F_out[i] = (double)F[i];
  *sweeps_out = ctl.sweeps;
  *fp_out = count;
  // clear must leave the map empty
  launch(k_ibm_clear, (size_t)cap, map.data(), (const uint32_t*)list.data(), (const int*)&count, cap);
  for (size_t c = 0; c < cells; ++c) if (map[c] != -1) return 2;
  return 0;
}
extern "C" int couple_cpu(int lattice, int cdt, int sdt, void* f, int nx, int ny, int nz, int64_t n, const float* pos, const float* area, const float* vel,
                          int sweeps, double tol, double relax, double* F_out, int* sweeps_out, int64_t* fp_out) {
#define GO(L) \
  if (cdt == 1) return couple<L, float, float>((float*)f, nx, ny, nz, n, pos, area, vel, sweeps, tol, relax, F_out, sweeps_out, fp_out); \
  if (sdt == 1) return couple<L, double, float>((float*)f, nx, ny, nz, n, pos, area, vel, sweeps, tol, relax, F_out, sweeps_out, fp_out); \
  return couple<L, double, double>((double*)f, nx, ny, nz, n, pos, area, vel, sweeps, tol, relax, F_out, sweeps_out, fp_out);
  if (lattice == 1) { GO(D3Q19) } else { GO(D3Q27) }
}
