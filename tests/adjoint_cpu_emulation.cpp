// The adjoint device code (xlb_amd/csrc/adjoint_kernels.hpp) compiled for the host through tests/hip_on_cpu: one adjoint step cell by
// cell with the functions the fused kernel calls for every cell (adjoint_local_cell after cell.hpp's apply_streaming_bc, then the
// gather bits of k_adjoint_gather_mask and adjoint_own_terms for the transposed streaming), and the small kernels launched thread by
// thread.  tests/test_adjoint_kernels_on_cpu.py compares the result with the NumPy restatement.  What it cannot show is the fused
// kernel's own addressing (adjoint_step_kernel.hpp), which tests/test_gpu_adjoint.py covers.
#include "adjoint_kernels.hpp"
#include <vector>
thread_local emulated_dim3 threadIdx, blockIdx, blockDim, gridDim;
using namespace xlb;

template <class K, class... A>
static void launch(K k, size_t n, A... a) {
  blockDim.x = 256;
  for (size_t b = 0; b < (n + 255) / 256; ++b)
    for (unsigned t = 0; t < 256; ++t) { blockIdx.x = (unsigned)b; threadIdx.x = t; k(a...); }
}

struct Case {
  void *f_n, *lam, *mu, *lam_prev;  // (q, nx, ny, nz) C-order in the store dtype, plane_stride = cells
  void* terms;                      // (nx, ny, nz) in the compute dtype
  void *rho_bar, *u_bar;            // MacroscopicAdjoint's inputs in the compute dtype
  const uint8_t* bc;
  const uint32_t* miss;
  int nx, ny, nz, sdt, cdt;
  const uint8_t* kind;   // [256]
  const double* values;  // [256][27]
  double omega;
};

template <class L, class T>
static void step(const Case& c) {
  const size_t cells = (size_t)c.nx * c.ny * c.nz;
  const Dims d{c.nx, c.ny, c.nz};
  const FieldView f0{c.f_n, cells, c.sdt, 0}, lam{c.lam, cells, c.sdt, 0}, mu{c.mu, cells, c.sdt, 0}, out{c.lam_prev, cells, c.sdt, 0};
  std::vector<T> vals(256 * 27);
  for (int i = 0; i < 256 * 27; ++i) vals[i] = (T)c.values[i];
  const BcView<T> tb{c.kind, vals.data(), nullptr, nullptr, 0, nullptr, nullptr, 0};
  // the local transpose: lam -> mu (store dtype) and the omega terms
  for (int x = 0; x < c.nx; ++x)
    for (int y = 0; y < c.ny; ++y)
      for (int z = 0; z < c.nz; ++z) {
        const size_t o = cell_index(f0, d, x, y, z);
        T fs[L::Q], l[L::Q];
        pull_cell<L, T>(f0, d, x, y, z, fs);
        own_cell<L, T>(lam, d, x, y, z, l);
        const unsigned id = c.bc[o];
        if (id != 0u) {
          T pre[L::Q];
          own_cell<L, T>(f0, d, x, y, z, pre);
          apply_streaming_bc<L, T>(tb, id, (unsigned)o, fs, pre, c.miss[o]);
        }
        static_cast<T*>(c.terms)[o] = adjoint_local_cell<L, T>(id ? c.kind[id] : 0u, fs, l, (T)c.omega);
        static_for<L::Q>([&](auto lc) { store_rt<T>(mu, (size_t) decltype(lc)::value * cells + o, l[decltype(lc)::value]); });
      }
  // the transposed streaming: gather what the neighbours did not redirect (their gather bits), add the cell's own redirected part
  std::vector<uint32_t> gmask(cells);
  launch(k_adjoint_gather_mask<L>, cells, c.bc, c.miss, c.kind, gmask.data(), d);
  for (int x = 0; x < c.nx; ++x)
    for (int y = 0; y < c.ny; ++y)
      for (int z = 0; z < c.nz; ++z) {
        const size_t o = cell_index(mu, d, x, y, z);
        T g[L::Q];
        static_for<L::Q>([&](auto lc) {
          constexpr int l = decltype(lc)::value;
          const size_t n = cell_index(mu, d, wrap(x + L::c(0, l), d.nx), wrap(y + L::c(1, l), d.ny), wrap(z + L::c(2, l), d.nz));
          g[l] = ((gmask[o] >> l) & 1u) ? T(0) : load_rt<T>(mu, (size_t)l * cells + n);
        });
        const unsigned id = c.bc[o];
        if (id != 0u) {
          T own[L::Q];
          own_cell<L, T>(mu, d, x, y, z, own);
          adjoint_own_terms<L, T>(c.kind[id], c.miss[o], own, g);
        }
        static_for<L::Q>([&](auto lc) { store_rt<T>(out, (size_t) decltype(lc)::value * cells + o, g[decltype(lc)::value]); });
      }
}

template <class L, class T>
static int go(const Case& c, int what) {
  const size_t cells = (size_t)c.nx * c.ny * c.nz;
  const Dims d{c.nx, c.ny, c.nz};
  if (what == 1) {
    launch(k_macroscopic_adjoint<L, T>, cells, FieldView{c.f_n, cells, c.sdt, 0}, FieldView{c.rho_bar, cells, c.cdt, 0}, FieldView{c.u_bar, cells, c.cdt, 0},
           FieldView{c.lam_prev, cells, c.sdt, 0}, d);
    return 0;
  }
  step<L, T>(c);
  return 0;
}

// what: 0 = one adjoint step (f_n, lam) -> (mu, lam_prev, terms); 1 = k_macroscopic_adjoint (f_n, rho_bar, u_bar) -> lam_prev
extern "C" int adjoint_cpu(int lattice, int what, const Case* c) {
  if (lattice == XLBHIP_D2Q9) return c->cdt == XLBHIP_F32 ? go<D2Q9, float>(*c, what) : go<D2Q9, double>(*c, what);
  if (lattice == XLBHIP_D3Q19) return c->cdt == XLBHIP_F32 ? go<D3Q19, float>(*c, what) : go<D3Q19, double>(*c, what);
  return c->cdt == XLBHIP_F32 ? go<D3Q27, float>(*c, what) : go<D3Q27, double>(*c, what);
}
