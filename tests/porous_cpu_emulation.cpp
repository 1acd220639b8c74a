// The porous device code (xlb_amd/csrc/porous_kernels.hpp) compiled for the host through tests/hip_on_cpu: one forward step and one
// adjoint step cell by cell with the functions the fused kernels call for every cell (porous_collide / porous_adjoint_local_cell after
// cell.hpp's apply_streaming_bc, then the gather bits of k_adjoint_gather_mask and adjoint_own_terms for the transposed streaming).
// tests/test_porous_kernels_on_cpu.py compares the result with the NumPy restatement.  What it cannot show is the fused kernels' own
// addressing (porous_step_kernel.hpp), which tests/test_gpu_porous.py covers.
#include "porous_kernels.hpp"
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
  void *f_n, *f_out, *lam, *mu, *lam_prev;  // (q, nx, ny, nz) C-order in the store dtype, plane_stride = cells
  void *alpha, *terms, *galpha;             // (nx, ny, nz) in the compute dtype
  const uint8_t* bc;
  const uint32_t* miss;
  int nx, ny, nz, sdt, cdt;
  const uint8_t* kind;   // [256]
  const double* values;  // [256][27]
  double omega;
};

// f* of one cell: the pull and the cell's streaming rule
template <class L, class T>
static unsigned post_stream(const Case& c, const BcView<T>& tb, const FieldView& f0, const Dims& d, int x, int y, int z, size_t o, T (&fs)[L::Q]) {
  pull_cell<L, T>(f0, d, x, y, z, fs);
  const unsigned id = c.bc[o];
  if (id != 0u) {
    T pre[L::Q];
    own_cell<L, T>(f0, d, x, y, z, pre);
    apply_streaming_bc<L, T>(tb, id, (unsigned)o, fs, pre, c.miss[o]);
  }
  return id ? c.kind[id] : 0u;
}

template <class L, class T>
static int go(const Case& c) {
  const size_t cells = (size_t)c.nx * c.ny * c.nz;
  const Dims d{c.nx, c.ny, c.nz};
  const FieldView f0{c.f_n, cells, c.sdt, 0}, f1{c.f_out, cells, c.sdt, 0}, lam{c.lam, cells, c.sdt, 0}, mu{c.mu, cells, c.sdt, 0},
      out{c.lam_prev, cells, c.sdt, 0};
  const T* alpha = static_cast<const T*>(c.alpha);
  std::vector<T> vals(256 * 27);
  for (int i = 0; i < 256 * 27; ++i) vals[i] = (T)c.values[i];
  const BcView<T> tb{c.kind, vals.data(), nullptr, nullptr, 0, nullptr, nullptr, 0};
  for (int x = 0; x < c.nx; ++x)
    for (int y = 0; y < c.ny; ++y)
      for (int z = 0; z < c.nz; ++z) {
        const size_t o = cell_index(f0, d, x, y, z);
        T fs[L::Q], f[L::Q], l[L::Q];
        const unsigned kind = post_stream<L, T>(c, tb, f0, d, x, y, z, o, fs);
        // the forward step
        static_for<L::Q>([&](auto lc) { f[decltype(lc)::value] = fs[decltype(lc)::value]; });
        if (kind == XLBHIP_BC_FULLWAY_BB)
          adjoint_fullway<L, T>(f);
        else
          porous_collide<L, T>(f, (T)c.omega, alpha[o]);
        static_for<L::Q>([&](auto lc) { store_rt<T>(f1, (size_t) decltype(lc)::value * cells + o, f[decltype(lc)::value]); });
        // the local transpose: lam -> mu (store dtype), the omega terms and the alpha terms
        own_cell<L, T>(lam, d, x, y, z, l);
        const PorousTerms<T> t = porous_adjoint_local_cell<L, T>(kind, fs, l, (T)c.omega, alpha[o]);
        static_cast<T*>(c.terms)[o] = t.omega;
        static_cast<T*>(c.galpha)[o] = t.alpha;
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
  return 0;
}

// one forward step f_n -> f_out and one adjoint step (f_n, lam) -> (mu, lam_prev, terms, galpha) at alpha
extern "C" int porous_cpu(int lattice, const Case* c) {
  if (lattice == XLBHIP_D2Q9) return c->cdt == XLBHIP_F32 ? go<D2Q9, float>(*c) : go<D2Q9, double>(*c);
  if (lattice == XLBHIP_D3Q19) return c->cdt == XLBHIP_F32 ? go<D3Q19, float>(*c) : go<D3Q19, double>(*c);
  return c->cdt == XLBHIP_F32 ? go<D3Q27, float>(*c) : go<D3Q27, double>(*c);
}
