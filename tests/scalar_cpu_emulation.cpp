// The scalar-transport device code (xlb_amd/csrc/scalar_kernels.hpp) compiled for the host through tests/hip_on_cpu: one coupled step
// cell by cell with the functions the fused kernel calls for every cell (scalar_apply_rule, scalar_collide_cell; the fluid's
// streaming rules through cell.hpp's apply_streaming_bc), then the fluid's outflow pass, and the two small kernels launched thread by
// thread.  tests/test_scalar_kernels_on_cpu.py compares the result with the NumPy restatement.  What it cannot show is the fused
// kernel's own addressing (scalar_step_kernel.hpp: vector loads, row ends), which tests/test_gpu_scalar_transport.py covers.
#include "scalar_kernels.hpp"
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
  void *f0, *f1, *g0, *g1, *phi;  // (q | qs | 1, nx, ny, nz) C-order, plane_stride = cells
  const uint8_t* bc;
  const uint32_t* miss;
  int nx, ny, nz, sdt, cdt, forced;
  const uint8_t* kind;    // [256]
  const double* values;   // [256][27]
  const uint8_t* rule;    // [256]
  const double* rvalue;   // [256]
  double omega, omega_s;
  ScalarCoupling cp;
};

template <class L, class T, int COLL>
static void step(const Case& c) {
  typedef ScalarSet<L> G;
  const size_t cells = (size_t)c.nx * c.ny * c.nz;
  const Dims d{c.nx, c.ny, c.nz};
  const FieldView f0{c.f0, cells, c.sdt, 0}, f1{c.f1, cells, c.sdt, 0}, g0{c.g0, cells, c.sdt, 0}, g1{c.g1, cells, c.sdt, 0};
  const FieldView bcv{(void*)c.bc, cells, XLBHIP_U8, 0}, mv{(void*)c.miss, cells, XLBHIP_MISSING, 0};
  std::vector<T> vals(256 * 27), rv(256);
  for (int i = 0; i < 256 * 27; ++i) vals[i] = (T)c.values[i];
  for (int i = 0; i < 256; ++i) rv[i] = (T)c.rvalue[i];
  const BcView<T> tb{c.kind, vals.data(), nullptr, nullptr, 0, nullptr, nullptr, 0};
  const CollideExtra ex{{0, 0, 0}, 0.17};
  bool outflow = false;
  for (int x = 0; x < c.nx; ++x)
    for (int y = 0; y < c.ny; ++y)
      for (int z = 0; z < c.nz; ++z) {
        const size_t o = cell_index(f0, d, x, y, z);
        T f[L::Q], g[G::Q];
        pull_cell<L, T>(f0, d, x, y, z, f);
        static_for<G::Q>([&](auto jc) {
          constexpr int j = decltype(jc)::value;
          constexpr int l = G::dir(j);
          g[j] = load_rt<T>(g0, (size_t)j * cells + cell_index(g0, d, wrap(x - L::c(0, l), d.nx), wrap(y - L::c(1, l), d.ny), wrap(z - L::c(2, l), d.nz)));
        });
        const unsigned id = c.bc[o];
        bool fullway = false;
        if (id != 0u) {
          const unsigned m = c.miss[o];
          T pre[L::Q], gpre[G::Q];
          own_cell<L, T>(f0, d, x, y, z, pre);
          apply_streaming_bc<L, T>(tb, id, (unsigned)o, f, pre, m);
          fullway = c.kind[id] == XLBHIP_BC_FULLWAY_BB;
          outflow = outflow || c.kind[id] == XLBHIP_BC_EXTRAPOLATION_OUTFLOW;
          static_for<G::Q>([&](auto jc) { gpre[decltype(jc)::value] = load_rt<T>(g0, (size_t) decltype(jc)::value * cells + o); });
          scalar_apply_rule<L, T>(c.rule[id], rv[id], m, gpre, g);
        }
        scalar_collide_cell<L, T, COLL>(f, g, fullway, (T)c.omega, (T)c.omega_s, ex, c.cp);
        static_for<L::Q>([&](auto lc) { store_rt<T>(f1, (size_t) decltype(lc)::value * cells + o, f[decltype(lc)::value]); });
        static_for<G::Q>([&](auto jc) { store_rt<T>(g1, (size_t) decltype(jc)::value * cells + o, g[decltype(jc)::value]); });
      }
  if (outflow) launch(k_outflow_aux<L, T>, cells, f0, f1, bcv, mv, d, tb);
}

template <class L, class T>
static int go(const Case& c, int what, double phi0) {
  const size_t cells = (size_t)c.nx * c.ny * c.nz;
  const Dims d{c.nx, c.ny, c.nz};
  if (what == 1) {  // g0 = geq(phi | phi0, u(f0))
    launch(k_scalar_init<L, T>, cells, FieldView{c.f0, cells, c.sdt, 0}, FieldView{c.phi, cells, c.cdt, 0}, (T)phi0, FieldView{c.g0, cells, c.sdt, 0}, d);
    return 0;
  }
  if (what == 2) {  // phi = sum g0
    launch(k_scalar_moment<L, T>, cells, FieldView{c.g0, cells, c.sdt, 0}, FieldView{c.phi, cells, c.cdt, 0}, d);
    return 0;
  }
  if (c.forced)
    step<L, T, XLBHIP_BGK | COLL_FORCED>(c);
  else
    step<L, T, XLBHIP_BGK>(c);
  return 0;
}

// what: 0 = one coupled BGK step (f0, g0) -> (f1, g1); 1 = k_scalar_init; 2 = k_scalar_moment
extern "C" int scalar_cpu(int lattice, int what, double phi0, const Case* c) {
  if (lattice == XLBHIP_D2Q9) return c->cdt == XLBHIP_F32 ? go<D2Q9, float>(*c, what, phi0) : go<D2Q9, double>(*c, what, phi0);
  if (lattice == XLBHIP_D3Q19) return c->cdt == XLBHIP_F32 ? go<D3Q19, float>(*c, what, phi0) : go<D3Q19, double>(*c, what, phi0);
  return c->cdt == XLBHIP_F32 ? go<D3Q27, float>(*c, what, phi0) : go<D3Q27, double>(*c, what, phi0);
}
