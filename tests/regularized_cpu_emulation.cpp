// The regularised collisions of xlb_amd/csrc/cell.hpp compiled for the host through tests/hip_on_cpu: one periodic step cell by cell —
// the pull of ops_kernels.hpp, collide<> with the COLL value the stepper's launch picks, the store in the store dtype — and the
// stand-alone operator's arithmetic (moments of f, then regularized<>).  tests/test_regularized_kernels_on_cpu.py compares both with the
// NumPy restatement bit for bit.  What it cannot show is the step kernel's addressing and boundary rules and the GPU's code generation
// (tests/test_gpu_regularized.py).
#include "ops_kernels.hpp"
thread_local emulated_dim3 threadIdx, blockIdx, blockDim, gridDim;
using namespace xlb;

struct Case {
  void *f0, *f1;  // (q, nx, ny, nz) C-order in the store dtype, plane_stride = cells
  int nx, ny, nz, sdt, cdt;
  int collision;  // public id: XLBHIP_REGULARIZED_BGK / XLBHIP_RECURSIVE_REGULARIZED_BGK
  int forced;
  double force[3], omega;
};

template <class L, class T, int COLL>
static int step(const Case& c) {
  const size_t cells = (size_t)c.nx * c.ny * c.nz;
  const Dims d{c.nx, c.ny, c.nz};
  const FieldView f0{c.f0, cells, c.sdt, 0}, f1{c.f1, cells, c.sdt, 0};
  CollideExtra ex = {};
  for (int k = 0; k < 3; ++k) ex.force[k] = c.force[k];
  for (int x = 0; x < c.nx; ++x)
    for (int y = 0; y < c.ny; ++y)
      for (int z = 0; z < c.nz; ++z) {
        T f[L::Q];
        pull_cell<L, T>(f0, d, x, y, z, f);
        collide<L, T, COLL>(f, (T)c.omega, ex);
        const size_t o = cell_index(f1, d, x, y, z);
        static_for<L::Q>([&](auto lc) { store_rt<T>(f1, (size_t) decltype(lc)::value * cells + o, f[decltype(lc)::value]); });
      }
  return 0;
}

template <class L, class T>
static int by_collision(const Case& c) {
  constexpr int RR = COLL_REGULARIZED | COLL_RECURSIVE;
  switch (coll_of_public(c.collision) | (c.forced ? COLL_FORCED : 0)) {
    case COLL_REGULARIZED: return step<L, T, COLL_REGULARIZED>(c);
    case COLL_REGULARIZED | COLL_FORCED: return step<L, T, COLL_REGULARIZED | COLL_FORCED>(c);
    case RR: return step<L, T, RR>(c);
    case RR | COLL_FORCED: return step<L, T, RR | COLL_FORCED>(c);
  }
  return 1;
}

// one periodic step f0 -> f1
extern "C" int regularized_cpu(int lattice, const Case* c) {
  if (lattice == XLBHIP_D2Q9) return c->cdt == XLBHIP_F32 ? by_collision<D2Q9, float>(*c) : by_collision<D2Q9, double>(*c);
  if (lattice == XLBHIP_D3Q19) return c->cdt == XLBHIP_F32 ? by_collision<D3Q19, float>(*c) : by_collision<D3Q19, double>(*c);
  return c->cdt == XLBHIP_F32 ? by_collision<D3Q27, float>(*c) : by_collision<D3Q27, double>(*c);
}

template <class L, class T, int COLL>
static void collide_cells(const Case& c) {
  // f0: f, f1: feq in, f' out (both in the compute dtype)
  const size_t cells = (size_t)c.nx * c.ny * c.nz;
  T *pf = static_cast<T*>(c.f0), *pe = static_cast<T*>(c.f1);
  for (size_t o = 0; o < cells; ++o) {
    T f[L::Q], fe[L::Q], rho, u[3];
    for (int l = 0; l < L::Q; ++l) {
      f[l] = pf[(size_t)l * cells + o];
      fe[l] = pe[(size_t)l * cells + o];
    }
    moments<L, T>(f, rho, u);
    regularized<L, T, (COLL & COLL_RECURSIVE) != 0 ? 3 : 2>(f, fe, rho, u, (T)c.omega);
    for (int l = 0; l < L::Q; ++l) pe[(size_t)l * cells + o] = f[l];
  }
}

template <class L, class T>
static int operator_by_collision(const Case& c) {
  if (c.collision == XLBHIP_REGULARIZED_BGK)
    collide_cells<L, T, COLL_REGULARIZED>(c);
  else
    collide_cells<L, T, COLL_REGULARIZED | COLL_RECURSIVE>(c);
  return 0;
}

// the stand-alone operator on (f, feq): what k_collide does per cell
extern "C" int regularized_operator_cpu(int lattice, const Case* c) {
  if (lattice == XLBHIP_D2Q9) return c->cdt == XLBHIP_F32 ? operator_by_collision<D2Q9, float>(*c) : operator_by_collision<D2Q9, double>(*c);
  if (lattice == XLBHIP_D3Q19) return c->cdt == XLBHIP_F32 ? operator_by_collision<D3Q19, float>(*c) : operator_by_collision<D3Q19, double>(*c);
  return c->cdt == XLBHIP_F32 ? operator_by_collision<D3Q27, float>(*c) : operator_by_collision<D3Q27, double>(*c);
}
