// The Shan-Chen device code (xlb_amd/csrc/multiphase_kernels.hpp) compiled for the host through tests/hip_on_cpu: one step cell by cell
// in the two passes of the device (psi of every cell, then force and collision) with the functions the row kernels call for every cell
// (psi_of, psi_force, multiphase_collide_cell, multiphase_velocity; the fluid's streaming rule through cell.hpp's apply_streaming_bc).
// tests/test_multiphase_kernels_on_cpu.py compares the result with the NumPy restatement.  What it cannot show is the row kernels' own
// addressing (multiphase_step_kernel.hpp), which tests/test_gpu_multiphase.py covers.
#include "multiphase_kernels.hpp"
#include <vector>
thread_local emulated_dim3 threadIdx, blockIdx, blockDim, gridDim;
using namespace xlb;

struct Case {
  void *f0, *f1;                  // (q, nx, ny, nz) C-order in the store dtype, plane_stride = cells
  void *psi, *rho, *u, *force;    // (1 | 1 | d | d, nx, ny, nz) in the compute dtype
  const uint8_t* bc;
  const uint32_t* miss;
  int nx, ny, nz, sdt, cdt;
  const uint8_t* kind;     // [256]
  const double* values;    // [256][27]
  const double* psi_wall;  // [256]
  int form;
  double g, par[4], fvec[3], omega;
};

template <class L, class T>
static void front(const Case& c, const FieldView& f0, const Dims& d, const BcView<T>& tb, int x, int y, int z, T (&f)[L::Q], unsigned& id, unsigned& m,
                  bool& fullway) {
  const size_t o = cell_index(f0, d, x, y, z);
  pull_cell<L, T>(f0, d, x, y, z, f);
  id = c.bc[o];
  m = 0u;
  fullway = false;
  if (id != 0u) {
    m = c.miss[o];
    if (c.kind[id] == XLBHIP_BC_HALFWAY_BB) {
      T pre[L::Q];
      own_cell<L, T>(f0, d, x, y, z, pre);
      apply_streaming_bc<L, T>(tb, id, (unsigned)o, f, pre, m);
    }
    fullway = c.kind[id] == XLBHIP_BC_FULLWAY_BB;
  }
}

template <class L, class T>
static int step(const Case& c) {
  const size_t cells = (size_t)c.nx * c.ny * c.nz;
  const Dims d{c.nx, c.ny, c.nz};
  const FieldView f0{c.f0, cells, c.sdt, 0}, f1{c.f1, cells, c.sdt, 0};
  std::vector<T> vals(256 * 27), pw(256);
  for (int i = 0; i < 256 * 27; ++i) vals[i] = (T)c.values[i];
  for (int i = 0; i < 256; ++i) pw[i] = (T)c.psi_wall[i];
  const BcView<T> tb{c.kind, vals.data(), nullptr, nullptr, 0, nullptr, nullptr, 0};
  PsiModel<T> mo;
  mo.form = c.form;
  mo.neg_g = (T)(-c.g);
  for (int k = 0; k < 4; ++k) mo.par[k] = (T)c.par[k];
  for (int k = 0; k < 3; ++k) mo.force[k] = (T)c.fvec[k];
  T* psi = static_cast<T*>(c.psi);
  T *rho_out = static_cast<T*>(c.rho), *u_out = static_cast<T*>(c.u), *force_out = static_cast<T*>(c.force);
  // pass 1: psi
  for (int x = 0; x < c.nx; ++x)
    for (int y = 0; y < c.ny; ++y)
      for (int z = 0; z < c.nz; ++z) {
        T f[L::Q], rho, u[3];
        unsigned id, m;
        bool fullway;
        front<L, T>(c, f0, d, tb, x, y, z, f, id, m, fullway);
        moments<L, T>(f, rho, u);
        const bool wall = fullway || id == BC_ID_SOLID;
        psi[cell_index(f0, d, x, y, z)] = wall ? pw[id] : psi_of<T>(mo, rho);
      }
  // pass 2: force, collision, outputs
  for (int x = 0; x < c.nx; ++x)
    for (int y = 0; y < c.ny; ++y)
      for (int z = 0; z < c.nz; ++z) {
        const size_t o = cell_index(f0, d, x, y, z);
        T f[L::Q], rho, u[3], F[3], nb[L::Q];
        unsigned id, m;
        bool fullway;
        front<L, T>(c, f0, d, tb, x, y, z, f, id, m, fullway);
        moments<L, T>(f, rho, u);
        nb[0] = T(0);
        static_for<L::Q - 1>([&](auto ic) {
          constexpr int i = decltype(ic)::value + 1;
          nb[i] = psi[cell_index(f0, d, wrap(x + L::c(0, i), d.nx), wrap(y + L::c(1, i), d.ny), wrap(z + L::c(2, i), d.nz))];
        });
        const bool wall = fullway || id == BC_ID_SOLID;
        psi_force<L, T>(mo, psi[o], nb, m, id != 0u ? pw[id] : T(0), wall, F);
        rho_out[o] = rho;
        static_for<L::D>([&](auto dc) {
          constexpr int k = decltype(dc)::value, a = k + (3 - L::D);
          u_out[(size_t)k * cells + o] = multiphase_velocity<T>(u[a], F[a], rho);
          force_out[(size_t)k * cells + o] = F[a];
        });
        multiphase_collide_cell<L, T>(f, fullway, (T)c.omega, rho, F, mo);
        static_for<L::Q>([&](auto lc) { store_rt<T>(f1, (size_t) decltype(lc)::value * cells + o, f[decltype(lc)::value]); });
      }
  return 0;
}

// one step f0 -> f1, with psi, rho, the physical velocity and the force of f0's post-streaming state
extern "C" int multiphase_cpu(int lattice, const Case* c) {
  if (lattice == XLBHIP_D2Q9) return c->cdt == XLBHIP_F32 ? step<D2Q9, float>(*c) : step<D2Q9, double>(*c);
  if (lattice == XLBHIP_D3Q19) return c->cdt == XLBHIP_F32 ? step<D3Q19, float>(*c) : step<D3Q19, double>(*c);
  return c->cdt == XLBHIP_F32 ? step<D3Q27, float>(*c) : step<D3Q27, double>(*c);
}
