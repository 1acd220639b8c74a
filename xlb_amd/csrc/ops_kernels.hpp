// Whole-field operator kernels (one thread per cell) and the small field utilities every unit shares (the boundary maskers'
// kernels are in masker_kernels.hpp).  The operators mirror the reference's stand-alone operator launches; the
// per-timestep hot path is the fused kernel in step_kernel.hpp.
#pragma once
#include "cell.hpp"

namespace xlb {

// Runtime-typed view of a field on the device.
struct FieldView {
  void* data;
  size_t plane_stride;
  int dtype;
  int halo;
};

struct Dims {
  int nx, ny, nz;
};

template <class T>
__device__ __forceinline__ T load_rt(const FieldView& v, size_t i) {
  switch (v.dtype) {
    case XLBHIP_F64: return static_cast<T>(static_cast<const double*>(v.data)[i]);
    case XLBHIP_F32: return static_cast<T>(static_cast<const float*>(v.data)[i]);
    case XLBHIP_F16: return static_cast<T>(static_cast<const _Float16*>(v.data)[i]);
    default: return static_cast<T>(static_cast<const uint8_t*>(v.data)[i]);
  }
}
template <class T>
__device__ __forceinline__ void store_rt(const FieldView& v, size_t i, T x) {
  switch (v.dtype) {
    case XLBHIP_F64: static_cast<double*>(v.data)[i] = static_cast<double>(x); break;
    case XLBHIP_F32: static_cast<float*>(v.data)[i] = static_cast<float>(x); break;
    case XLBHIP_F16: static_cast<_Float16*>(v.data)[i] = static_cast<_Float16>(x); break;
    default: static_cast<uint8_t*>(v.data)[i] = static_cast<uint8_t>(x); break;
  }
}

__device__ __forceinline__ bool cell_of_thread(const Dims& d, int& x, int& y, int& z) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)d.nx * d.ny * d.nz;
  if (t >= n) return false;
  z = (int)(t % d.nz);
  const size_t r = t / d.nz;
  y = (int)(r % d.ny);
  x = (int)(r / d.ny);
  return true;
}
__device__ __forceinline__ size_t cell_index(const FieldView& v, const Dims& d, int x, int y, int z) {
  return ((size_t)(x + v.halo) * d.ny + y) * d.nz + z;
}
__device__ __forceinline__ int wrap(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

// Stream()(f_0, f_1): stream.py:29-62 / :96-110 — periodic pull
template <class L>
__global__ void k_stream(FieldView src, FieldView dst, Dims d) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  const size_t o = cell_index(dst, d, x, y, z);
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    const int xs = src.halo ? x - L::c(0, l) : wrap(x - L::c(0, l), d.nx);
    const int ys = wrap(y - L::c(1, l), d.ny);
    const int zs = wrap(z - L::c(2, l), d.nz);
    const size_t i = (size_t)l * src.plane_stride + cell_index(src, d, xs, ys, zs);
    // pure data movement: go through double, exact for every storage type
    store_rt<double>(dst, (size_t)l * dst.plane_stride + o, load_rt<double>(src, i));
  });
}

// QuadraticEquilibrium()(rho, u, f): quadratic_equilibrium.py:23-30
template <class L, class T>
__global__ void k_equilibrium(FieldView rho, FieldView u, FieldView f, Dims d) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  const T r = load_rt<T>(rho, cell_index(rho, d, x, y, z));
  T uu[3] = {T(0), T(0), T(0)};
  static_for<L::D>([&](auto ac) {
    constexpr int a = decltype(ac)::value;
    uu[a + 3 - L::D] = load_rt<T>(u, (size_t)a * u.plane_stride + cell_index(u, d, x, y, z));
  });
  T feq[L::Q];
  equilibrium<L, T>(r, uu, feq);
  const size_t o = cell_index(f, d, x, y, z);
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    store_rt<T>(f, (size_t)l * f.plane_stride + o, feq[l]);
  });
}

// Macroscopic()(f, rho, u): macroscopic.py:21-26
template <class L, class T>
__global__ void k_macroscopic(FieldView f, FieldView rho, FieldView u, Dims d) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  T ff[L::Q];
  const size_t i = cell_index(f, d, x, y, z);
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    ff[l] = load_rt<T>(f, (size_t)l * f.plane_stride + i);
  });
  T r, uu[3];
  moments<L, T>(ff, r, uu);
  if (rho.data) store_rt<T>(rho, cell_index(rho, d, x, y, z), r);
  if (u.data) {
    static_for<L::D>([&](auto ac) {
      constexpr int a = decltype(ac)::value;
      store_rt<T>(u, (size_t)a * u.plane_stride + cell_index(u, d, x, y, z), uu[a + 3 - L::D]);
    });
  }
}

// SecondMoment()(f, pi): second_moment.py:55
template <class L, class T>
__global__ void k_second_moment(FieldView f, FieldView pi, Dims d) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  T ff[L::Q];
  const size_t i = cell_index(f, d, x, y, z);
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    ff[l] = load_rt<T>(f, (size_t)l * f.plane_stride + i);
  });
  T p[6];
  second_moment<L, T>(ff, p);
  static_for<n_pi<L>()>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    store_rt<T>(pi, (size_t)k * pi.plane_stride + cell_index(pi, d, x, y, z), p[k]);
  });
}

// BGK()/KBC()(f, feq, fout, omega): bgk.py:27-32, kbc.py:40-79
template <class L, class T, int COLL>
__global__ void k_collide(FieldView f, FieldView feq, FieldView fout, Dims d, T omega, T smag_cs) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  T ff[L::Q], fe[L::Q];
  const size_t i = cell_index(f, d, x, y, z), j = cell_index(feq, d, x, y, z);
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    ff[l] = load_rt<T>(f, (size_t)l * f.plane_stride + i);
    fe[l] = load_rt<T>(feq, (size_t)l * feq.plane_stride + j);
  });
  if constexpr (COLL == XLBHIP_BGK)
    bgk<L, T>(ff, fe, omega);
  else if constexpr (COLL == XLBHIP_KBC)
    kbc<L, T>(ff, fe, omega);
  else if constexpr (COLL == XLBHIP_SMAGORINSKY_LES_BGK)
    smagorinsky<L, T>(ff, fe, omega, smag_cs);
  else {
    static_assert((COLL & 3) == COLL_REGULARIZED, "collision not built for the stand-alone operator");
    T rho, u[3];
    moments<L, T>(ff, rho, u);
    regularized<L, T, (COLL & COLL_RECURSIVE) != 0 ? 3 : 2>(ff, fe, rho, u, omega);
  }
  const size_t o = cell_index(fout, d, x, y, z);
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    store_rt<T>(fout, (size_t)l * fout.plane_stride + o, ff[l]);
  });
}

template <class T>
struct BcValues {
  T v[27];  // the constants of one BC in the compute dtype (converted on the host), passed by value
};

// The stepper's boundary tables: kind and constants by id, per-cell prescribed values and HybridBC wall-distance weights by sorted storage cell
template <class T>
struct BcView {
  const uint8_t* kind;  // [256]
  const T* values;      // [256][27]
  const uint32_t* prof_keys;
  const T* prof_vals;
  int n_prof;
  const uint32_t* dist_keys;
  const float* dist_vals;
  int n_dist;
};

// apply_streaming_bc for cell `key` (storage cell index) of BC `id`, its wall velocity and weights looked up in the tables
template <class L, class T>
__device__ __forceinline__ void apply_streaming_bc(const BcView<T>& tb, unsigned id, unsigned key, T (&f)[L::Q], const T (&pre)[L::Q], unsigned m) {
  const unsigned kind = tb.kind[id];
  const T* val = tb.values + id * 27u;
  T uw[5] = {T(0), T(0), T(0), T(0), T(0)};
  if (kind == XLBHIP_BC_HALFWAY_BB_PROFILE)
    profile_entry<T>(tb.prof_keys, tb.prof_vals, tb.n_prof, key, uw);
  else if (bc_is_extended(kind))
    wall_velocity<T>(val, tb.prof_keys, tb.prof_vals, tb.n_prof, key, uw);
  const float* wgt = bc_is_hybrid(kind) ? wall_weights<L, T>(val, tb.dist_keys, tb.dist_vals, tb.n_dist, key) : nullptr;
  apply_streaming_bc<L, T>(kind, f, pre, m, val, uw, wgt);
}

// bc(f_pre, f_post, bc_mask, missing_mask) -> f_post: boundary_condition.py:146-180.  Stand-alone operator: the prescribed
// values of a Zou-He / Regularized BC come from the call's own table when the host flagged them (PROF_FLAG), HybridBC has no distances.
template <class L, class T>
__global__ void __launch_bounds__(BC_BLOCK) k_apply_bc(int id, int kind, BcValues<T> vals, FieldView f_pre, FieldView f_post, FieldView bc, FieldView miss,
                           Dims d, const uint32_t* prof_keys, const T* prof_vals, int n_prof) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  const uint8_t b = static_cast<const uint8_t*>(bc.data)[cell_index(bc, d, x, y, z)];
  if (b != id) return;
  const size_t ip = cell_index(f_pre, d, x, y, z), io = cell_index(f_post, d, x, y, z);
  unsigned m = 0;
  if (bc_reads_missing(kind)) m = static_cast<const uint32_t*>(miss.data)[cell_index(miss, d, x, y, z)];
  T ff[L::Q], pre[L::Q];
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    ff[l] = load_rt<T>(f_post, (size_t)l * f_post.plane_stride + io);
    pre[l] = load_rt<T>(f_pre, (size_t)l * f_pre.plane_stride + ip);
  });
  // halfway walls and the outflow's streaming part replace the missing directions only: the others are not written
  unsigned written = (kind == XLBHIP_BC_HALFWAY_BB || kind == XLBHIP_BC_EXTRAPOLATION_OUTFLOW) ? m : ~0u;
  if (kind == XLBHIP_BC_FULLWAY_BB) {
    // bc_fullway_bounce_back.py:52-56 (post-collision)
    static_for<L::Q>([&](auto lc) { ff[decltype(lc)::value] = pre[opp<L>(decltype(lc)::value)]; });
  } else {
    T uw[5] = {T(0), T(0), T(0), T(0), T(0)};
    if (bc_is_extended(kind)) wall_velocity<T>(vals.v, prof_keys, prof_vals, n_prof, (unsigned)cell_index(bc, d, x, y, z), uw);
    apply_streaming_bc<L, T>((unsigned)kind, ff, pre, m, vals.v, uw, nullptr);
  }
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    if ((written >> l) & 1u) store_rt<T>(f_post, (size_t)l * f_post.plane_stride + io, ff[l]);
  });
}

// ---- post-processing: Vorticity and QCriterion (postprocess/vorticity.py:30-84, q_criterion.py:36-131) ----
// The reference has these for its kernel backend only: one thread per cell of the box shrunk by one cell per side,
// nothing is written where any of the six face neighbours carries a boundary id, central differences elsewhere.
// MODE 0: out_a = vorticity (3 components), out_b = |vorticity|;  MODE 1: out_a = |vorticity|, out_b = Q.
template <class T, int MODE>
__global__ void k_velocity_gradient(FieldView u, FieldView bc, FieldView out_a, FieldView out_b, Dims d) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  if (x < 1 || y < 1 || z < 1 || x > d.nx - 2 || y > d.ny - 2 || z > d.nz - 2) return;
  const uint8_t* b = static_cast<const uint8_t*>(bc.data);
  if (b[cell_index(bc, d, x + 1, y, z)] != 0 || b[cell_index(bc, d, x, y + 1, z)] != 0 || b[cell_index(bc, d, x, y, z + 1)] != 0 ||
      b[cell_index(bc, d, x - 1, y, z)] != 0 || b[cell_index(bc, d, x, y - 1, z)] != 0 || b[cell_index(bc, d, x, y, z - 1)] != 0)
    return;
  auto U = [&](int a, int i, int j, int k) { return load_rt<T>(u, (size_t)a * u.plane_stride + cell_index(u, d, i, j, k)); };
  const T two = T(2.0), half = T(0.5);
  const T u_x_dy = (U(0, x, y + 1, z) - U(0, x, y - 1, z)) / two;
  const T u_x_dz = (U(0, x, y, z + 1) - U(0, x, y, z - 1)) / two;
  const T u_y_dx = (U(1, x + 1, y, z) - U(1, x - 1, y, z)) / two;
  const T u_y_dz = (U(1, x, y, z + 1) - U(1, x, y, z - 1)) / two;
  const T u_z_dx = (U(2, x + 1, y, z) - U(2, x - 1, y, z)) / two;
  const T u_z_dy = (U(2, x, y + 1, z) - U(2, x, y - 1, z)) / two;
  const T vx = u_z_dy - u_y_dz, vy = u_x_dz - u_z_dx, vz = u_y_dx - u_x_dy;
  const T mag = sqrt((vx * vx + vy * vy) + vz * vz);
  const size_t oa = cell_index(out_a, d, x, y, z), ob = cell_index(out_b, d, x, y, z);
  if constexpr (MODE == 0) {
    store_rt<T>(out_a, oa, vx);
    store_rt<T>(out_a, out_a.plane_stride + oa, vy);
    store_rt<T>(out_a, 2 * out_a.plane_stride + oa, vz);
    store_rt<T>(out_b, ob, mag);
  } else {
    const T u_x_dx = (U(0, x + 1, y, z) - U(0, x - 1, y, z)) / two;
    const T u_y_dy = (U(1, x, y + 1, z) - U(1, x, y - 1, z)) / two;
    const T u_z_dz = (U(2, x, y, z + 1) - U(2, x, y, z - 1)) / two;
    const T s01 = half * (u_x_dy + u_y_dx), s02 = half * (u_x_dz + u_z_dx), s12 = half * (u_y_dz + u_z_dy);
    // s_dot_s: the nine squares summed in row-major order, as the reference writes them
    T ss = u_x_dx * u_x_dx;
    ss = ss + s01 * s01;
    ss = ss + s02 * s02;
    ss = ss + s01 * s01;
    ss = ss + u_y_dy * u_y_dy;
    ss = ss + s12 * s12;
    ss = ss + s02 * s02;
    ss = ss + s12 * s12;
    ss = ss + u_z_dz * u_z_dz;
    const T o01 = half * (u_x_dy - u_y_dx), o02 = half * (u_x_dz - u_z_dx), o12 = half * (u_y_dz - u_z_dy);
    const T o10 = -o01, o20 = -o02, o21 = -o12;
    // omega_dot_omega: same order; the three 0.0**2 terms add exact zeros to non-negative partial sums
    T oo = T(0.0) + o01 * o01;
    oo = oo + o02 * o02;
    oo = oo + o10 * o10;
    oo = oo + T(0.0);
    oo = oo + o12 * o12;
    oo = oo + o20 * o20;
    oo = oo + o21 * o21;
    oo = oo + T(0.0);
    store_rt<T>(out_a, oa, mag);
    store_rt<T>(out_b, ob, half * (oo - ss));
  }
}

// any Zou-He / Regularized / outflow / do-nothing cell strictly inside the x range?  (two-step kernel with inlet / outlet planes)
static __global__ void k_ext_interior_scan(FieldView bc, const uint8_t* kind_tab, Dims d, int* flag) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  if (x < 1 || x > d.nx - 2) return;
  const unsigned id = static_cast<const uint8_t*>(bc.data)[cell_index(bc, d, x, y, z)];
  if (id != 0u && bc_is_edge_kind(kind_tab[id])) *flag = 1;
}

// periodic pull of the q populations arriving at a cell (stream.py:57-62), and the cell's own ones
template <class L, class T>
__device__ __forceinline__ void pull_cell(const FieldView& f0, const Dims& d, int x, int y, int z, T (&f)[L::Q]) {
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    const int xs = f0.halo ? x - L::c(0, l) : wrap(x - L::c(0, l), d.nx);
    f[l] = load_rt<T>(f0, (size_t)l * f0.plane_stride + cell_index(f0, d, xs, wrap(y - L::c(1, l), d.ny), wrap(z - L::c(2, l), d.nz)));
  });
}
template <class L, class T>
__device__ __forceinline__ void own_cell(const FieldView& f0, const Dims& d, int x, int y, int z, T (&f)[L::Q]) {
  const size_t c = cell_index(f0, d, x, y, z);
  static_for<L::Q>([&](auto lc) { f[decltype(lc)::value] = load_rt<T>(f0, (size_t) decltype(lc)::value * f0.plane_stride + c); });
}

// ---- MomentumTransfer (force/momentum_transfer.py:167-205, JAX): force on the solid behind a no-slip BC ----------
// f0 holds post-collision populations.  At every cell of the BC that is not itself solid (rest direction not
// missing), for every missing direction l:  phi_l = f0[opp l] + f_post_stream[l],  f_post_stream[l] = the BC's
// bounce-back of the own cell (halfway: f0[opp l] + wall term; fullway: f0[opp l]);  F = sum c_{opp l} phi_l.
// One double-precision atomic per block and component (the grid sum's order is unpinned in the reference as well).
template <class L, class T>
__global__ void __launch_bounds__(BC_BLOCK) k_momentum_transfer(FieldView f0, FieldView bc, FieldView miss, Dims d, int id, BcValues<T> vals, int add_wall_term,
                                    double* force /*[3]*/) {
  int x, y, z;
  T fx = T(0), fy = T(0), fz = T(0);
  if (cell_of_thread(d, x, y, z)) {
    const uint8_t b = static_cast<const uint8_t*>(bc.data)[cell_index(bc, d, x, y, z)];
    if (b == id) {
      const unsigned m = static_cast<const uint32_t*>(miss.data)[cell_index(miss, d, x, y, z)];
      if ((m & 1u) == 0u) {  // is_edge: boundary & ~missing_mask[0]
        const size_t own = cell_index(f0, d, x, y, z);
        static_for<L::Q>([&](auto lc) {
          constexpr int l = decltype(lc)::value;
          constexpr int o = opp<L>(l);
          if ((m >> l) & 1u) {
            const T fo = load_rt<T>(f0, (size_t)o * f0.plane_stride + own);
            T ps = fo;
            if (add_wall_term) ps = fo + vals.v[l];
            add_link_force<L, o>(fo + ps, fx, fy, fz);
          }
        });
      }
    }
  }
  block_sum3_add(fx, fy, fz, force);
}

// MomentumTransfer for the BCs whose post-stream populations need the stepper's tables (HybridBC: wall distances, wall-velocity
// profile; halfway bounce-back with a profile) — the kernel backends' path of the reference, force/momentum_transfer.py:225-262 with
// FetchPopulations (:75-92): f_post_stream = the BC applied to (own populations of f_0, populations pulled from f_0).
template <class L, class T>
__global__ void __launch_bounds__(BC_BLOCK) k_momentum_transfer_tab(FieldView f0, FieldView bc, FieldView miss, Dims d, int id, BcView<T> tb, double* force /*[3]*/) {
  constexpr int Q = L::Q;
  int x, y, z;
  T fx = T(0), fy = T(0), fz = T(0);
  if (cell_of_thread(d, x, y, z)) {
    const uint8_t b = static_cast<const uint8_t*>(bc.data)[cell_index(bc, d, x, y, z)];
    if (b == id) {
      const unsigned m = static_cast<const uint32_t*>(miss.data)[cell_index(miss, d, x, y, z)];
      if ((m & 1u) == 0u) {
        T pre[Q], ps[Q];
        own_cell<L, T>(f0, d, x, y, z, pre);
        pull_cell<L, T>(f0, d, x, y, z, ps);
        apply_streaming_bc<L, T>(tb, (unsigned)id, (unsigned)cell_index(bc, d, x, y, z), ps, pre, m);
        static_for<Q>([&](auto lc) {
          constexpr int l = decltype(lc)::value;
          constexpr int o = opp<L>(l);
          if ((m >> l) & 1u) add_link_force<L, o>(pre[o] + ps[l], fx, fy, fz);
        });
      }
    }
  }
  block_sum3_add(fx, fy, fz, force);
}

// ---- GridToPoint (postprocess/grid_to_point.py:28-94): trilinear interpolation of component 0 at arbitrary points ----
// weights in fp32 from the fp32 point coordinates, as the reference computes them; products and the 8-term sum in its order
template <class T>
__global__ void k_grid_to_point(FieldView g, Dims d, const float* pts /*[n][3]*/, T* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
  const int x = (int)px, y = (int)py, z = (int)pz;
  const float dx = px - (float)x, dy = py - (float)y, dz = pz - (float)z;
  const float one = 1.0f;
  auto G = [&](int a, int b, int c) { return load_rt<T>(g, cell_index(g, d, x + a, y + b, z + c)); };
  T v = T((one - dx) * (one - dy) * (one - dz)) * G(0, 0, 0);
  v = v + T((one - dx) * (one - dy) * dz) * G(0, 0, 1);
  v = v + T((one - dx) * dy * (one - dz)) * G(0, 1, 0);
  v = v + T((one - dx) * dy * dz) * G(0, 1, 1);
  v = v + T(dx * (one - dy) * (one - dz)) * G(1, 0, 0);
  v = v + T(dx * (one - dy) * dz) * G(1, 0, 1);
  v = v + T(dx * dy * (one - dz)) * G(1, 1, 0);
  v = v + T(dx * dy * dz) * G(1, 1, 1);
  out[i] = v;
}

// ---- ExtrapolationOutflowBC: auxiliary data after the collision --------------------------
// assemble_auxiliary_data of ExtrapolationOutflowBC (bc_extrapolation_outflow.py:104-134), run after the step kernel: at an outflow cell b
// with outward normal n, for every l whose opposite is missing, f_1[l](b) = cs * f_post_stream[opp l](b - n) + (1 - cs) * f_post_stream[opp l](b).
// f_post_stream of a cell: periodic pull + that cell's STREAMING-step BC (nse_stepper.py:246-257): the outflow rule for b, any kind behind it.
template <class L, class T>
__global__ void __launch_bounds__(BC_BLOCK) k_outflow_aux(FieldView f0, FieldView f1, FieldView bc, FieldView miss, Dims d, BcView<T> tb) {
  // nearly every thread leaves here: its bc_mask byte sits at the thread's linear index (cell_index is linear in it), no division needed
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)d.nx * d.ny * d.nz) return;
  const unsigned id = static_cast<const uint8_t*>(bc.data)[t + (size_t)bc.halo * d.ny * d.nz];
  if (id == 0u || tb.kind[id] != XLBHIP_BC_EXTRAPOLATION_OUTFLOW) return;
  int x, y, z;
  cell_of_thread(d, x, y, z);
  const T* val = tb.values + id * 27u;
  const int n0 = (int)val[0], n1 = (int)val[1], n2 = (int)val[2];
  const T cs = val[3], omcs = val[4];
  int xn = x - n0;
  if (f0.halo) {
    if (xn < 0 || xn >= d.nx) return;  // the cell behind the face lives on another rank: outflow faces must be domain faces
  } else {
    xn = wrap(xn, d.nx);
  }
  const int yn = wrap(y - n1, d.ny), zn = wrap(z - n2, d.nz);
  const uint32_t* mp = static_cast<const uint32_t*>(miss.data);
  const unsigned m = mp[cell_index(miss, d, x, y, z)];
  const T none[5] = {T(0), T(0), T(0), T(0), T(0)};
  T fb[L::Q], fn[L::Q], pre[L::Q];
  pull_cell<L, T>(f0, d, x, y, z, fb);
  own_cell<L, T>(f0, d, x, y, z, pre);
  apply_streaming_bc<L, T>(XLBHIP_BC_EXTRAPOLATION_OUTFLOW, fb, pre, m, val, none, nullptr);
  pull_cell<L, T>(f0, d, xn, yn, zn, fn);
  const unsigned idn = static_cast<const uint8_t*>(bc.data)[cell_index(bc, d, xn, yn, zn)];
  if (idn != 0u) {
    own_cell<L, T>(f0, d, xn, yn, zn, pre);
    apply_streaming_bc<L, T>(tb, idn, (unsigned)cell_index(bc, d, xn, yn, zn), fn, pre, mp[cell_index(miss, d, xn, yn, zn)]);
  }
  const size_t o1 = cell_index(f1, d, x, y, z);
  static_for<L::Q>([&](auto lc) {
    constexpr int l = decltype(lc)::value;
    constexpr int o = opp<L>(l);
    if ((m >> o) & 1u) store_rt<T>(f1, (size_t)l * f1.plane_stride + o1, cs * fn[o] + omcs * fb[o]);
  });
}

// pack / unpack the host (q, nx, ny, nz) u8 view of missing_mask <-> device bit-sets
static __global__ void k_pack_missing(const uint8_t* bytes, uint32_t* bits, int q, Dims d, int halo) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  const size_t n = (size_t)d.nx * d.ny * d.nz;
  const size_t c = ((size_t)x * d.ny + y) * d.nz + z;
  unsigned b = 0;
  for (int l = 0; l < q; ++l) b |= (bytes[(size_t)l * n + c] ? 1u : 0u) << l;
  bits[((size_t)(x + halo) * d.ny + y) * d.nz + z] = b;
}
static __global__ void k_unpack_missing(const uint32_t* bits, uint8_t* bytes, int q, Dims d, int halo) {
  int x, y, z;
  if (!cell_of_thread(d, x, y, z)) return;
  const size_t n = (size_t)d.nx * d.ny * d.nz;
  const size_t c = ((size_t)x * d.ny + y) * d.nz + z;
  const unsigned b = bits[((size_t)(x + halo) * d.ny + y) * d.nz + z];
  for (int l = 0; l < q; ++l) bytes[(size_t)l * n + c] = (b >> l) & 1u;
}

// plain streaming copy, W bytes per lane: the bandwidth yardstick and the byte-count
// calibration kernel for the FETCH_SIZE / WRITE_SIZE counters (known traffic: n bytes each way)
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
template <class V>
__global__ void k_copy(const V* __restrict__ src, V* __restrict__ dst, size_t n) {
  // grid-stride: HIP refuses launches of 2^32 threads or more, an 81.6 GB field (4096 x 512 x 512, D3Q19) has 5.1e9 16-byte words
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    __builtin_nontemporal_store(src[i], dst + i);
}

// rows of a field at listed interior cells: out[i][l] = field[l][cells[i]] (small device -> host transfers of boundary data)
template <class E>
__global__ void k_gather(const E* data, size_t plane_stride, size_t ghost, int card, const uint32_t* cells, int64_t n, E* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int l = 0; l < card; ++l) out[i * card + l] = data[(size_t)l * plane_stride + ghost + cells[i]];
}

// meta word of the two-step kernel, resolved once per run so that the kernel never searches an id table (layouts: step2_kernel.hpp
// S2Meta): kind (0 fluid, XLBHIP_BC_* for the basic kinds, or "halfway wall WITH a moving-wall term"), slot of the BC in the
// stepper's packed tables, missing bit-set.  wide = 0: 4 + 4 + up to 24 bits (D3Q19); wide = 1: 3 + 3 + bits 1 .. 26 (D3Q27).
static __global__ void k_build_meta(const uint8_t* bc, const uint32_t* miss, uint32_t* meta, size_t n, unsigned long long ids_packed,
                             unsigned kinds_packed, unsigned moving_mask, int wide) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned id = bc[i];
  unsigned w = 0;
  if (id != 0u) {
    unsigned kind = 0, slot = 0;
    for (int s = 0; s < 8; ++s)
      if (((unsigned)(ids_packed >> (8 * s)) & 0xffu) == id) {
        kind = (kinds_packed >> (4 * s)) & 0xfu;
        slot = (unsigned)s;
      }
    const unsigned m = miss ? miss[i] : 0u;
    if (wide) {
      if (kind == XLBHIP_BC_HALFWAY_BB && ((moving_mask >> slot) & 1u)) kind = 5u;  // S2Meta<D3Q27>::K_HWM
      w = (kind & 7u) | (slot << 3) | ((m >> 1) << 6);
    } else {
      if (kind == XLBHIP_BC_HALFWAY_BB && ((moving_mask >> slot) & 1u)) kind = 15u;  // S2Meta<D3Q19>::K_HWM
      w = kind | (slot << 4) | (m << 8);
    }
  }
  meta[i] = w;
}

template <class E>
__global__ void k_fill(E* p, size_t n, E v) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;  // grid-stride (see k_copy)
}

}  // namespace xlb
