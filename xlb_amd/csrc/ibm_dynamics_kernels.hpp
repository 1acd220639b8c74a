// Free (force-driven) rigid bodies of the immersed-boundary stepper: the pose table every step's move and loads read, and the
// integrator that advances a body from the loads of the step (no counterpart in the reference: its examples/ibm/wind_turbine_ibm.py
// prescribes the rotor's rate; the effective mass and inertia follow Uhlmann, J. Comput. Phys. 209 (2005) 448).
//
//   k_ibm_pose       (per step, before the move)   live[body][18] = R | c | w | v of the step: from the state of a dynamic body, the
//                                                  staged row of a prescribed one, the rest pose of a body at rest (+ a history row)
//   k_ibm_integrate  (per step, after the loads)   state(t) -> state(t + 1) of the dynamic bodies from loads[body][6]
//
// Both are ONE block with one thread per body (at most IBM_MAX_BODIES = 64): two launches bound by their latency.
//
// State of a body, IBM_DYN_STATE_DOUBLES = 16 doubles:   c[3] | v[3] | q[4] (w, x, y, z; unit) | L[3] | 3 unused
//   L is the world-frame angular momentum of a free rotation; in axis mode L[0] is the scalar rate about the axis.
// Parameters, IBM_DYN_PARAM_DOUBLES = 32 doubles:
//   0 1/mass | 1-3 translate (0. or 1.) | 4-6 force | 7-9 torque | 10-12 anchor | 13-15 stiffness | 16-18 damping |
//   19-27 inverse body-frame inertia, row-major | 28-30 axis (unit) | 31 1 / (inertia about the axis)
//
// The update, dt = 1, with (Fh, Th) the loads of the step about c(t):
//   F  = ((Fh + force) + (-(stiffness (c - anchor)))) + (-(damping v));  v' = v + translate (F (1/mass));  c' = c + v'
//   free:   L' = L + (Th + torque);  w* = R (Iinv (R^T L'));  q' = normalise(cay(w*) (x) q)
//   axis:   L0' = L0 + (a . (Th + torque)) (1/Ia);            q' = normalise(cay(L0' a) (x) q)
//   locked: q' = q
//   cay(th) = (1, th/2) / sqrt(1 + |th/2|^2): the Cayley map — rational and exactly orthogonal, no sin / cos whose bits differ
//   between libraries.  Divisions and square roots are the correctly rounded fp64 ones, never reciprocal approximations.
// Every line is fp64 in ONE stated order — 3-term sums from the left, (a b + c d) + e f — so that the elementwise NumPy restatement
// tests/_ibm_dynamics_ref.py gives the same bits (the build has -ffp-contract=off).  A new state with a component that is not finite
// is NOT stored: the body keeps its state and its bit is set in the sticky status word.
//
// Virtual mass and contact (k_ibm_integrate_contact, launched in place of k_ibm_integrate when either is switched on; a run with
// neither launches k_ibm_integrate itself, the kernel of a stepper that has neither).  The virtual-mass scheme is Schwarz, Kempe &
// Froehlich, J. Comput. Phys. 281 (2015) 591: the virtual term is added to both sides, the right-hand side with the PREVIOUS step's
// acceleration.  virt[b][2] = (m_v, I_v), both >= 0; prev[b][6] = a_prev | alpha_prev, zero at the start.  The host passes
// 1 / (mass + m_v) in slot 0, the inverse of (Ib + I_v E) in 19-27 and 1 / (I_a + I_v) in 31; L is the momentum of that inertia.
//   F as above, + Fc when the body has a contact radius:  F = (((Fh + force) + spring) + damping) + Fc
//   m_v > 0:  a = (F + m_v a_prev) (1/(mass + m_v))     else  a = F (1/mass)            [per axis]
//   ta = translate a;  v' = v + ta;  c' = c + v';  a_prev' = ta
//   I_v > 0:  T' = (Th + torque) + I_v alpha_prev       else  T' = Th + torque          [per component, also in axis mode]
//   L', w*, q' as above with T' for (Th + torque);  alpha_prev' = w* - w(R, L), w the angular velocity of the state the step
//   started from with the same R (componentwise; zero for a locked body)
// A body whose m_v (I_v) is zero is advanced by exactly the operations of k_ibm_integrate.  The 13 state doubles and the 6 of prev
// are stored together or not at all.
// Contact: a central repulsive soft-sphere force of the Glowinski / Wan-Turek kind on every DYNAMIC body i with radius[i] > 0, from
// the centres c of the pose table k_ibm_pose wrote for the step (live[b][9..11]: every body's c(t), no thread reads a state another
// writes).  M = range zeta, stiffness k, wall stiffness kw, planes lo[3], hi[3] (-inf / +inf: no plane).  Fc starts at zero, then
//   walls, axis 0, 1, 2, lo before hi:   gap = (c_a - lo_a) - r_i;  gap < zeta:  Fc_a = Fc_a + kw ((zeta - gap) (zeta - gap))
//                                        gap = (hi_a - c_a) - r_i;  gap < zeta:  Fc_a = Fc_a + (-(kw ((zeta - gap) (zeta - gap))))
//   bodies j = 0, 1, ... (j != i, radius[j] > 0, of any kind):   e = c_i - c_j;  d = sqrt((e_0 e_0 + e_1 e_1) + e_2 e_2);
//                                        gap = d - (r_i + r_j);  gap < zeta and d > 0:  s = k ((zeta - gap) (zeta - gap));
//                                        Fc_a = Fc_a + (s e_a) / d
// so the pair terms of i and j are exact negatives of each other.  contact[b][3] keeps Fc of the last step (zero for a body that is
// not dynamic or has no radius), also when the new state was refused.  No torque: the force is central.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "ibm_bodies.hpp"
#include "ibm_motion_kernels.hpp"

namespace xlb {

__device__ __forceinline__ bool ibm_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }  // (false for a NaN)

// y = M x and y = M^T x, M row-major
__device__ __forceinline__ void ibm_mat_vec(const double* M, const double* x, double* y) {
#pragma unroll
  for (int a = 0; a < 3; ++a) y[a] = (M[3 * a] * x[0] + M[3 * a + 1] * x[1]) + M[3 * a + 2] * x[2];
}
__device__ __forceinline__ void ibm_mat_t_vec(const double* M, const double* x, double* y) {
#pragma unroll
  for (int a = 0; a < 3; ++a) y[a] = (M[a] * x[0] + M[3 + a] * x[1]) + M[6 + a] * x[2];
}

// the rotation of the unit quaternion q = (w, x, y, z), row-major
__device__ __forceinline__ void ibm_quat_matrix(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  R[0] = 1.0 - 2.0 * (yy + zz);
  R[1] = 2.0 * (xy - wz);
  R[2] = 2.0 * (xz + wy);
  R[3] = 2.0 * (xy + wz);
  R[4] = 1.0 - 2.0 * (xx + zz);
  R[5] = 2.0 * (yz - wx);
  R[6] = 2.0 * (xz - wy);
  R[7] = 2.0 * (yz + wx);
  R[8] = 1.0 - 2.0 * (xx + yy);
}

// the world-frame angular velocity that belongs to (R, L): R Iinv R^T L, L[0] a, or zero
__device__ __forceinline__ void ibm_angular_velocity(int rotate, const double* R, const double* L, const double* P, double* w) {
  if (rotate == IBM_ROTATE_FREE) {
    double u[3], s[3];
    ibm_mat_t_vec(R, L, u);
    ibm_mat_vec(P + 19, u, s);
    ibm_mat_vec(R, s, w);
  } else if (rotate == IBM_ROTATE_AXIS) {
#pragma unroll
    for (int a = 0; a < 3; ++a) w[a] = L[0] * P[28 + a];
  } else {
    w[0] = w[1] = w[2] = 0.0;
  }
}

// q' = normalise(cay(th) (x) q)
__device__ __forceinline__ void ibm_cayley_step(const double* th, const double* q, double* out) {
  const double h[3] = {0.5 * th[0], 0.5 * th[1], 0.5 * th[2]};
  const double den = sqrt(1.0 + ((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]));
  const double p[4] = {1.0 / den, h[0] / den, h[1] / den, h[2] / den};
  const double r[4] = {((p[0] * q[0] - p[1] * q[1]) - p[2] * q[2]) - p[3] * q[3], ((p[0] * q[1] + p[1] * q[0]) + p[2] * q[3]) - p[3] * q[2],
                       ((p[0] * q[2] - p[1] * q[3]) + p[2] * q[0]) + p[3] * q[1], ((p[0] * q[3] + p[1] * q[2]) - p[2] * q[1]) + p[3] * q[0]};
  const double norm = sqrt(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]);
#pragma unroll
  for (int a = 0; a < 4; ++a) out[a] = r[a] / norm;
}

// kind[b]: IBM_BODY_*.  staged: the poses [n_bodies][18] staged for this timestep, or null (then a prescribed body reads its rest
// pose).  history_row (may be null): the same rows, one step of the recorded pose history.
__global__ __launch_bounds__(IBM_MAX_BODIES) void k_ibm_pose(const int32_t* __restrict__ kind, const int32_t* __restrict__ rotate,
                                                             const double* __restrict__ state, const double* __restrict__ params,
                                                             const double* __restrict__ staged, const double* __restrict__ rest, int n_bodies,
                                                             double* __restrict__ live, double* __restrict__ history_row) {
  const int b = (int)threadIdx.x;
  if (b >= n_bodies) return;
  double row[IBM_POSE_DOUBLES];
  if (kind[b] == IBM_BODY_DYNAMIC) {
    const double* S = state + (size_t)b * IBM_DYN_STATE_DOUBLES;
    const double q[4] = {S[6], S[7], S[8], S[9]}, L[3] = {S[10], S[11], S[12]};
    ibm_quat_matrix(q, row);
    ibm_angular_velocity(rotate[b], row, L, params + (size_t)b * IBM_DYN_PARAM_DOUBLES, row + 12);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      row[9 + a] = S[a];
      row[15 + a] = S[3 + a];
    }
  } else {
    const double* src = (kind[b] == IBM_BODY_PRESCRIBED && staged ? staged : rest) + (size_t)b * IBM_POSE_DOUBLES;
#pragma unroll
    for (int a = 0; a < IBM_POSE_DOUBLES; ++a) row[a] = src[a];
  }
#pragma unroll
  for (int a = 0; a < IBM_POSE_DOUBLES; ++a) {
    live[(size_t)b * IBM_POSE_DOUBLES + a] = row[a];
    if (history_row) history_row[(size_t)b * IBM_POSE_DOUBLES + a] = row[a];
  }
}

// the contact force on body i (header comment: walls by axis, lo before hi, then the bodies in ascending order)
__device__ __forceinline__ void ibm_contact_force(int i, const double* __restrict__ radius, const IbmContactModel& M, const double* __restrict__ live,
                                                  int n_bodies, double* Fc) {
  const double ri = radius[i];
  const double* ci = live + (size_t)i * IBM_POSE_DOUBLES + 9;
  Fc[0] = Fc[1] = Fc[2] = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double glo = (ci[a] - M.lo[a]) - ri;
    if (glo < M.range) {
      const double p = M.range - glo;
      Fc[a] = Fc[a] + M.wall_stiffness * (p * p);
    }
    const double ghi = (M.hi[a] - ci[a]) - ri;
    if (ghi < M.range) {
      const double p = M.range - ghi;
      Fc[a] = Fc[a] + (-(M.wall_stiffness * (p * p)));
    }
  }
  for (int j = 0; j < n_bodies; ++j) {
    if (j == i || !(radius[j] > 0.0)) continue;
    const double* cj = live + (size_t)j * IBM_POSE_DOUBLES + 9;
    const double e[3] = {ci[0] - cj[0], ci[1] - cj[1], ci[2] - cj[2]};
    const double d = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    const double gap = d - (ri + radius[j]);
    if (gap < M.range && d > 0.0) {
      const double p = M.range - gap;
      const double s = M.stiffness * (p * p);
#pragma unroll
      for (int a = 0; a < 3; ++a) Fc[a] = Fc[a] + (s * e[a]) / d;
    }
  }
}

// one dynamic body from state(t) to state(t + 1).  Extended = false is k_ibm_integrate as it has always been; Extended = true adds the
// virtual mass and the contact force of the header comment (virt, prev, contact are never null then; radius null: no contact)
template <bool Extended>
__device__ __forceinline__ void ibm_integrate_body(int b, int mode, const double* __restrict__ P, const double* __restrict__ H, double* __restrict__ S,
                                                   unsigned long long* __restrict__ status, const double* __restrict__ virt, double* __restrict__ prev,
                                                   const double* __restrict__ radius, const IbmContactModel& M, const double* __restrict__ live,
                                                   int n_bodies, double* __restrict__ contact) {
  double next[13 + 6];
  double Fc[3] = {0.0, 0.0, 0.0};
  bool touching = false;
  double mv = 0.0, iv = 0.0;
  double* A = nullptr;
  if constexpr (Extended) {
    mv = virt[2 * b];
    iv = virt[2 * b + 1];
    A = prev + (size_t)b * 6;
    touching = radius && radius[b] > 0.0;
    if (touching) ibm_contact_force(b, radius, M, live, n_bodies, Fc);
#pragma unroll
    for (int a = 0; a < 3; ++a) contact[(size_t)b * 3 + a] = Fc[a];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double c = S[a], v = S[3 + a];
    double F = ((H[a] + P[4 + a]) + (-(P[13 + a] * (c - P[10 + a])))) + (-(P[16 + a] * v));
    if constexpr (Extended) {
      if (touching) F = F + Fc[a];
    }
    double acc = F * P[0];
    if constexpr (Extended) {
      if (mv > 0.0) acc = (F + mv * A[a]) * P[0];
    }
    const double ta = P[1 + a] * acc;
    const double vn = v + ta;
    next[3 + a] = vn;
    next[a] = c + vn;
    next[13 + a] = ta;
  }
  const double q[4] = {S[6], S[7], S[8], S[9]};
  double T[3] = {H[3] + P[7], H[4] + P[8], H[5] + P[9]};
  if constexpr (Extended) {
    if (iv > 0.0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) T[a] = T[a] + iv * A[3 + a];
    }
  }
  if (mode == IBM_ROTATE_LOCKED) {
#pragma unroll
    for (int a = 0; a < 7; ++a) next[6 + a] = S[6 + a];
    next[16] = next[17] = next[18] = 0.0;
  } else {
    double R[9], th[3];
    if (mode == IBM_ROTATE_FREE) {
#pragma unroll
      for (int a = 0; a < 3; ++a) next[10 + a] = S[10 + a] + T[a];
    } else {
      next[10] = S[10] + ((P[28] * T[0] + P[29] * T[1]) + P[30] * T[2]) * P[31];
      next[11] = S[11];
      next[12] = S[12];
    }
    ibm_quat_matrix(q, R);
    ibm_angular_velocity(mode, R, next + 10, P, th);
    ibm_cayley_step(th, q, next + 6);
    if constexpr (Extended) {
      double w0[3];
      ibm_angular_velocity(mode, R, S + 10, P, w0);
#pragma unroll
      for (int a = 0; a < 3; ++a) next[16 + a] = th[a] - w0[a];
    }
  }
  constexpr int checked = Extended ? 19 : 13;
  bool ok = true;
#pragma unroll
  for (int a = 0; a < checked; ++a) ok = ok && ibm_finite(next[a]);
  if (ok) {
#pragma unroll
    for (int a = 0; a < 13; ++a) S[a] = next[a];
    if constexpr (Extended) {
#pragma unroll
      for (int a = 0; a < 6; ++a) A[a] = next[13 + a];
    }
  } else {
    atomicOr(status, 1ull << b);
  }
}

// loads[b][6]: what k_ibm_loads_combine left for the step, about the c of the state
__global__ __launch_bounds__(IBM_MAX_BODIES) void k_ibm_integrate(const int32_t* __restrict__ kind, const int32_t* __restrict__ rotate,
                                                                  const double* __restrict__ params, const double* __restrict__ loads, int n_bodies,
                                                                  double* __restrict__ state, unsigned long long* __restrict__ status) {
  const int b = (int)threadIdx.x;
  if (b >= n_bodies || kind[b] != IBM_BODY_DYNAMIC) return;
  ibm_integrate_body<false>(b, rotate[b], params + (size_t)b * IBM_DYN_PARAM_DOUBLES, loads + (size_t)b * 6, state + (size_t)b * IBM_DYN_STATE_DOUBLES, status,
                            nullptr, nullptr, nullptr, IbmContactModel{}, nullptr, n_bodies, nullptr);
}

// the same with virtual mass and contact: virt [n_bodies][2], prev [n_bodies][6], radius [n_bodies] or null (no contact), live the pose
// table of the step, contact [n_bodies][3]
__global__ __launch_bounds__(IBM_MAX_BODIES) void k_ibm_integrate_contact(const int32_t* __restrict__ kind, const int32_t* __restrict__ rotate,
                                                                          const double* __restrict__ params, const double* __restrict__ loads, int n_bodies,
                                                                          double* __restrict__ state, unsigned long long* __restrict__ status,
                                                                          const double* __restrict__ virt, double* __restrict__ prev,
                                                                          const double* __restrict__ radius, IbmContactModel model,
                                                                          const double* __restrict__ live, double* __restrict__ contact) {
  const int b = (int)threadIdx.x;
  if (b >= n_bodies) return;
  if (kind[b] != IBM_BODY_DYNAMIC) {
    contact[(size_t)b * 3] = contact[(size_t)b * 3 + 1] = contact[(size_t)b * 3 + 2] = 0.0;
    return;
  }
  ibm_integrate_body<true>(b, rotate[b], params + (size_t)b * IBM_DYN_PARAM_DOUBLES, loads + (size_t)b * 6, state + (size_t)b * IBM_DYN_STATE_DOUBLES, status,
                           virt, prev, radius, model, live, n_bodies, contact);
}

}  // namespace xlb
