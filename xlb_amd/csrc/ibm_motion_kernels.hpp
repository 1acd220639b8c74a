// Rigid bodies of the immersed-boundary stepper: the kernel that moves the markers of a body and the ones that sum the coupling
// forces to a force and a torque per body (reference: examples/ibm/wind_turbine_ibm.py:160-199, the `rotate_rotor` kernel that turns
// the rotor's vertices and sets their velocities on the device after every step; the per-body loads have no counterpart there).
//
//   k_ibm_move           (per step, bodies that move)  X = c + R (X0 - c0), U = v + w x (X - c) for the markers of moving bodies
//   k_ibm_loads          (per step)                    six partial sums per chunk of 256 consecutive markers of one body
//   k_ibm_loads_combine  (per step)                    the chunks of a body added in index order -> loads[body][6] (and a history row)
//
// A POSE is 18 doubles per (step, body): R (3 x 3, row-major) | c | w | v, evaluated by the host and staged ahead of the steps
// (csrc/ibm.hip).  The arithmetic of k_ibm_move is fp64 in ONE stated order, so that a host restatement with elementwise operations
// gives the same bits (the build has -ffp-contract=off); the result is rounded to the float32 the coupling kernels read.
//
// Loads.  No floating-point atomics: the partition (chunks of 256 consecutive markers of a body, laid out by the host when the
// bodies are declared), the tree inside a chunk and the order of the chunks are fixed, so two runs give the same bits.  The tree
// adds neighbours upwards — at level s the threads whose low bits are all ones take part[t] = part[t - s] + part[t] — and leaves the
// sum with the last thread.  A thread only ever reads an element whose owner has finished all its levels, which is also what makes
// the kernel runnable one emulated thread after the other (tests/ibm_motion_cpu_emulation.cpp).  The tree goes through LDS rather
// than cross-lane moves: a launch is (markers / 256) blocks of a few hundred bytes each, bound by its latency, not by LDS traffic.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "ibm_bodies.hpp"

namespace xlb {

// move_id[k]: the body of marker k when that body moves, else -1 (a body at rest, no body: the marker is not touched)
__global__ void k_ibm_move(const float* __restrict__ pos0, const int32_t* __restrict__ move_id, const double* __restrict__ pose,
                           const double* __restrict__ centre0, int64_t n, float* __restrict__ pos, float* __restrict__ vel) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int b = move_id[k];
  if (b < 0) return;
  const double* P = pose + (size_t)b * IBM_POSE_DOUBLES;
  const double* R = P;
  const double c[3] = {P[9], P[10], P[11]}, w[3] = {P[12], P[13], P[14]}, v[3] = {P[15], P[16], P[17]};
  double d[3], r[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) d[a] = (double)pos0[3 * k + a] - centre0[3 * b + a];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double X = ((R[3 * a] * d[0] + R[3 * a + 1] * d[1]) + R[3 * a + 2] * d[2]) + c[a];
    const float Xf = (float)X;
    pos[3 * k + a] = Xf;
    r[a] = (double)Xf - c[a];  // the velocity belongs to the position the coupling sees
  }
  vel[3 * k] = (float)(v[0] + (w[1] * r[2] - w[2] * r[1]));
  vel[3 * k + 1] = (float)(v[1] + (w[2] * r[0] - w[0] * r[2]));
  vel[3 * k + 2] = (float)(v[2] + (w[0] * r[1] - w[1] * r[0]));
}

// partial[chunk][0..2] = sum A F, [3..5] = sum A ((X - c) x F) over the chunk's markers; every factor is a double before any product
template <class T>
__global__ __launch_bounds__(IBM_LOADS_CHUNK) void k_ibm_loads(const IbmLoadChunk* __restrict__ chunks, const T* __restrict__ F,
                                                               const float* __restrict__ area, const float* __restrict__ pos,
                                                               const double* __restrict__ pose, double* __restrict__ partial) {
  __shared__ double part[6][IBM_LOADS_CHUNK];
  const int t = (int)threadIdx.x;
  const IbmLoadChunk ch = chunks[blockIdx.x];
  double term[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (t < ch.count) {
    const size_t k = (size_t)ch.first + t;
    const double* c = pose + (size_t)ch.body * IBM_POSE_DOUBLES + 9;
    const double A = (double)area[k];
    const double f[3] = {(double)F[3 * k], (double)F[3 * k + 1], (double)F[3 * k + 2]};
    const double r[3] = {(double)pos[3 * k] - c[0], (double)pos[3 * k + 1] - c[1], (double)pos[3 * k + 2] - c[2]};
    term[0] = A * f[0];
    term[1] = A * f[1];
    term[2] = A * f[2];
    term[3] = A * (r[1] * f[2] - r[2] * f[1]);
    term[4] = A * (r[2] * f[0] - r[0] * f[2]);
    term[5] = A * (r[0] * f[1] - r[1] * f[0]);
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) part[a][t] = term[a];
  for (int s = 1; s < IBM_LOADS_CHUNK; s <<= 1) {
    __syncthreads();
    if ((t & (2 * s - 1)) == 2 * s - 1) {
#pragma unroll
      for (int a = 0; a < 6; ++a) part[a][t] = part[a][t - s] + part[a][t];
    }
  }
  if (t == IBM_LOADS_CHUNK - 1) {
#pragma unroll
    for (int a = 0; a < 6; ++a) partial[(size_t)blockIdx.x * 6 + a] = part[a][t];
  }
}

// loads[body][a] = -(partial[chunk0[body]][a] + partial[chunk0[body] + 1][a] + ...): the force and the torque ON the body are the
// reaction to what the markers exert on the fluid.  history_row (may be null): the same values, row `step` of the recorded history.
__global__ void k_ibm_loads_combine(const int32_t* __restrict__ chunk0, const double* __restrict__ partial, int n_bodies, double* __restrict__ loads,
                                    double* __restrict__ history_row) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n_bodies * 6) return;
  const int b = i / 6, a = i - 6 * b;
  double s = 0.0;
  for (int j = chunk0[b]; j < chunk0[b + 1]; ++j) s = s + partial[(size_t)j * 6 + a];
  loads[i] = -s;
  if (history_row) history_row[i] = -s;
}

}  // namespace xlb
