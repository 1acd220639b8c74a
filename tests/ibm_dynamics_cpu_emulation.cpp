// The free-body kernels of the immersed-boundary stepper (xlb_amd/csrc/ibm_dynamics_kernels.hpp) compiled for the host through
// tests/hip_on_cpu: the launches of csrc/ibm.hip — one block of IBM_MAX_BODIES threads — every thread run one after the other.
// tests/test_ibm_dynamics_on_cpu.py compares with tests/_ibm_dynamics_ref.py.
#include "ibm_dynamics_kernels.hpp"
thread_local emulated_dim3 threadIdx, blockIdx, blockDim, gridDim;
using namespace xlb;
template <class K, class... A>
static void launch(K k, size_t blocks, unsigned threads, A... a) {
  blockDim.x = threads;
  gridDim.x = (unsigned)blocks;
  for (size_t b = 0; b < blocks; ++b)
    for (unsigned t = 0; t < threads; ++t) { blockIdx.x = (unsigned)b; threadIdx.x = t; k(a...); }
}
// live [nb][18] (and history_row, may be null) of one step; staged may be null
extern "C" int pose_cpu(int nb, const int32_t* kind, const int32_t* rotate, const double* state, const double* params, const double* staged,
                        const double* rest, double* live, double* history_row) {
  if (nb > IBM_MAX_BODIES) return 1;
  launch(k_ibm_pose, 1, (unsigned)IBM_MAX_BODIES, kind, rotate, state, params, staged, rest, nb, live, history_row);
  return 0;
}
// state [nb][16] advanced in place by one step with loads [nb][6]
extern "C" int integrate_cpu(int nb, const int32_t* kind, const int32_t* rotate, const double* params, const double* loads, double* state,
                             unsigned long long* status) {
  if (nb > IBM_MAX_BODIES) return 1;
  launch(k_ibm_integrate, 1, (unsigned)IBM_MAX_BODIES, kind, rotate, params, loads, nb, state, status);
  return 0;
}
// the move with the live table, as csrc/ibm.hip launches it behind k_ibm_pose
extern "C" int move_live_cpu(int64_t n, const int32_t* move_id, const double* centre0, const double* live, const float* pos0, float* pos, float* vel) {
  launch(k_ibm_move, (size_t)(n + 255) / 256, 256u, pos0, move_id, live, centre0, n, pos, vel);
  return 0;
}
