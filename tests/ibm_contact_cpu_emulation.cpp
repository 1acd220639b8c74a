// The free-body integrator with virtual mass and contact (k_ibm_integrate_contact of xlb_amd/csrc/ibm_dynamics_kernels.hpp) compiled
// for the host through tests/hip_on_cpu: the launches of csrc/ibm.hip — one block of IBM_MAX_BODIES threads — every thread run one
// after the other.  tests/test_ibm_contact_on_cpu.py compares with tests/_ibm_contact_ref.py.
#include "ibm_dynamics_kernels.hpp"
thread_local emulated_dim3 threadIdx, blockIdx, blockDim, gridDim;
using namespace xlb;
template <class K, class... A>
static void launch(K k, unsigned threads, A... a) {
  blockDim.x = threads;
  gridDim.x = 1;
  blockIdx.x = 0;
  for (unsigned t = 0; t < threads; ++t) { threadIdx.x = t; k(a...); }
}
// live [nb][18] of one step; staged may be null
extern "C" int pose_table_cpu(int nb, const int32_t* kind, const int32_t* rotate, const double* state, const double* params, const double* staged,
                              const double* rest, double* live) {
  if (nb > IBM_MAX_BODIES) return 1;
  launch(k_ibm_pose, (unsigned)IBM_MAX_BODIES, kind, rotate, state, params, staged, rest, nb, live, (double*)nullptr);
  return 0;
}
// state [nb][16] and prev [nb][6] advanced in place by one step with loads [nb][6]; model: range | stiffness | wall stiffness | lo[3] |
// hi[3]; radius may be null (no contact); contact [nb][3] is written
extern "C" int integrate_contact_cpu(int nb, const int32_t* kind, const int32_t* rotate, const double* params, const double* loads, double* state,
                                     unsigned long long* status, const double* virt, double* prev, const double* radius, const double* model,
                                     const double* live, double* contact) {
  if (nb > IBM_MAX_BODIES) return 1;
  const IbmContactModel M{model[0], model[1], model[2], {model[3], model[4], model[5]}, {model[6], model[7], model[8]}};
  launch(k_ibm_integrate_contact, (unsigned)IBM_MAX_BODIES, kind, rotate, params, loads, nb, state, status, virt, prev, radius, M, live, contact);
  return 0;
}
