// The rigid-body kernels of the immersed-boundary stepper (xlb_amd/csrc/ibm_motion_kernels.hpp) compiled for the host through
// tests/hip_on_cpu: the launches of csrc/ibm.hip, every thread run one after the other in ascending order (k_ibm_loads' tree is
// written so that this gives the bits of the parallel run).  tests/test_ibm_motion_on_cpu.py compares with tests/_ibm_motion_ref.py.
#include "ibm_motion_kernels.hpp"
#include <vector>
thread_local emulated_dim3 threadIdx, blockIdx, blockDim, gridDim;
using namespace xlb;
template <class K, class... A>
static void launch(K k, size_t blocks, unsigned threads, A... a) {
  blockDim.x = threads;
  gridDim.x = (unsigned)blocks;
  for (size_t b = 0; b < blocks; ++b)
    for (unsigned t = 0; t < threads; ++t) { blockIdx.x = (unsigned)b; threadIdx.x = t; k(a...); }
}
// pos / vel hold the uploaded arrays on entry and the moved ones on return; pose [nb][18], centre0 [nb][3]
extern "C" int move_cpu(int64_t n, int nb, const int64_t* first, const int64_t* count, const int* moving, const double* centre0, const double* pose,
                        const float* pos0, float* pos, float* vel) {
  const IbmBodyTables t = ibm_body_tables(n, nb, first, count, moving, centre0);  // the tables xlbhip_ibm_set_bodies uploads
  if (!t.error.empty()) return 1;
  launch(k_ibm_move, (size_t)(n + 255) / 256, 256u, pos0, (const int32_t*)t.move_id.data(), pose, centre0, n, pos, vel);
  return 0;
}
// F (n, 3) in the compute dtype (f32 != 0: float, else double) -> loads [nb][6]
extern "C" int loads_cpu(int64_t n, int nb, const int64_t* first, const int64_t* count, const double* pose, int f32, const void* F, const float* area,
                         const float* pos, double* loads, double* history_row) {
  const int moving[IBM_MAX_BODIES] = {};
  const double centre0[IBM_MAX_BODIES * 3] = {};  // (the chunks do not depend on them)
  const IbmBodyTables t = ibm_body_tables(n, nb, first, count, moving, centre0);
  if (!t.error.empty()) return 1;
  std::vector<double> partial(t.chunks.size() * 6 + 1, 0.0);
  if (!t.chunks.empty()) {
    if (f32) launch(k_ibm_loads<float>, t.chunks.size(), (unsigned)IBM_LOADS_CHUNK, t.chunks.data(), (const float*)F, area, pos, pose, partial.data());
    else launch(k_ibm_loads<double>, t.chunks.size(), (unsigned)IBM_LOADS_CHUNK, t.chunks.data(), (const double*)F, area, pos, pose, partial.data());
  }
  launch(k_ibm_loads_combine, (size_t)(nb * 6 + 255) / 256, 256u, (const int32_t*)t.chunk0.data(), (const double*)partial.data(), nb, loads, history_row);
  return 0;
}
