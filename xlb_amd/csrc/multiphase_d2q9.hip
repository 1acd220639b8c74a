// Instantiates the kernels of the Shan-Chen step (multiphase_step_kernel.hpp) for D2Q9.
#include "multiphase_launch.hpp"

namespace xlb {
int launch_multiphase_d2q9(const MultiphaseLaunch& q, MultiphaseKernel which) { return launch_multiphase_lattice<D2Q9>(q, which); }
}  // namespace xlb
