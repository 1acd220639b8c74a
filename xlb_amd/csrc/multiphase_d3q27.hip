// Instantiates the kernels of the Shan-Chen step (multiphase_step_kernel.hpp) for D3Q27.
#include "multiphase_launch.hpp"

namespace xlb {
int launch_multiphase_d3q27(const MultiphaseLaunch& q, MultiphaseKernel which) { return launch_multiphase_lattice<D3Q27>(q, which); }
}  // namespace xlb
