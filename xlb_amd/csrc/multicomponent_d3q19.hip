// Instantiates the kernels of the two-component Shan-Chen step (multicomponent_step_kernel.hpp) for D3Q19.
#include "multicomponent_launch.hpp"

namespace xlb {
int launch_multicomponent_d3q19(const MixLaunch& q, MixKernel which) { return launch_mix_lattice<D3Q19>(q, which); }
}  // namespace xlb
