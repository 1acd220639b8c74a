// Instantiates the kernels of the two-component Shan-Chen step (multicomponent_step_kernel.hpp) for D2Q9.
#include "multicomponent_launch.hpp"

namespace xlb {
int launch_multicomponent_d2q9(const MixLaunch& q, MixKernel which) { return launch_mix_lattice<D2Q9>(q, which); }
}  // namespace xlb
