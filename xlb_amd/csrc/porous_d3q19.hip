// Instantiates the porous step and its adjoint step (porous_step_kernel.hpp) for D3Q19.
#include "porous_launch.hpp"

namespace xlb {
int launch_porous_d3q19(const PorousLaunch& q) { return launch_porous_lattice<D3Q19>(q); }
int launch_porous_adjoint_d3q19(const PorousAdjointLaunch& q) { return launch_porous_adjoint_lattice<D3Q19>(q); }
}  // namespace xlb
