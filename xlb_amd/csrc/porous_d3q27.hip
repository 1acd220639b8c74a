// Instantiates the porous step and its adjoint step (porous_step_kernel.hpp) for D3Q27.
#include "porous_launch.hpp"

namespace xlb {
int launch_porous_d3q27(const PorousLaunch& q) { return launch_porous_lattice<D3Q27>(q); }
int launch_porous_adjoint_d3q27(const PorousAdjointLaunch& q) { return launch_porous_adjoint_lattice<D3Q27>(q); }
}  // namespace xlb
