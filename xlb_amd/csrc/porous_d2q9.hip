// Instantiates the porous step and its adjoint step (porous_step_kernel.hpp) for D2Q9.
#include "porous_launch.hpp"

namespace xlb {
int launch_porous_d2q9(const PorousLaunch& q) { return launch_porous_lattice<D2Q9>(q); }
int launch_porous_adjoint_d2q9(const PorousAdjointLaunch& q) { return launch_porous_adjoint_lattice<D2Q9>(q); }
}  // namespace xlb
