// Instantiates the fused adjoint step kernel (adjoint_step_kernel.hpp) for D3Q27.
#include "adjoint_launch.hpp"

namespace xlb {
int launch_adjoint_d3q27(const AdjointLaunch& q) { return launch_adjoint_lattice<D3Q27>(q); }
}  // namespace xlb
