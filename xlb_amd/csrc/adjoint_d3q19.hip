// Instantiates the fused adjoint step kernel (adjoint_step_kernel.hpp) for D3Q19.
#include "adjoint_launch.hpp"

namespace xlb {
int launch_adjoint_d3q19(const AdjointLaunch& q) { return launch_adjoint_lattice<D3Q19>(q); }
}  // namespace xlb
