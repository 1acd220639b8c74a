// Instantiates the fused adjoint step kernel (adjoint_step_kernel.hpp) for D2Q9.
#include "adjoint_launch.hpp"

namespace xlb {
int launch_adjoint_d2q9(const AdjointLaunch& q) { return launch_adjoint_lattice<D2Q9>(q); }
}  // namespace xlb
