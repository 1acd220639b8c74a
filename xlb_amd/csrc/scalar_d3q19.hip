// Instantiates the coupled fluid + scalar step kernel (scalar_step_kernel.hpp) for D3Q19.
#include "scalar_launch.hpp"

namespace xlb {
int launch_scalar_d3q19(const ScalarLaunch& q, int coll) { return launch_scalar_lattice<D3Q19>(q, coll); }
}  // namespace xlb
