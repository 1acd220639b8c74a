// Instantiates the coupled fluid + scalar step kernel (scalar_step_kernel.hpp) for D2Q9.
#include "scalar_launch.hpp"

namespace xlb {
int launch_scalar_d2q9(const ScalarLaunch& q, int coll) { return launch_scalar_lattice<D2Q9>(q, coll); }
}  // namespace xlb
