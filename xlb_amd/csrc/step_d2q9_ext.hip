// Instantiates the fused step kernel for D2Q9 with the extended collisions (step_launch.hpp: launch_step_ext_lattice).
#include "step_launch.hpp"

namespace xlb {
int launch_step_d2q9_ext(const StepLaunch& p, int coll) { return launch_step_ext_lattice<D2Q9>(p, coll); }
}  // namespace xlb
