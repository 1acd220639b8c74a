// Instantiates the fused step kernel for D3Q19 with the extended collisions (step_launch.hpp: launch_step_ext_lattice).
#include "step_launch.hpp"

namespace xlb {
int launch_step_d3q19_ext(const StepLaunch& p, int coll) { return launch_step_ext_lattice<D3Q19>(p, coll); }
}  // namespace xlb
