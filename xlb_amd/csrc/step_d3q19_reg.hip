// Instantiates the fused step kernel for D3Q19 with the regularised collisions (step_launch.hpp: launch_step_reg_lattice).
#include "step_launch.hpp"

namespace xlb {
int launch_step_d3q19_reg(const StepLaunch& p, int coll) { return launch_step_reg_lattice<D3Q19>(p, coll); }
}  // namespace xlb
