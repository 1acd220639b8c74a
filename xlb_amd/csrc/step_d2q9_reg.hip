// Instantiates the fused step kernel for D2Q9 with the regularised collisions (step_launch.hpp: launch_step_reg_lattice).
#include "step_launch.hpp"

namespace xlb {
int launch_step_d2q9_reg(const StepLaunch& p, int coll) { return launch_step_reg_lattice<D2Q9>(p, coll); }
}  // namespace xlb
