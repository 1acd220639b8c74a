// Instantiates the fused step kernel for D3Q19 with the regularised collisions (projected and recursive,
// each with and without exact-difference forcing): cell.hpp regularized.
#include "step_launch.hpp"

namespace xlb {
int launch_step_d3q19_reg(const StepLaunch& p, int coll) {
  constexpr int RR = COLL_REGULARIZED | COLL_RECURSIVE;
  switch (coll) {
    case COLL_REGULARIZED: return launch_step_ext<D3Q19, COLL_REGULARIZED>(p);
    case COLL_REGULARIZED | COLL_FORCED: return launch_step_ext<D3Q19, COLL_REGULARIZED | COLL_FORCED>(p);
    case RR: return launch_step_ext<D3Q19, RR>(p);
    case RR | COLL_FORCED: return launch_step_ext<D3Q19, RR | COLL_FORCED>(p);
  }
  XLB_FAIL("collision variant %d not built for D3Q19", coll);
}
}  // namespace xlb
