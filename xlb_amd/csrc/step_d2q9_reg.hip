// Instantiates the fused step kernel for D2Q9 with the regularised collisions (projected and recursive,
// each with and without exact-difference forcing): cell.hpp regularized.
#include "step_launch.hpp"

namespace xlb {
int launch_step_d2q9_reg(const StepLaunch& p, int coll) {
  constexpr int RR = COLL_REGULARIZED | COLL_RECURSIVE;
  switch (coll) {
    case COLL_REGULARIZED: return launch_step_ext<D2Q9, COLL_REGULARIZED>(p);
    case COLL_REGULARIZED | COLL_FORCED: return launch_step_ext<D2Q9, COLL_REGULARIZED | COLL_FORCED>(p);
    case RR: return launch_step_ext<D2Q9, RR>(p);
    case RR | COLL_FORCED: return launch_step_ext<D2Q9, RR | COLL_FORCED>(p);
  }
  XLB_FAIL("collision variant %d not built for D2Q9", coll);
}
}  // namespace xlb
