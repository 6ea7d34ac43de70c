// The closed-loop BeerGame rollout kernels with the per-env linear policy (bg_rollout_kernel with
// PolicyArgs as its source): a unit of its own, compiled beside the per-level units.
#include "scg_bg_closed_launch.h"

namespace scg {

template int bg_launch_closed<PolicyArgs>(int, int, dim3, hipStream_t, const BgArgs&, int32_t, const RolloutWeeks&,
                                          const PolicyArgs&);

}  // namespace scg
