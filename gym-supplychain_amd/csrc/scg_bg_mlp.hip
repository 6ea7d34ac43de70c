// The closed-loop BeerGame rollout kernels with the float32 MLP policy (scg_bg_mlp.h;
// bg_rollout_kernel with MlpArgs as its source): a unit of its own, compiled beside the
// per-level units.
#include "scg_bg_closed_launch.h"

namespace scg {

template int bg_launch_closed<MlpArgs>(int, int, dim3, hipStream_t, const BgArgs&, int32_t, const RolloutWeeks&,
                                       const MlpArgs&);

}  // namespace scg
