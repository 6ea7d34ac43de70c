// The closed-loop BeerGame rollout kernels with the float32 MLP policy (scg_bg_mlp.h;
// scg_beergame_kernels.h: bg_rollout_kernel with MlpArgs as its source) instantiated for levels
// 1-8, both variants, ring in LDS and in HBM, behind their launcher: a unit of its own, compiled
// beside the per-level units.
#include "scg_beergame_kernels.h"

namespace scg {

int bg_launch_mlp_rollout(int L, int variant, dim3 grid, hipStream_t s, const BgArgs& a, int32_t K,
                          const RolloutWeeks& weeks, const MlpArgs& ma) {
  switch (L) {
#define X(l) \
  case l: return bg_launch_rollout<l>(variant, grid, s, a, K, weeks, ma);
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#undef X
    default: return fail(SCG_ERR_INVALID, "MLP policy rollout: levels=%d outside 1..%d", L, SCG_BG_POLICY_MAX_LEVELS);
  }
}

}  // namespace scg
