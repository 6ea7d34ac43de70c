// The closed-loop BeerGame rollout kernels (scg_beergame_kernels.h: bg_policy_rollout_kernel,
// bg_policy_rollout_lds_kernel and BeerGameEnv2's pair) instantiated for levels 1-8, and their
// launcher: a unit of its own, compiled beside the per-level units.
#include "scg_beergame_kernels.h"

namespace scg {

template <int L>
static int launch_policy_level(int variant, dim3 grid, hipStream_t s, const BgArgs& a, int32_t K,
                               const RolloutWeeks& weeks, const PolicyArgs& pa) {
  const size_t lds = static_cast<size_t>(a.ring_slots) * L * kBlock * sizeof(int32_t);
  const bool in_lds = lds <= 64 * 1024;  // ring staged in LDS for the launch (bg_launch_rollout's rule)
  if (variant == 2) {
    if (in_lds) {
      hipLaunchKernelGGL(bg2_policy_rollout_lds_kernel<L>, grid, dim3(kBlock), lds, s, a, K, weeks, pa);
      return check_launch("bg2_policy_rollout_lds_kernel");
    }
    hipLaunchKernelGGL(bg2_policy_rollout_kernel<L>, grid, dim3(kBlock), 0, s, a, K, weeks, pa);
    return check_launch("bg2_policy_rollout_kernel");
  }
  if (in_lds) {
    hipLaunchKernelGGL(bg_policy_rollout_lds_kernel<L>, grid, dim3(kBlock), lds, s, a, K, weeks, pa);
    return check_launch("bg_policy_rollout_lds_kernel");
  }
  hipLaunchKernelGGL(bg_policy_rollout_kernel<L>, grid, dim3(kBlock), 0, s, a, K, weeks, pa);
  return check_launch("bg_policy_rollout_kernel");
}

int bg_launch_policy_rollout(int L, int variant, dim3 grid, hipStream_t s, const BgArgs& a, int32_t K,
                             const RolloutWeeks& weeks, const PolicyArgs& pa) {
  switch (L) {
#define X(l) \
  case l: return launch_policy_level<l>(variant, grid, s, a, K, weeks, pa);
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#undef X
    default: return fail(SCG_ERR_INVALID, "policy rollout: levels=%d outside 1..%d", L, SCG_BG_POLICY_MAX_LEVELS);
  }
}

}  // namespace scg
