// The closed-loop BeerGame rollout kernels with the local-information policy
// (bg_rollout_kernel with LocalArgs as its source), and the kernel that writes the policy's
// features of the state as it stands: a unit of its own, compiled beside the per-level units.
#include "scg_bg_closed_launch.h"

namespace scg {

// f[n][l][0..4) of scg_bg_local.h for the state in HBM, one env per lane, L at run time: the
// same feature function and the same live mask as the rollout, each row word read where the
// rollout reads it.
__global__ __launch_bounds__(kBlock) void bg_local_features_kernel(const BgArgs a, int32_t L, int32_t w0, uint64_t live,
                                                                   int32_t last_fixed, int32_t* __restrict__ out) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (n >= a.n) return;
  const int64_t row = n * L;
  const int64_t stride = a.n * L;
  const int32_t last_demand = local_last_demand(a, n, w0, last_fixed);
  for (int32_t l = 0; l < L; ++l) {
    const int32_t inv[1] = {a.inv[row + l]}, bk[1] = {a.bk[row + l]};
    int32_t net[1];
    policy_obs<1>(inv, bk, a.max_stock, net);
    int32_t transit = 0;
    for (uint64_t m = live; m; m &= m - 1)
      transit = local_wrap_add(transit, a.ring[((w0 + 1 + __builtin_ctzll(m)) % a.ring_slots) * stride + row + l]);
    int32_t f[kLocalFeatures];
    local_level_features(net[0], a.op[row + l], l + 1 < L ? a.bk[row + l + 1] : 0, transit,
                         l ? a.op[row + l - 1] : last_demand, f);
#pragma unroll
    for (int j = 0; j < kLocalFeatures; ++j) out[(row + l) * kLocalFeatures + j] = f[j];
  }
}

int bg_launch_local_features(dim3 grid, hipStream_t s, const BgArgs& a, int32_t L, int32_t w0, uint64_t live,
                             int32_t last_fixed, int32_t* out) {
  hipLaunchKernelGGL(bg_local_features_kernel, grid, dim3(kBlock), 0, s, a, L, w0, live, last_fixed, out);
  return check_launch("bg_local_features_kernel");
}

template int bg_launch_closed<LocalArgs>(int, int, dim3, hipStream_t, const BgArgs&, int32_t, const RolloutWeeks&,
                                         const LocalArgs&);

}  // namespace scg
