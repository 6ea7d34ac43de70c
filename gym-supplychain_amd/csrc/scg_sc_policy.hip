// SupplyChain closed loop, host side and the small kernels (include/scgpu.h scg_sc_observe,
// scg_sc_rollout_policy): the observation of a state as it stands, the action rows of a
// linear policy from observation rows (csrc/scg_sc_policy.h: the one definition of the
// formula), and the entry point that runs either the fused kernel (scg_sc_nodes.hip
// sc_policy_rollout_nodes_kernel) or, for every other config, the action kernel and
// scg_sc_step per step.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "scg_common.h"
#include "scg_supplychain_core.h"
#include "scg_supplychain_args.h"
#include "scg_sc_policy.h"

namespace scg {

// scg_supplychain.hip
int sc_host_check(const scg_sc_config* cfg, const scg_sc_state* st);
ScArgs sc_host_args(const scg_sc_config* cfg, const scg_sc_state* st);
int sc_rollout_chunk_steps();
// scg_sc_nodes.hip
int sc_launch_nodes_policy(const ScArgs& a, const ScPolicyLaunch& p, int maxd_bucket, int W, int E, int K, hipStream_t s);

// sc_reset_kernel's addressing without the reset: env n's observation at a.t of a.episode.
__global__ __launch_bounds__(kScBlock) void sc_observe_kernel(const ScArgs a) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kScBlock + threadIdx.x;
  if (n >= a.n) return;
  ScEnv e = env_view(a, n, a.episode);
  ObsRow out{a.obs, n * a.c.O, a.obs_f64};
  sc_observe(a.c, e, a.t, out);
}

// Action q of env n, thread q * N + n (env fastest: a wave reads each parameter word of its
// envs as one row), from row n of obs [N][O] into row n of out0 and, when given, out1 [N][A].
constexpr int kPolicyActBlock = 256;
constexpr int kPolicyActChunk = 16;
__global__ __launch_bounds__(kPolicyActBlock) void sc_policy_act_kernel(const ScPolicyView pv, const void* obs, int obs_f64,
                                                                         int64_t N, int A, int O, float* out0, float* out1) {
  const int64_t id = static_cast<int64_t>(blockIdx.x) * kPolicyActBlock + threadIdx.x;
  if (id >= N * A) return;
  const int q = static_cast<int>(id / N);
  const int64_t n = id - static_cast<int64_t>(q) * N;
  float act;
  if (obs_f64) {
    const double* row = static_cast<const double*>(obs) + n * O;
    act = sc_policy_action<kPolicyActChunk>(pv, O, n, q, [&](int j) { return static_cast<float>(row[j]); });
  } else {
    const float* row = static_cast<const float*>(obs) + n * O;
    act = sc_policy_action<kPolicyActChunk>(pv, O, n, q, [&](int j) { return row[j]; });
  }
  out0[n * A + q] = act;
  if (out1) out1[n * A + q] = act;
}

// sum = (add ? sum : 0.0) + r: the per-step path's reward_sum.
__global__ __launch_bounds__(kPolicyActBlock) void sc_reward_sum_kernel(double* sum, const double* r, int64_t N, int add) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kPolicyActBlock + threadIdx.x;
  if (n >= N) return;
  const double s = add ? sum[n] : 0.0;
  sum[n] = s + r[n];
}

}  // namespace scg

using namespace scg;

extern "C" {

int scg_sc_observe(const scg_sc_config* cfg, const scg_sc_state* st, void* obs, void* stream) {
  if (int rc = sc_host_check(cfg, st)) return rc;
  if (!obs) return fail(SCG_ERR_INVALID, "the obs buffer is required");
  if (st->time_step < 0) return fail(SCG_ERR_NOT_RESET, "observe() before reset()");
  ScArgs a = sc_host_args(cfg, st);
  a.obs = obs;
  a.t = st->time_step;
  const dim3 grid(static_cast<unsigned>((st->n_envs + kScBlock - 1) / kScBlock));
  hipLaunchKernelGGL(sc_observe_kernel, grid, dim3(kScBlock), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("sc_observe_kernel");
}

int scg_sc_rollout_policy(const scg_sc_config* cfg, scg_sc_state* st, int32_t n_steps, const scg_sc_policy* policy,
                          void* obs_io, float* act_work, float* actions_out, void* obs_out, double* rewards_out,
                          double* reward_sum, void* terminal_obs, uint32_t flags, int32_t* n_done, void* stream) {
  if (int rc = sc_host_check(cfg, st)) return rc;
  if (!policy || !policy->params) return fail(SCG_ERR_INVALID, "a policy with device parameters is required");
  if (!sc_policy_valid(policy->kind, policy->act_lo, policy->act_hi))
    return fail(SCG_ERR_INVALID, "policy: kind must be SCG_SC_POLICY_LINEAR, act_lo <= act_hi, both finite");
  if (!obs_io || !act_work || !reward_sum) return fail(SCG_ERR_INVALID, "obs_io/act_work/reward_sum buffers are required");
  if (n_steps < 0) return fail(SCG_ERR_INVALID, "rollout of %d steps", n_steps);
  if (flags & ~(SCG_BG_AUTORESET | SCG_SC_SERIAL)) return fail(SCG_ERR_INVALID, "unknown rollout flags");
  const bool fused = cfg->kernel == SCG_SC_KERNEL_NODES && !st->ledger;
  if (!fused && !rewards_out)
    return fail(SCG_ERR_INVALID, "the per-step closed loop (every config but node-parallel without ledgers) needs rewards_out");
  if (st->time_step < 0) return fail(SCG_ERR_NOT_RESET, "rollout_policy() before reset()");
  const int T = cfg->total_time_steps;
  if (st->time_step >= T) return fail(SCG_ERR_PAST_HORIZON, "rollout_policy() after the terminal step %d", T);
  const bool reset = flags & SCG_BG_AUTORESET;
  if (!reset && static_cast<int64_t>(st->time_step) + n_steps > T)
    return fail(SCG_ERR_PAST_HORIZON, "rollout_policy() of %d steps from step %d passes the terminal step %d", n_steps,
                st->time_step, T);
  if (fused && (cfg->layout != SCG_SC_LAYOUT_ENV_FASTEST || cfg->inbox_size < 0))
    return fail(SCG_ERR_INVALID, "node-parallel kernel needs the layout and inbox scg_sc_prepare derives");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t N = st->n_envs;
  const int A = cfg->n_actions, O = cfg->n_obs;
  const size_t obs_row = static_cast<size_t>(N) * O * (cfg->obs_f64 ? 8 : 4);
  const ScPolicyView pv = sc_policy_view(policy->params, policy->shared != 0, N, policy->act_lo, policy->act_hi);
  int32_t crossed = 0;
  if (n_done) *n_done = 0;
  if (n_steps == 0) {
    if (hipMemsetAsync(reward_sum, 0, sizeof(double) * N, s) != hipSuccess) return fail(SCG_ERR_HIP, "reward_sum clear");
    return SCG_OK;
  }
  if (!fused) {  // the action kernel and one step launch per step
    const uint32_t step_flags = flags & (SCG_BG_AUTORESET | SCG_SC_SERIAL);
    const dim3 agrid(static_cast<unsigned>((N * A + kPolicyActBlock - 1) / kPolicyActBlock));
    const dim3 rgrid(static_cast<unsigned>((N + kPolicyActBlock - 1) / kPolicyActBlock));
    unsigned char* const oo = static_cast<unsigned char*>(obs_out);
    for (int32_t k = 0; k < n_steps; ++k) {
      const void* src = (k == 0 || !oo) ? obs_io : oo + obs_row * (k - 1);
      float* const arow = actions_out ? actions_out + static_cast<int64_t>(k) * N * A : nullptr;
      hipLaunchKernelGGL(sc_policy_act_kernel, agrid, dim3(kPolicyActBlock), 0, s, pv, src, cfg->obs_f64, N, A, O, act_work,
                         arow);
      if (int rc = check_launch("sc_policy_act_kernel")) return rc;
      int32_t done = 0;
      double* const rrow = rewards_out + static_cast<int64_t>(k) * N;
      if (int rc = scg_sc_step(cfg, st, act_work, oo ? static_cast<void*>(oo + obs_row * k) : obs_io, rrow, terminal_obs,
                               step_flags, &done, stream))
        return rc;
      crossed += done;
      hipLaunchKernelGGL(sc_reward_sum_kernel, rgrid, dim3(kPolicyActBlock), 0, s, reward_sum, rrow, N, k > 0 ? 1 : 0);
      if (int rc = check_launch("sc_reward_sum_kernel")) return rc;
    }
    if (oo && hipMemcpyAsync(obs_io, oo + obs_row * (n_steps - 1), obs_row, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return fail(SCG_ERR_HIP, "obs_io copy");
    if (n_done) *n_done = crossed;
    return SCG_OK;
  }
  const int maxd = sc_maxd_bucket(cfg->max_dests);
  const int chunk = sc_rollout_chunk_steps();
  // launches of at most `chunk` steps, as scg_sc_rollout cuts them: each ends with the state,
  // obs_io and reward_sum written back, and the next one starts from those
  for (int32_t k0 = 0; k0 < n_steps; k0 += chunk) {
    const int32_t kc = std::min<int32_t>(chunk, n_steps - k0);
    ScArgs a = sc_host_args(cfg, st);
    a.obs = obs_out ? static_cast<unsigned char*>(obs_out) + obs_row * k0 : nullptr;
    a.term_obs = terminal_obs;
    a.rew = rewards_out ? rewards_out + static_cast<int64_t>(k0) * N : nullptr;
    a.t = st->time_step + 1;
    a.flags = (reset ? 2 : 0) | ((flags & SCG_SC_SERIAL) ? 4 : 0);
    const ScPolicyLaunch p{pv, obs_io, act_work, actions_out ? actions_out + static_cast<int64_t>(k0) * N * A : nullptr,
                           reward_sum, k0 > 0 ? 1 : 0};
    if (int rc = sc_launch_nodes_policy(a, p, maxd, cfg->group, cfg->inbox_size, kc, s)) return rc;
    const int64_t end = static_cast<int64_t>(st->time_step) + kc;  // <= T without auto-reset
    if (reset) {
      crossed += static_cast<int32_t>(end / T);
      st->episode += static_cast<uint32_t>(end / T);
      st->time_step = static_cast<int32_t>(end % T);
    } else {
      crossed += end == T ? 1 : 0;
      st->time_step = static_cast<int32_t>(end);
    }
  }
  if (n_done) *n_done = crossed;
  return SCG_OK;
}

}  // extern "C"
