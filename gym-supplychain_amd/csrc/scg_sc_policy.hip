// SupplyChain closed loop, host side and the small kernels (include/scgpu.h scg_sc_observe,
// scg_sc_rollout_policy, scg_sc_rollout_mlp, scg_sc_rollout_sampled, scg_sc_rollout_drawn,
// scg_sc_noise_fill): the observation of a state
// as it stands, the action rows of a linear policy or a one-hidden-layer ReLU policy from
// observation rows, deterministic or with noise added before the clamp, the caller's or drawn here
// (csrc/scg_sc_policy.h, csrc/scg_sc_mlp.h, csrc/scg_normal.h: the one definition of each formula), and the entry
// points, one host body for both policies, which runs either the fused kernel (scg_sc_nodes.hip
// sc_closed_rollout_nodes_kernel) or, for every other case, the action kernel and scg_sc_step
// per step.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "scg_common.h"
#include "scg_supplychain_core.h"
#include "scg_supplychain_args.h"
#include "scg_sc_nodes_launch.h"

namespace scg {

// scg_supplychain.hip
int sc_host_check(const scg_sc_config* cfg, const scg_sc_state* st);
ScArgs sc_host_args(const scg_sc_config* cfg, const scg_sc_state* st);
int sc_rollout_chunk_steps();

// sc_reset_kernel's addressing without the reset: env n's observation at a.t of a.episode.
__global__ __launch_bounds__(kScBlock) void sc_observe_kernel(const ScArgs a) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kScBlock + threadIdx.x;
  if (n >= a.n) return;
  ScEnv e = env_view(a, n, a.episode);
  ObsRow out{a.obs, n * a.c.O, a.obs_f64};
  sc_observe(a.c, e, a.t, out);
}

// f(o), for o(j) the float32 of element j of row n of obs [N][O], float64 or float32. (The
// callers' f capture the thread's indices by value: captured by reference they compiled to
// other code for the four action kernels, whose instruction counts are pinned.)
template <class F>
__device__ __forceinline__ auto sc_with_obs_row(const void* obs, int obs_f64, int64_t n, int O, const F& f) {
  if (obs_f64) {
    const double* row = static_cast<const double*>(obs) + n * O;
    return f([&](int j) { return static_cast<float>(row[j]); });
  } else {
    const float* row = static_cast<const float*>(obs) + n * O;
    return f([&](int j) { return row[j]; });
  }
}

// Action q of env n, thread q * N + n (env fastest: a wave reads each parameter word of its
// envs as one row), from row n of obs [N][O] into row n of out0 and, when given, out1 [N][A].
// kSampled (scg_sc_rollout_sampled): smp.noise and, when given, smp.samples are the step's rows
// [N][A] of the call's noise and samples_out; a thread reads its element of the one and then
// writes the same element of the other, so the two may be one buffer.
// A drawn step (scg_sc_rollout_drawn) passes an ScDrawView for smp: the same, with the element not
// read but computed (sc_drawn_noise: element (n, q) of the step's row).
constexpr int kPolicyActBlock = 256;
constexpr int kPolicyActChunk = 16;
__device__ __forceinline__ float sc_drawn_noise(const ScDrawView& drw, int64_t n, int q) {
  return sc_noise_element(drw.k0, drw.k1, drw.row0, drw.env0 + static_cast<uint32_t>(n), static_cast<uint32_t>(q));
}
template <bool kSampled, class Noise>
__device__ __forceinline__ void sc_policy_act(const ScPolicyView& pv, const void* obs, int obs_f64, int64_t N, int A, int O,
                                              float* out0, float* out1, const Noise& smp) {
  const int64_t id = static_cast<int64_t>(blockIdx.x) * kPolicyActBlock + threadIdx.x;
  if (id >= N * A) return;
  const int q = static_cast<int>(id / N);
  const int64_t n = id - static_cast<int64_t>(q) * N;
  [[maybe_unused]] float sd, e, u;  // the sampled body's alone: set and read only under kSampled
  if constexpr (std::is_same_v<Noise, ScDrawView>) {
    sd = smp.std[q], e = sc_drawn_noise(smp, n, q);
  } else if constexpr (kSampled) {
    sd = smp.std[q], e = smp.noise[n * A + q];
  }
  float* const u_out = &u;
  const float act = sc_with_obs_row(obs, obs_f64, n, O, [=, &pv](auto o) {
    if constexpr (kSampled) {
      return sc_policy_action_sampled<kPolicyActChunk>(pv, O, n, q, o, sd, e, u_out);
    } else {
      return sc_policy_action<kPolicyActChunk>(pv, O, n, q, o);
    }
  });
  out0[n * A + q] = act;
  if (out1) out1[n * A + q] = act;
  if constexpr (kSampled)
    if (smp.samples) smp.samples[n * A + q] = u;
}

// The three kernels of it: the deterministic one takes no noise arguments.
__global__ __launch_bounds__(kPolicyActBlock) void sc_policy_act_kernel(const ScPolicyView pv, const void* obs, int obs_f64,
                                                                         int64_t N, int A, int O, float* out0, float* out1) {
  sc_policy_act<false>(pv, obs, obs_f64, N, A, O, out0, out1, ScSampleView{});
}
__global__ __launch_bounds__(kPolicyActBlock) void sc_policy_act_sampled_kernel(const ScPolicyView pv, const void* obs,
                                                                                 int obs_f64, int64_t N, int A, int O,
                                                                                 float* out0, float* out1, const float* std,
                                                                                 const float* eps, float* samples) {
  sc_policy_act<true>(pv, obs, obs_f64, N, A, O, out0, out1, ScSampleView{std, eps, samples});
}
__global__ __launch_bounds__(kPolicyActBlock) void sc_policy_act_drawn_kernel(const ScPolicyView pv, const void* obs, int obs_f64,
                                                                               int64_t N, int A, int O, float* out0, float* out1,
                                                                               const ScDrawView drw) {
  sc_policy_act<true>(pv, obs, obs_f64, N, A, O, out0, out1, drw);
}

// sum = (add ? sum : 0.0) + r: the per-step path's reward_sum.
__global__ __launch_bounds__(kPolicyActBlock) void sc_reward_sum_kernel(double* sum, const double* r, int64_t N, int add) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kPolicyActBlock + threadIdx.x;
  if (n >= N) return;
  const double s = add ? sum[n] : 0.0;
  sum[n] = s + r[n];
}

// The MLP's action rows: thread l of a block is env blockIdx.x * 64 + l. It computes its env's H
// hidden units from row n of obs [N][O] into its column of the block's hidden tile [H][64] in
// dynamic LDS (lane fastest: conflict-free, and no register array that H = 64 would spill; 256 B
// per unit, 16 KB at most), then its A
// actions from that column into row n of out0 and, when given, out1 [N][A]. A thread reads and
// writes its own column only: no barrier. Per-env parameter words are read as 256-byte rows.
constexpr int kMlpActBlock = 64;
constexpr int kMlpActChunk = 16;
// kSampled: smp as sc_policy_act's, the env's row read and written by the env's thread.
template <bool kSampled, class Noise>
__device__ __forceinline__ void sc_mlp_act(const ScMlpView& mv, const void* obs, int obs_f64, int64_t N, int A, int O,
                                           float* out0, float* out1, const Noise& smp) {
  extern __shared__ float hid_t[];  // [H][64]
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kMlpActBlock + threadIdx.x;
  if (n >= N) return;
  float* const hid = hid_t + threadIdx.x;
  sc_with_obs_row(obs, obs_f64, n, O, [=, &mv](auto o) {
    for (int i = 0; i < mv.H; ++i) hid[i * kMlpActBlock] = sc_mlp_hidden<kMlpActChunk>(mv, O, n, i, o);
  });
  auto h = [&](int i) { return hid[i * kMlpActBlock]; };
  for (int q = 0; q < A; ++q) {
    [[maybe_unused]] float u;
    float act;
    if constexpr (std::is_same_v<Noise, ScDrawView>) {
      act = sc_mlp_action_sampled<kMlpActChunk>(mv, O, n, q, h, smp.std[q], sc_drawn_noise(smp, n, q), &u);
    } else if constexpr (kSampled) {
      act = sc_mlp_action_sampled<kMlpActChunk>(mv, O, n, q, h, smp.std[q], smp.noise[n * A + q], &u);
    } else {
      act = sc_mlp_action<kMlpActChunk>(mv, O, n, q, h);
    }
    out0[n * A + q] = act;
    if (out1) out1[n * A + q] = act;
    if constexpr (kSampled)
      if (smp.samples) smp.samples[n * A + q] = u;
  }
}

// The three kernels of it. (Four waves per SIMD: at most 128 VGPRs, as the node-parallel kernels.)
__global__ __launch_bounds__(kMlpActBlock) __attribute__((amdgpu_waves_per_eu(4)))
void sc_mlp_act_kernel(const ScMlpView mv, const void* obs, int obs_f64, int64_t N, int A, int O, float* out0, float* out1) {
  sc_mlp_act<false>(mv, obs, obs_f64, N, A, O, out0, out1, ScSampleView{});
}
__global__ __launch_bounds__(kMlpActBlock) __attribute__((amdgpu_waves_per_eu(4)))
void sc_mlp_act_sampled_kernel(const ScMlpView mv, const void* obs, int obs_f64, int64_t N, int A, int O, float* out0,
                               float* out1, const float* std, const float* eps, float* samples) {
  sc_mlp_act<true>(mv, obs, obs_f64, N, A, O, out0, out1, ScSampleView{std, eps, samples});
}
__global__ __launch_bounds__(kMlpActBlock) __attribute__((amdgpu_waves_per_eu(4)))
void sc_mlp_act_drawn_kernel(const ScMlpView mv, const void* obs, int obs_f64, int64_t N, int A, int O, float* out0,
                             float* out1, const ScDrawView drw) {
  sc_mlp_act<true>(mv, obs, obs_f64, N, A, O, out0, out1, drw);
}

// Rows of the drawn loop's noise as a tensor (scg_sc_noise_fill): thread id is group g = id % G of
// element row id / G of out [K * N][A], G = ceil(A / 4) groups of 4 consecutive actions: one
// Philox block, both pairs, up to four stores next to the neighbouring threads'.
constexpr int kNoiseFillBlock = 256;
__global__ __launch_bounds__(kNoiseFillBlock) void sc_noise_fill_kernel(float* out, int64_t rows, int64_t N, int A, int G,
                                                                        uint32_t k0, uint32_t k1, uint32_t row0, uint32_t env0) {
  const int64_t id = static_cast<int64_t>(blockIdx.x) * kNoiseFillBlock + threadIdx.x;
  if (id >= rows * G) return;
  const int64_t kn = id / G;
  const int g = static_cast<int>(id - kn * G);
  const int64_t k = kn / N, n = kn - k * N;
  const U4 b = sc_noise_block(k0, k1, row0 + static_cast<uint32_t>(k), env0 + static_cast<uint32_t>(n), static_cast<uint32_t>(g));
  const NormalPair p0 = normal_from_words(b.x, b.y), p1 = normal_from_words(b.z, b.w);
  float* const o = out + kn * A + 4 * g;
  const int left = A - 4 * g;
  o[0] = p0.c;
  if (left > 1) o[1] = p0.s;
  if (left > 2) o[2] = p1.c;
  if (left > 3) o[3] = p1.s;
}

// The transform alone on the caller's word pairs (scg_noise_from_words).
__global__ __launch_bounds__(kNoiseFillBlock) void noise_from_words_kernel(const uint32_t* words, float* out, int64_t n) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kNoiseFillBlock + threadIdx.x;
  if (i >= n) return;
  const NormalPair p = normal_from_words(words[2 * i], words[2 * i + 1]);
  out[2 * i] = p.c;
  out[2 * i + 1] = p.s;
}

// Whether hidden units fit the LDS the fused kernel has idle for them (a config scg_sc_prepare
// has not derived an inbox for has none).
bool sc_mlp_fits(const scg_sc_config* cfg, int32_t hidden) {
  return cfg->inbox_size >= 0 && hidden <= sc_mlp_fused_hidden_max(cfg->inbox_size, cfg->n_nodes);
}

// What the closed loop's host body needs of a policy: its argument check, whether it fuses
// beyond the linear condition, its view for the fused launch (sc_launch_nodes_closed) and the
// launch of the action rows of one step (smp: the step's rows of a sampled call's noise, drw: a
// drawn call's noise at the step's row; at most one of them, or both null).
struct LinearHost {
  const scg_sc_policy* pol;
  int check() const {
    if (!pol || !pol->params) return fail(SCG_ERR_INVALID, "a policy with device parameters is required");
    if (!sc_policy_valid(pol->kind, pol->act_lo, pol->act_hi))
      return fail(SCG_ERR_INVALID, "policy: kind must be SCG_SC_POLICY_LINEAR, act_lo <= act_hi, both finite");
    return SCG_OK;
  }
  bool fits(const scg_sc_config*) const { return true; }
  ScPolicyView view(int64_t N) const { return sc_policy_view(pol->params, pol->shared != 0, N, pol->act_lo, pol->act_hi); }
  static int act(const ScPolicyView& pv, const void* obs, int obs_f64, int64_t N, int A, int O, float* out0, float* out1,
                 const ScSampleView* smp, const ScDrawView* drw, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>((N * A + kPolicyActBlock - 1) / kPolicyActBlock));
    if (drw) {
      hipLaunchKernelGGL(sc_policy_act_drawn_kernel, grid, dim3(kPolicyActBlock), 0, s, pv, obs, obs_f64, N, A, O, out0, out1, *drw);
      return check_launch("sc_policy_act_drawn_kernel");
    }
    if (smp) {
      hipLaunchKernelGGL(sc_policy_act_sampled_kernel, grid, dim3(kPolicyActBlock), 0, s, pv, obs, obs_f64, N, A, O, out0, out1,
                         smp->std, smp->noise, smp->samples);
      return check_launch("sc_policy_act_sampled_kernel");
    }
    hipLaunchKernelGGL(sc_policy_act_kernel, grid, dim3(kPolicyActBlock), 0, s, pv, obs, obs_f64, N, A, O, out0, out1);
    return check_launch("sc_policy_act_kernel");
  }
};

struct MlpHost {
  const scg_sc_mlp* pol;
  int check() const {
    if (!pol || !pol->params) return fail(SCG_ERR_INVALID, "an mlp with device parameters is required");
    if (!sc_mlp_valid(pol->hidden, pol->activation, pol->reserved, pol->act_lo, pol->act_hi))
      return fail(SCG_ERR_INVALID,
                  "mlp: hidden in 1..%d, activation SCG_SC_ACT_RELU, reserved 0, act_lo <= act_hi, both finite",
                  SCG_SC_MLP_MAX_HIDDEN);
    return SCG_OK;
  }
  bool fits(const scg_sc_config* cfg) const { return sc_mlp_fits(cfg, pol->hidden); }
  ScMlpView view(int64_t N) const {
    return sc_mlp_view(pol->params, pol->shared != 0, N, pol->hidden, pol->act_lo, pol->act_hi);
  }
  static int act(const ScMlpView& mv, const void* obs, int obs_f64, int64_t N, int A, int O, float* out0, float* out1,
                 const ScSampleView* smp, const ScDrawView* drw, hipStream_t s) {
    const dim3 grid(static_cast<unsigned>((N + kMlpActBlock - 1) / kMlpActBlock));
    const size_t lds = sizeof(float) * kMlpActBlock * mv.H;
    if (drw) {
      hipLaunchKernelGGL(sc_mlp_act_drawn_kernel, grid, dim3(kMlpActBlock), lds, s, mv, obs, obs_f64, N, A, O, out0, out1, *drw);
      return check_launch("sc_mlp_act_drawn_kernel");
    }
    if (smp) {
      hipLaunchKernelGGL(sc_mlp_act_sampled_kernel, grid, dim3(kMlpActBlock), lds, s, mv, obs, obs_f64, N, A, O, out0, out1,
                         smp->std, smp->noise, smp->samples);
      return check_launch("sc_mlp_act_sampled_kernel");
    }
    hipLaunchKernelGGL(sc_mlp_act_kernel, grid, dim3(kMlpActBlock), lds, s, mv, obs, obs_f64, N, A, O, out0, out1);
    return check_launch("sc_mlp_act_kernel");
  }
};

// The fused closed loop's condition: scg_sc_rollout's (a node-parallel config, no ledgers).
bool sc_closed_fused(const scg_sc_config* cfg, const scg_sc_state* st) {
  return cfg->kernel == SCG_SC_KERNEL_NODES && !st->ledger;
}

// smp: the call's noise (scg_sc_rollout_sampled), draw: the noise it draws itself
// (scg_sc_rollout_drawn); neither: the deterministic loop.
template <class Policy>
int sc_rollout_closed(const scg_sc_config* cfg, scg_sc_state* st, int32_t n_steps, const Policy& policy,
                      const scg_sc_sampling* smp, const scg_sc_noise_draw* draw, void* obs_io, float* act_work, float* actions_out, void* obs_out,
                      double* rewards_out, double* reward_sum, void* terminal_obs, uint32_t flags, int32_t* n_done,
                      void* stream) {
  if (int rc = sc_host_check(cfg, st)) return rc;
  if (int rc = policy.check()) return rc;
  if (smp) {
    if (smp->reserved != 0) return fail(SCG_ERR_INVALID, "sampling: reserved must be 0");
    if (n_steps > 0 && (!smp->std || !smp->noise)) return fail(SCG_ERR_INVALID, "sampling: device std and noise are required");
  }
  if (draw) {
    if (draw->reserved != 0) return fail(SCG_ERR_INVALID, "noise draw: reserved must be 0");
    if (n_steps > 0 && !draw->std) return fail(SCG_ERR_INVALID, "noise draw: device std is required");
    if (n_steps > 0 && static_cast<int64_t>(draw->row0) + n_steps > (int64_t(1) << 32))
      return fail(SCG_ERR_INVALID, "noise draw: rows %u + %d pass 2^32", draw->row0, n_steps);
  }
  if (!obs_io || !act_work || !reward_sum) return fail(SCG_ERR_INVALID, "obs_io/act_work/reward_sum buffers are required");
  if (n_steps < 0) return fail(SCG_ERR_INVALID, "rollout of %d steps", n_steps);
  if (flags & ~(SCG_BG_AUTORESET | SCG_SC_SERIAL)) return fail(SCG_ERR_INVALID, "unknown rollout flags");
  const bool fused = sc_closed_fused(cfg, st) && policy.fits(cfg);
  if (!fused && !rewards_out)
    return fail(SCG_ERR_INVALID,
                "the per-step closed loop (every case but node-parallel without ledgers, the policy in its LDS) needs "
                "rewards_out");
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
  auto pv = policy.view(N);
  // rows k, k + 1, ... of the call's noise and samples
  auto rows = [&](int32_t k) {
    const int64_t at = sc_sample_index(N, A, k, 0, 0);
    return ScSampleView{smp->std, smp->noise + at, smp->samples_out ? smp->samples_out + at : nullptr};
  };
  // the same of a drawn call: its samples' rows and the global index of row k
  auto drawn_rows = [&](int32_t k) {
    const int64_t at = sc_sample_index(N, A, k, 0, 0);
    return ScDrawView{draw->std, draw->samples_out ? draw->samples_out + at : nullptr, static_cast<uint32_t>(draw->seed),
                      static_cast<uint32_t>(draw->seed >> 32), draw->row0 + static_cast<uint32_t>(k),
                      static_cast<uint32_t>(st->env_offset)};
  };
  int32_t crossed = 0;
  if (n_done) *n_done = 0;
  if (n_steps == 0) {
    if (hipMemsetAsync(reward_sum, 0, sizeof(double) * N, s) != hipSuccess) return fail(SCG_ERR_HIP, "reward_sum clear");
    return SCG_OK;
  }
  if (!fused) {  // the action kernel and one step launch per step
    const uint32_t step_flags = flags & (SCG_BG_AUTORESET | SCG_SC_SERIAL);
    const dim3 rgrid(static_cast<unsigned>((N + kPolicyActBlock - 1) / kPolicyActBlock));
    unsigned char* const oo = static_cast<unsigned char*>(obs_out);
    for (int32_t k = 0; k < n_steps; ++k) {
      const void* src = (k == 0 || !oo) ? obs_io : oo + obs_row * (k - 1);
      float* const arow = actions_out ? actions_out + static_cast<int64_t>(k) * N * A : nullptr;
      const ScSampleView row = smp ? rows(k) : ScSampleView{};
      const ScDrawView drow = draw ? drawn_rows(k) : ScDrawView{};
      if (int rc = Policy::act(pv, src, cfg->obs_f64, N, A, O, act_work, arow, smp ? &row : nullptr, draw ? &drow : nullptr, s))
        return rc;
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
    float* const arows = actions_out ? actions_out + static_cast<int64_t>(k0) * N * A : nullptr;
    const ScClosedLaunch<decltype(pv)> p{pv, obs_io, act_work, arows, reward_sum, k0 > 0 ? 1 : 0};
    const int W = cfg->group, E = cfg->inbox_size;
    if (int rc = draw  ? sc_launch_nodes_closed(a, ScDrawnLaunch<decltype(pv)>{p, drawn_rows(k0)}, maxd, W, E, kc, s)
                 : smp ? sc_launch_nodes_closed(a, ScSampledLaunch<decltype(pv)>{p, rows(k0)}, maxd, W, E, kc, s)
                       : sc_launch_nodes_closed(a, p, maxd, W, E, kc, s))
      return rc;
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
  return sc_rollout_closed(cfg, st, n_steps, LinearHost{policy}, nullptr, nullptr, obs_io, act_work, actions_out, obs_out, rewards_out,
                           reward_sum, terminal_obs, flags, n_done, stream);
}

int scg_sc_rollout_mlp(const scg_sc_config* cfg, scg_sc_state* st, int32_t n_steps, const scg_sc_mlp* mlp, void* obs_io,
                       float* act_work, float* actions_out, void* obs_out, double* rewards_out, double* reward_sum,
                       void* terminal_obs, uint32_t flags, int32_t* n_done, void* stream) {
  return sc_rollout_closed(cfg, st, n_steps, MlpHost{mlp}, nullptr, nullptr, obs_io, act_work, actions_out, obs_out, rewards_out, reward_sum,
                           terminal_obs, flags, n_done, stream);
}

int scg_sc_rollout_sampled(const scg_sc_config* cfg, scg_sc_state* st, int32_t n_steps, const scg_sc_policy* linear,
                           const scg_sc_mlp* mlp, const scg_sc_sampling* smp, void* obs_io, float* act_work, float* actions_out,
                           void* obs_out, double* rewards_out, double* reward_sum, void* terminal_obs, uint32_t flags,
                           int32_t* n_done, void* stream) {
  if (!linear == !mlp) return fail(SCG_ERR_INVALID, "sampled rollout: exactly one of the linear policy and the mlp");
  if (!smp) return fail(SCG_ERR_INVALID, "sampled rollout: the sampling struct is required");
  if (linear)
    return sc_rollout_closed(cfg, st, n_steps, LinearHost{linear}, smp, nullptr, obs_io, act_work, actions_out, obs_out, rewards_out,
                             reward_sum, terminal_obs, flags, n_done, stream);
  return sc_rollout_closed(cfg, st, n_steps, MlpHost{mlp}, smp, nullptr, obs_io, act_work, actions_out, obs_out, rewards_out, reward_sum,
                           terminal_obs, flags, n_done, stream);
}

int scg_sc_rollout_drawn(const scg_sc_config* cfg, scg_sc_state* st, int32_t n_steps, const scg_sc_policy* linear,
                         const scg_sc_mlp* mlp, const scg_sc_noise_draw* draw, void* obs_io, float* act_work, float* actions_out,
                         void* obs_out, double* rewards_out, double* reward_sum, void* terminal_obs, uint32_t flags,
                         int32_t* n_done, void* stream) {
  if (!linear == !mlp) return fail(SCG_ERR_INVALID, "drawn rollout: exactly one of the linear policy and the mlp");
  if (!draw) return fail(SCG_ERR_INVALID, "drawn rollout: the noise draw struct is required");
  if (linear)
    return sc_rollout_closed(cfg, st, n_steps, LinearHost{linear}, nullptr, draw, obs_io, act_work, actions_out, obs_out,
                             rewards_out, reward_sum, terminal_obs, flags, n_done, stream);
  return sc_rollout_closed(cfg, st, n_steps, MlpHost{mlp}, nullptr, draw, obs_io, act_work, actions_out, obs_out, rewards_out,
                           reward_sum, terminal_obs, flags, n_done, stream);
}

int scg_sc_noise_fill(const scg_sc_config* cfg, const scg_sc_state* st, uint64_t seed, uint32_t row0, int32_t n_rows, float* out,
                      void* stream) {
  if (int rc = sc_host_check(cfg, st)) return rc;
  if (n_rows < 0 || static_cast<int64_t>(row0) + n_rows > (int64_t(1) << 32))
    return fail(SCG_ERR_INVALID, "noise fill: rows %u + %d", row0, n_rows);
  if (n_rows == 0) return SCG_OK;
  if (!out) return fail(SCG_ERR_INVALID, "noise fill: the out buffer is required");
  const int A = cfg->n_actions, G = (A + 3) / 4;
  const int64_t rows = static_cast<int64_t>(n_rows) * st->n_envs;
  const int64_t blocks = (rows * G + kNoiseFillBlock - 1) / kNoiseFillBlock;
  if (blocks > 0x7fffffff) return fail(SCG_ERR_INVALID, "noise fill: %lld blocks", static_cast<long long>(blocks));
  hipLaunchKernelGGL(sc_noise_fill_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kNoiseFillBlock), 0,
                     static_cast<hipStream_t>(stream), out, rows, st->n_envs, A, G, static_cast<uint32_t>(seed),
                     static_cast<uint32_t>(seed >> 32), row0, static_cast<uint32_t>(st->env_offset));
  return check_launch("sc_noise_fill_kernel");
}

int scg_noise_from_words(const uint32_t* words, float* out, int64_t n, void* stream) {
  if (n < 0 || (n > 0 && (!words || !out))) return fail(SCG_ERR_INVALID, "noise from words: device words and out are required");
  if (n == 0) return SCG_OK;
  const int64_t blocks = (n + kNoiseFillBlock - 1) / kNoiseFillBlock;
  if (blocks > 0x7fffffff) return fail(SCG_ERR_INVALID, "noise from words: %lld pairs", static_cast<long long>(n));
  hipLaunchKernelGGL(noise_from_words_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kNoiseFillBlock), 0,
                     static_cast<hipStream_t>(stream), words, out, n);
  return check_launch("noise_from_words_kernel");
}

int scg_sc_mlp_fused(const scg_sc_config* cfg, const scg_sc_state* st, int32_t hidden) {
  if (int rc = sc_host_check(cfg, st)) return -rc;
  if (hidden < 1 || hidden > SCG_SC_MLP_MAX_HIDDEN)
    return -fail(SCG_ERR_INVALID, "mlp: hidden in 1..%d, got %d", SCG_SC_MLP_MAX_HIDDEN, hidden);
  return sc_closed_fused(cfg, st) && sc_mlp_fits(cfg, hidden) ? 1 : 0;
}

}  // extern "C"
