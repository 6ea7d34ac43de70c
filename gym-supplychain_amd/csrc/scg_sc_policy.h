// The SupplyChain linear policy, host and device (no HIP runtime header: a host program can
// include this alone). It is the one place that knows the formula and the two layouts of the
// parameters scg_sc_rollout_policy takes (include/scgpu.h, scg_sc_policy):
//
//   z_a = b_a;  for j = 0 .. O-1 ascending:  z_a = z_a + W[a][j] * o_j
//   act_a = !(z_a >= lo) ? lo : (z_a > hi ? hi : z_a)
//
// for the observation o[0..O) the env last produced, as float32 (a float64 observation
// element is rounded to float32 first: what a float32-observation env stores). Every multiply
// and every add is rounded to float32 on its own (the units that include this are built with
// -ffp-contract=off), in IEEE arithmetic, as NumPy computes the same loop; a NaN z gives lo.
//
// Word a*(O+1)+j of a policy is W[a][j] for j < O and b[a] for j == O. Per env the parameters
// are float32 [A*(O+1)][N], env fastest, so a wave reads each word of its 64 envs as one
// 256-byte row; shared they are float32 [A*(O+1)], one policy for every env. The same code
// reads both through two strides: word q of env n is params[q * qstride + n * nstride], with
// (qstride, nstride) = (N, 1) per env and (1, 0) shared.
//
// Sampled actions (scg_sc_rollout_sampled, scg_sc_sampling), for this policy and for the MLP of
// scg_sc_mlp.h alike: with z_a as above, a standard deviation std_a and the caller's noise eps,
//
//   u_a   = z_a + (std_a * eps[k][n][a])      the product rounded to float32, then the sum
//   act_a = !(u_a >= lo) ? lo : (u_a > hi ? hi : u_a)
//
// k the step's index in the call; a NaN u (a NaN z, 0 * inf) gives lo. sc_policy_sample is the
// one definition of u. A drawn loop (scg_sc_rollout_drawn, scg_sc_noise_draw) is the sampled one
// with eps[k][n][a] not read but computed: element (row0 + k, env_offset + n, a) of the seed's
// noise (csrc/scg_normal.h).
#pragma once

#include <cstdint>

#include "scgpu.h"

#if defined(__HIPCC__)
#define SCG_SC_POLICY_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define SCG_SC_POLICY_HD inline
#endif

namespace scg {

// Parameter words of one policy, and the index of W[a][j] (j < O) or b[a] (j == O) among them.
constexpr int sc_policy_words(int A, int O) { return A * (O + 1); }
SCG_SC_POLICY_HD int sc_policy_word(int O, int a, int j) { return a * (O + 1) + j; }

// The parameters as the formula reads them: the two strides and the clamp.
struct ScPolicyView {
  static constexpr bool kMlp = false;
  const float* params;
  int64_t qstride, nstride;
  float lo, hi;
};

SCG_SC_POLICY_HD ScPolicyView sc_policy_view(const float* params, bool shared, int64_t N, float lo, float hi) {
  return shared ? ScPolicyView{params, 1, 0, lo, hi} : ScPolicyView{params, N, 1, lo, hi};
}

SCG_SC_POLICY_HD int64_t sc_policy_param_index(const ScPolicyView& pv, int O, int64_t n, int a, int j) {
  return static_cast<int64_t>(sc_policy_word(O, a, j)) * pv.qstride + n * pv.nstride;
}

// Finite bounds lo <= hi (x - x is 0 only for a finite x); with a known kind, a valid policy.
SCG_SC_POLICY_HD bool sc_policy_bounds_valid(float lo, float hi) { return lo - lo == 0.0f && hi - hi == 0.0f && lo <= hi; }
SCG_SC_POLICY_HD bool sc_policy_valid(int32_t kind, float lo, float hi) {
  return kind == SCG_SC_POLICY_LINEAR && sc_policy_bounds_valid(lo, hi);
}

SCG_SC_POLICY_HD float sc_policy_clamp(float z, float lo, float hi) { return !(z >= lo) ? lo : (z > hi ? hi : z); }

// One row of a layer: z = bias; z = z + w[j] * in(j) for j = 0 .. L-1 ascending, for the L weight
// words at row[j * qstride] and the bias word after them. The weight words and the inputs are
// requested kChunk at a time, all of a chunk before the first is used (one memory round per
// chunk instead of one dependent load per term), past the row's end the last element again,
// so the requests are straight-line code; the sum itself runs in the formula's order over the
// terms j < L alone. (The linear policy's action rows and both layers of scg_sc_mlp.h.)
template <int kChunk, class In>
SCG_SC_POLICY_HD float sc_policy_row_sum(const float* row, int64_t qstride, int L, const In& in) {
  float z = row[static_cast<int64_t>(L) * qstride];
  for (int j0 = 0; j0 < L; j0 += kChunk) {
    float wv[kChunk], ov[kChunk];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int u = 0; u < kChunk; ++u) {
      const int j = j0 + u < L ? j0 + u : L - 1;
      wv[u] = row[static_cast<int64_t>(j) * qstride];
      ov[u] = in(j);
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int u = 0; u < kChunk; ++u) {
      const float term = wv[u] * ov[u];
      z = j0 + u < L ? z + term : z;
    }
  }
  return z;
}

// The sample u of an action whose formula gave z before its clamp.
SCG_SC_POLICY_HD float sc_policy_sample(float z, float std, float eps) {
  const float d = std * eps;
  return z + d;
}

// The noise of one launch (or, on the host side, one call) of a sampled closed loop: std [A],
// the noise rows [K][N][A] from the launch's first step on and, when asked for, the rows the
// samples go to (which may be the noise rows themselves: an element is read, then written, by
// one thread).
struct ScSampleView {
  const float* std;
  const float* noise;
  float* samples;  // or null
};

// The noise of one launch (or one step's action kernel) of a drawn closed loop: std [A], the
// rows the samples go to when asked for, the Philox key of the seed, the global row index of the
// first step and the global id of env 0 (csrc/scg_normal.h: what element (row, env, a) is).
struct ScDrawView {
  const float* std;
  float* samples;  // or null
  uint32_t k0, k1;
  uint32_t row0, env0;
};

// Element (k, n, a) of the noise and sample rows.
SCG_SC_POLICY_HD int64_t sc_sample_index(int64_t N, int A, int64_t k, int64_t n, int a) { return (k * N + n) * A + a; }

// The value z_a of env n before its clamp, from the env's observation obs(j), j = 0 .. O-1.
template <int kChunk, class Obs>
SCG_SC_POLICY_HD float sc_policy_z(const ScPolicyView& pv, int O, int64_t n, int a, const Obs& obs) {
  const float* row = pv.params + sc_policy_param_index(pv, O, n, a, 0);
  return sc_policy_row_sum<kChunk>(row, pv.qstride, O, obs);
}

// The two finishes of a z, the linear policy's or the MLP's (scg_sc_mlp.h sc_mlp_z): the action
// is sc_policy_clamp(z, lo, hi), or sampled the clamp of u, which goes to *u_out.
SCG_SC_POLICY_HD float sc_policy_clamp_sampled(float z, float std, float eps, float lo, float hi, float* u_out) {
  const float u = sc_policy_sample(z, std, eps);
  *u_out = u;
  return sc_policy_clamp(u, lo, hi);
}

// Action a of env n in one call, deterministic and sampled (u to *u_out): sc_policy_z under its
// two finishes, for callers with nothing to do between the two.
template <int kChunk, class Obs>
SCG_SC_POLICY_HD float sc_policy_action(const ScPolicyView& pv, int O, int64_t n, int a, const Obs& obs) {
  return sc_policy_clamp(sc_policy_z<kChunk>(pv, O, n, a, obs), pv.lo, pv.hi);
}
template <int kChunk, class Obs>
SCG_SC_POLICY_HD float sc_policy_action_sampled(const ScPolicyView& pv, int O, int64_t n, int a, const Obs& obs, float std,
                                                float eps, float* u_out) {
  return sc_policy_clamp_sampled(sc_policy_z<kChunk>(pv, O, n, a, obs), std, eps, pv.lo, pv.hi, u_out);
}

// What a closed-loop launch takes beside the step's launch arguments (scg_sc_nodes.hip), for
// a policy read through View (ScPolicyView; scg_sc_mlp.h ScMlpView).
template <class View>
struct ScClosedLaunch {
  static constexpr bool kSampled = false;
  static constexpr bool kDrawn = false;
  static constexpr bool kMlp = View::kMlp;
  View pv;
  void* obs_io;         // [N][O], obs dtype: read at the launch's first step, written at its last
  float* act_work;      // [N][A]: the launch's last action rows
  float* actions_out;   // [K][N][A] of this launch, or null
  double* reward_sum;   // [N]
  int32_t sum_add;      // 0: the launch stores its rewards' sum; else it adds to what is there
};

// A sampled closed-loop launch: the same, and behind it the launch's noise.
template <class View>
struct ScSampledLaunch : ScClosedLaunch<View> {
  static constexpr bool kSampled = true;
  ScSampleView smp;
};
static_assert(sizeof(ScSampledLaunch<ScPolicyView>) == sizeof(ScClosedLaunch<ScPolicyView>) + sizeof(ScSampleView),
              "the kernel arguments: smp directly behind the common fields");

// A drawn closed-loop launch: a sampled one that computes its noise (kDrawn) instead of reading it.
template <class View>
struct ScDrawnLaunch : ScClosedLaunch<View> {
  static constexpr bool kSampled = true;
  static constexpr bool kDrawn = true;
  ScDrawView drw;
};

}  // namespace scg
