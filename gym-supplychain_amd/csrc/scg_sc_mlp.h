// The SupplyChain one-hidden-layer ReLU policy, host and device (no HIP runtime header: a host
// program can include this alone). It is the one place that knows the formula and the two
// layouts of the parameters scg_sc_rollout_mlp takes (include/scgpu.h, scg_sc_mlp):
//
//   h_i = b1_i;  for j = 0 .. O-1 ascending:  h_i = h_i + W1[i][j] * o_j;   h_i = (h_i > 0) ? h_i : +0.0f
//   z_a = b2_a;  for i = 0 .. H-1 ascending:  z_a = z_a + W2[a][i] * h_i
//   act_a = !(z_a >= lo) ? lo : (z_a > hi ? hi : z_a)
//
// for the observation o[0..O) the env last produced, as float32 (a float64 element rounded to
// float32 first), and hidden width H. Every multiply and every add is rounded to float32 on
// its own (the units that include this are built with -ffp-contract=off), as NumPy computes
// the same loops; a NaN or -0 pre-activation gives +0, a NaN z gives lo (sc_policy_clamp).
// Sampled (scg_sc_rollout_sampled): act_a is the clamp of u_a = z_a + (std_a * eps), as
// scg_sc_policy.h states it for both policies.
// Each layer's row is the linear policy's row (scg_sc_policy.h sc_policy_row_sum: L weight
// words, then the bias) under another epilogue.
//
// A policy is Q = H*(O+1) + A*(H+1) words: word i*(O+1)+j is W1[i][j] for j < O and b1[i] for
// j == O; word H*(O+1) + a*(H+1) + i is W2[a][i] for i < H and b2[a] for i == H. Per env the
// parameters are float32 [Q][N], env fastest; shared they are float32 [Q]. Both are read
// through the linear policy's two strides: word q of env n is params[q * qstride + n * nstride],
// (qstride, nstride) = (N, 1) per env and (1, 0) shared.
#pragma once

#include "scg_sc_policy.h"

namespace scg {

constexpr int sc_mlp_words(int A, int O, int H) { return H * (O + 1) + A * (H + 1); }
// The word of (layer 0, unit i, input j <= O) or (layer 1, action a, unit i <= H).
SCG_SC_POLICY_HD int sc_mlp_word(int O, int H, int layer, int r, int k) {
  return layer == 0 ? r * (O + 1) + k : H * (O + 1) + r * (H + 1) + k;
}

// Hidden units the fused closed loop holds for a config: two float32 per float64 of the
// inbox values and node cost rows of its LDS block (scg_sc_nodes.hip, sc_nodes_tile).
constexpr int sc_mlp_fused_hidden_max(int inbox_size, int n_nodes) { return 2 * (inbox_size + n_nodes); }

struct ScMlpView {
  static constexpr bool kMlp = true;
  const float* params;
  int64_t qstride, nstride;
  float lo, hi;
  int32_t H;
};

SCG_SC_POLICY_HD ScMlpView sc_mlp_view(const float* params, bool shared, int64_t N, int32_t H, float lo, float hi) {
  return shared ? ScMlpView{params, 1, 0, lo, hi, H} : ScMlpView{params, N, 1, lo, hi, H};
}

SCG_SC_POLICY_HD int64_t sc_mlp_param_index(const ScMlpView& mv, int O, int64_t n, int layer, int r, int k) {
  return static_cast<int64_t>(sc_mlp_word(O, mv.H, layer, r, k)) * mv.qstride + n * mv.nstride;
}

SCG_SC_POLICY_HD bool sc_mlp_valid(int32_t hidden, int32_t activation, int32_t reserved, float lo, float hi) {
  return hidden >= 1 && hidden <= SCG_SC_MLP_MAX_HIDDEN && activation == SCG_SC_ACT_RELU && reserved == 0 &&
         sc_policy_bounds_valid(lo, hi);
}

SCG_SC_POLICY_HD float sc_mlp_relu(float h) { return h > 0.0f ? h : 0.0f; }

// Hidden unit i of env n from its observation obs(j), j = 0 .. O-1.
template <int kChunk, class Obs>
SCG_SC_POLICY_HD float sc_mlp_hidden(const ScMlpView& mv, int O, int64_t n, int i, const Obs& obs) {
  const float* row = mv.params + sc_mlp_param_index(mv, O, n, 0, i, 0);
  return sc_mlp_relu(sc_policy_row_sum<kChunk>(row, mv.qstride, O, obs));
}

// The value z_a of env n before its clamp (scg_sc_policy.h: sc_policy_clamp, sc_policy_clamp_sampled),
// from the env's hidden units hid(i), i = 0 .. H-1.
template <int kChunk, class Hid>
SCG_SC_POLICY_HD float sc_mlp_z(const ScMlpView& mv, int O, int64_t n, int a, const Hid& hid) {
  const float* row = mv.params + sc_mlp_param_index(mv, O, n, 1, a, 0);
  return sc_policy_row_sum<kChunk>(row, mv.qstride, mv.H, hid);
}

// Action a of env n in one call, deterministic and sampled (scg_sc_policy.h sc_policy_action):
// sc_mlp_z under the two finishes.
template <int kChunk, class Hid>
SCG_SC_POLICY_HD float sc_mlp_action(const ScMlpView& mv, int O, int64_t n, int a, const Hid& hid) {
  return sc_policy_clamp(sc_mlp_z<kChunk>(mv, O, n, a, hid), mv.lo, mv.hi);
}
template <int kChunk, class Hid>
SCG_SC_POLICY_HD float sc_mlp_action_sampled(const ScMlpView& mv, int O, int64_t n, int a, const Hid& hid, float std, float eps,
                                             float* u_out) {
  return sc_policy_clamp_sampled(sc_mlp_z<kChunk>(mv, O, n, a, hid), std, eps, mv.lo, mv.hi, u_out);
}

static_assert(sizeof(ScSampledLaunch<ScMlpView>) == sizeof(ScClosedLaunch<ScMlpView>) + sizeof(ScSampleView),
              "the kernel arguments: smp directly behind the common fields");

}  // namespace scg
