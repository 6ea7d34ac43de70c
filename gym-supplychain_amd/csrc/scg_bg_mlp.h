// The BeerGame one-hidden-layer ReLU policy in float32, host and device (no HIP runtime header: a
// host program can include this alone). It is the one place that knows the formula and the
// layout of the parameters scg_bg_rollout_mlp takes (include/scgpu.h, scg_bg_mlp).
//
// With f[l][j] the int32 features of scg_bg_local.h (l < L, j < 4: net, line, down, own) of the
// state the env stands in, x[l*4+j] = (float)f[l][j] (round to nearest even, exact below 2^24),
// I = 4L inputs and H hidden units:
//
//   z_a = b2_a                                   a < L
//   for i = 0 .. H-1 ascending:
//       h = b1_i;  for j = 0 .. I-1 ascending:  h = h + W1[i][j] * x_j
//       h = (h > 0) ? h : +0.0f
//       for a < L:  z_a = z_a + W2[a][i] * h
//   u_a   = z_a                                   deterministic
//   u_a   = z_a + (std_a * eps_a)                 sampled; the product is rounded first
//   act_a = !(u_a >= (float)lo) ? lo : (u_a >= (float)hi ? hi : (int32)rintf(u_a))
//
// Every multiply and every add is rounded to float32 on its own (the units that include this are
// built with -ffp-contract=off), as NumPy computes the same loops; rintf rounds ties to even; a
// NaN or -0 pre-activation gives +0, a NaN u gives lo. lo <= hi, both within [-2^24, 2^24], so
// (float)lo and (float)hi are exact. Hidden unit i is finished and folded into the L sums before
// unit i+1 starts: no hidden array, and H is a run-time loop bound.
//
// A policy is Q = H*(I+1) + L*(H+1) float32 words, one block shared by every env: word
// i*(I+1)+j is W1[i][j] for j < I and b1[i] for j == I; word H*(I+1) + a*(H+1) + i is W2[a][i]
// for i < H and b2[a] for i == H (the layout of scg_sc_mlp.h with O = I and A = L). The reads
// are indexed by nothing a lane owns, so on the device they go through the scalar cache when
// `Params` is a constant-address-space pointer.
#pragma once

#include <cstdint>

#include "scg_bg_local.h"
#include "scg_bg_policy.h"
#include "scgpu.h"

namespace scg {

constexpr int kBgMlpMaxHidden = SCG_BG_MLP_MAX_HIDDEN;
constexpr int32_t kBgMlpMaxBound = 1 << 24;  // |lo|, |hi| up to here: exact as float32

constexpr int bg_mlp_inputs(int L) { return L * kLocalFeatures; }
constexpr int bg_mlp_words(int L, int H) { return H * (bg_mlp_inputs(L) + 1) + L * (H + 1); }
static_assert(bg_mlp_words(4, 16) == 340, "L = 4, H = 16: 340 words");

// The word of (layer 0, unit i, input j <= I) or (layer 1, action a, unit i <= H).
SCG_POLICY_HD int bg_mlp_word(int L, int H, int layer, int r, int k) {
  const int I = bg_mlp_inputs(L);
  return layer == 0 ? r * (I + 1) + k : H * (I + 1) + r * (H + 1) + k;
}

SCG_POLICY_HD bool bg_mlp_valid(int32_t kind, int32_t hidden, int32_t lo, int32_t hi) {
  return kind == SCG_BG_POLICY_MLP && hidden >= 1 && hidden <= kBgMlpMaxHidden && lo >= -kBgMlpMaxBound &&
         hi <= kBgMlpMaxBound && lo <= hi;
}

SCG_POLICY_HD float bg_mlp_relu(float h) { return h > 0.0f ? h : 0.0f; }

// z[a] before the noise and the finish, from the features. `Params` is const float* or the
// device's constant-address-space pointer to the same words.
template <int L, class Params>
SCG_POLICY_HD void bg_mlp_z(Params params, int32_t H, const int32_t (&f)[L][kLocalFeatures], float (&z)[L]) {
  constexpr int I = L * kLocalFeatures;
  float x[I];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < I; ++q) x[q] = static_cast<float>(f[q / kLocalFeatures][q % kLocalFeatures]);
  const Params w2 = params + H * (I + 1);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int a = 0; a < L; ++a) z[a] = w2[a * (H + 1) + H];
  for (int32_t i = 0; i < H; ++i) {
    const Params row = params + i * (I + 1);
    float h = row[I];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < I; ++j) h = h + row[j] * x[j];
    h = bg_mlp_relu(h);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int a = 0; a < L; ++a) z[a] = z[a] + w2[a * (H + 1) + i] * h;
  }
}

// The sample: the product is rounded before the add.
SCG_POLICY_HD float bg_mlp_sample(float z, float std, float eps) {
  const float d = std * eps;
  return z + d;
}

// u to the action: the bounds win over the rounding, a NaN gives lo.
SCG_POLICY_HD int32_t bg_mlp_finish(float u, int32_t lo, int32_t hi) {
  return !(u >= static_cast<float>(lo)) ? lo : (u >= static_cast<float>(hi) ? hi : static_cast<int32_t>(__builtin_rintf(u)));
}

// The whole policy on one env's features: u[a] (z[a], or the sample when std and eps are given)
// and act[a].
template <int L, class Params>
SCG_POLICY_HD void bg_mlp_act(Params params, int32_t H, const int32_t (&f)[L][kLocalFeatures], const float* std,
                              const float* eps, int32_t lo, int32_t hi, float (&u)[L], int32_t (&act)[L]) {
  bg_mlp_z<L>(params, H, f, u);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int a = 0; a < L; ++a) {
    if (std && eps) u[a] = bg_mlp_sample(u[a], std[a], eps[a]);
    act[a] = bg_mlp_finish(u[a], lo, hi);
  }
}

}  // namespace scg
