// The BeerGame per-env linear policy, host and device (no HIP runtime header: a host program
// can include this alone). It is the one place that knows the formula and the layout of the
// parameters scg_bg_rollout_policy takes (include/scgpu.h, scg_bg_policy):
//
//   z_l = b_l + sum_j W[l][j] * o_j          int64, two's-complement wrap
//   a_l = min(max(z_l >> shift, act_lo), act_hi)    arithmetic shift (floor), then the clamp
//
// for the observation o[0..L) the env last produced. The parameters of N envs are int32
// [L*(L+1)][N], env fastest: word l*(L+1)+j of an env is W[l][j] for j < L and b[l] for j == L,
// so a wave reads each word of its 64 envs as one 256-byte row.
#pragma once

#include <cstdint>

#include "scgpu.h"

#if defined(__HIPCC__)
#define SCG_POLICY_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define SCG_POLICY_HD inline
#endif

namespace scg {

constexpr int kPolicyMaxShift = 30;

// Parameter words per env.
constexpr int policy_words(int L) { return L * (L + 1); }
static_assert(policy_words(SCG_BG_POLICY_MAX_LEVELS) == 72, "8 levels: 72 words per env");

// Word index of W[l][j] (j < L) or b[l] (j == L), and where env n of N keeps that word.
SCG_POLICY_HD int policy_word(int L, int l, int j) { return l * (L + 1) + j; }
SCG_POLICY_HD int64_t policy_param_index(int L, int64_t N, int64_t n, int l, int j) {
  return static_cast<int64_t>(policy_word(L, l, j)) * N + n;
}

// What a launch needs of a scg_bg_policy beside the parameters.
struct PolicyClamp {
  int32_t shift, lo, hi;
};

// The shift and the clamp every integer policy takes (scg_bg_local.h too).
SCG_POLICY_HD bool clamp_valid(int32_t shift, int32_t lo, int32_t hi) {
  return shift >= 0 && shift <= kPolicyMaxShift && lo <= hi;
}

SCG_POLICY_HD bool policy_valid(int32_t kind, int32_t shift, int32_t lo, int32_t hi) {
  return kind == SCG_BG_POLICY_LINEAR && clamp_valid(shift, lo, hi);
}

// Env n's W words out of a [W][N] block of per-env parameters.
template <int W>
SCG_POLICY_HD void param_load(const int32_t* params, int64_t N, int64_t n, int32_t (&p)[W]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < W; ++q) p[q] = params[static_cast<int64_t>(q) * N + n];
}

// Env n's L*(L+1) words out of the [L*(L+1)][N] block.
template <int L>
SCG_POLICY_HD void policy_load(const int32_t* params, int64_t N, int64_t n, int32_t (&p)[L * (L + 1)]) {
  param_load(params, N, n, p);
}

// One level's action from its row of words (L weights, then the bias). A product of two int32
// fits int64; the sum is formed in uint64, where wrapping is defined, and read back as int64.
template <int L>
SCG_POLICY_HD int32_t policy_level(const int32_t* row, const int32_t (&o)[L], const PolicyClamp& c) {
  uint64_t z = static_cast<uint64_t>(static_cast<int64_t>(row[L]));
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int j = 0; j < L; ++j) z += static_cast<uint64_t>(static_cast<int64_t>(row[j]) * static_cast<int64_t>(o[j]));
  const int64_t s = static_cast<int64_t>(z) >> c.shift;  // arithmetic: floor for negative z
  return static_cast<int32_t>(s < c.lo ? c.lo : (s > c.hi ? c.hi : s));
}

template <int L>
SCG_POLICY_HD void policy_act(const int32_t (&p)[L * (L + 1)], const int32_t (&o)[L], const PolicyClamp& c,
                              int32_t (&act)[L]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int l = 0; l < L; ++l) act[l] = policy_level<L>(p + l * (L + 1), o, c);
}

// The observation an env last produced, from its inventory and backlog rows: inventory -
// backlog (+ max_stock for BeerGameEnv2; 0 for BeerGameEnv), wrapped to int32 as the kernels
// store it.
template <int L>
SCG_POLICY_HD void policy_obs(const int32_t (&inv)[L], const int32_t (&bk)[L], int32_t max_stock, int32_t (&o)[L]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int l = 0; l < L; ++l)
    o[l] = static_cast<int32_t>(static_cast<uint32_t>(inv[l]) - static_cast<uint32_t>(bk[l]) +
                                static_cast<uint32_t>(max_stock));
}

}  // namespace scg
