// The BeerGame local-information policy, host and device (no HIP runtime header: a host
// program can include this alone). It is the one place that knows the four features, the
// formula, the layout of the parameters scg_bg_rollout_local takes (include/scgpu.h,
// scg_bg_local_policy) and which rows of the shipment ring are live.
//
// Each level decides from four int32 about itself. For the state after week w of the current
// episode (w = 0: just reset), horizon T, level l of L, in the reference's attribute names:
//
//   f[l][0] net   inventory[l] - backlog[l] (+ max_stock for BeerGameEnv2): policy_obs, unchanged
//   f[l][1] line  orders_placed[l] + (backlog[l+1] if l+1 < L else 0) + sum_{v=w+1..T} shipments[v][l]:
//                 the order slip on its way up, what the supplier owes, and what is in transit
//                 and still arrives within the episode
//   f[l][2] down  the latest order from downstream: orders_placed[l-1] for l >= 1; for l = 0 the
//                 customer demand of week w (incoming_orders[0]), initial_orders_value at w = 0
//                 (also after an auto-reset inside a call)
//   f[l][3] own   orders_placed[l]
//
// Shipments scheduled past week T are not in `line`: the kernels drop them (MODE_DROP), so they
// are not in the state. Every feature is int32 in wrapping arithmetic, formed in uint32_t as
// policy_obs does; none touches the overflow flag.
//
//   z_l = b_l + sum_{j<4} W[l][j] * f[l][j]         int64, the sum formed in uint64 (wraps)
//   a_l = min(max(z_l >> shift, act_lo), act_hi)    arithmetic shift (floor), then the clamp
//
// which is policy_level<4> on level l's row of five words. The parameters of N envs are int32
// [5*L][N], env fastest: word l*5+j of an env is W[l][j] for j < 4 and b[l] for j == 4.
// Order-up-to S on the inventory position is W = (-1, -1, 0, 0), b = S (BeerGameEnv2:
// b = S + max_stock).
#pragma once

#include <cstdint>

#include "scg_bg_plan.h"
#include "scg_bg_policy.h"
#include "scgpu.h"

namespace scg {

constexpr int kLocalFeatures = 4;
constexpr int kLocalRow = kLocalFeatures + 1;  // a level's weights, then its bias
enum : int { LOCAL_NET = 0, LOCAL_LINE = 1, LOCAL_DOWN = 2, LOCAL_OWN = 3 };

// Parameter words per env.
constexpr int local_words(int L) { return L * kLocalRow; }
static_assert(local_words(4) == policy_words(4) && local_words(SCG_BG_POLICY_MAX_LEVELS) == 40, "20 and 40 words per env");

// Word index of W[l][j] (j < 4) or b[l] (j == 4), and where env n of N keeps that word.
SCG_POLICY_HD int local_word(int l, int j) { return l * kLocalRow + j; }
SCG_POLICY_HD int64_t local_param_index(int64_t N, int64_t n, int l, int j) {
  return static_cast<int64_t>(local_word(l, j)) * N + n;
}

SCG_POLICY_HD bool local_valid(int32_t kind, int32_t shift, int32_t lo, int32_t hi) {
  return kind == SCG_BG_POLICY_LOCAL && clamp_valid(shift, lo, hi);
}

// Env n's 5*L words out of the [5*L][N] block.
template <int L>
SCG_POLICY_HD void local_load(const int32_t* params, int64_t N, int64_t n, int32_t (&p)[L * kLocalRow]) {
  param_load(params, N, n, p);
}

SCG_POLICY_HD int32_t local_wrap_add(int32_t x, int32_t y) {
  return static_cast<int32_t>(static_cast<uint32_t>(x) + static_cast<uint32_t>(y));
}

// One level's features: its net stock (policy_obs), its own orders_placed, the backlog of the
// level above (0 at the top), its in-transit sum and the latest order from downstream.
SCG_POLICY_HD void local_level_features(int32_t net, int32_t own, int32_t up_backlog, int32_t transit, int32_t down,
                                        int32_t (&f)[kLocalFeatures]) {
  f[LOCAL_NET] = net;
  f[LOCAL_LINE] = local_wrap_add(local_wrap_add(own, up_backlog), transit);
  f[LOCAL_DOWN] = down;
  f[LOCAL_OWN] = own;
}

// Every level's features from the state rows: net is policy_obs of the inventory and backlog,
// transit[l] the sum of the live shipment rows of level l, last_demand the customer demand of
// the week the state stands after (initial_orders_value just after a reset).
template <int L>
SCG_POLICY_HD void local_features(const int32_t (&net)[L], const int32_t (&bk)[L], const int32_t (&op)[L],
                                  const int32_t (&transit)[L], int32_t last_demand, int32_t (&f)[L][kLocalFeatures]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int l = 0; l < L; ++l)
    local_level_features(net[l], op[l], l + 1 < L ? bk[l + 1] : 0, transit[l], l ? op[l - 1] : last_demand, f[l]);
}

template <int L>
SCG_POLICY_HD void local_act(const int32_t (&p)[L * kLocalRow], const int32_t (&f)[L][kLocalFeatures],
                             const PolicyClamp& c, int32_t (&act)[L]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int l = 0; l < L; ++l) act[l] = policy_level<kLocalFeatures>(p + l * kLocalRow, f[l], c);
}

// ---- which ring rows are live ------------------------------------------------------------
// With a delay list a consumed ring slot is not cleared (the next MODE_STORE overwrites it), so
// the in-transit sum runs over the weeks the episode has scheduled, not over the ring. For the
// state after week w0, bit j-1 (1 <= j <= 64) of the mask is set when week v = w0 + j <= T was
// scheduled by weeks <= w0 of this episode: v <= min(d_0, T) (the initial pipeline), or some
// week 1 <= w <= w0 has d_w > 0 and w + d_w = v. These are the weeks scg_bg_prepare marks in
// written[] by week w0. No delay exceeds kLocalMaxDelay, so no scheduled week lies past bit 63.
// The row of week v is ring slot v % R.
constexpr int kLocalMaxDelay = SCG_BG_LOCAL_MAX_DELAY;
static_assert(kLocalMaxDelay == 64, "the live mask is one 64-bit word");

SCG_PLAN_HD uint64_t local_live_mask(const int32_t* delays, int32_t T, int32_t w0) {
  uint64_t m = 0;
  const int32_t d0 = delays[0] < T ? delays[0] : T;
  for (int32_t j = 1; j <= kLocalMaxDelay && w0 + j <= d0; ++j) m |= uint64_t(1) << (j - 1);
  for (int32_t w = w0 - kLocalMaxDelay + 1 > 1 ? w0 - kLocalMaxDelay + 1 : 1; w <= w0; ++w) {
    const int32_t d = delays[w], j = w + d - w0;
    if (d > 0 && j >= 1 && j <= kLocalMaxDelay && w + d <= T) m |= uint64_t(1) << (j - 1);
  }
  return m;
}

// With stochastic delays every lane schedules its own weeks, but there a consumed slot is
// cleared and a reset zeroes the ring, so every slot but week w0's own holds what is in transit
// (or zero): every j <= min(R - 1, T - w0) is live.
SCG_PLAN_HD uint64_t local_live_mask_stochastic(int32_t R, int32_t T, int32_t w0) {
  int32_t k = R - 1 < T - w0 ? R - 1 : T - w0;
  k = k < 0 ? 0 : (k > kLocalMaxDelay ? kLocalMaxDelay : k);
  return k >= 64 ? ~uint64_t(0) : (uint64_t(1) << k) - 1;
}

}  // namespace scg
