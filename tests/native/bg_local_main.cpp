// The BeerGame local-information policy (csrc/scg_bg_local.h) on the host: a table of cases for
// L = 1, 4 and 8, each with its parameters in env n of a [5*L][3] block, read back with
// local_load, its features formed by local_features from per-level state inputs and turned into
// actions with local_act; the parameter-word index of every (l, j); and the live-row mask on a
// table of delay lists. One line per case, inputs and result; tests/test_bg_local_host.py
// restates all of it in Python and compares. Includes nothing but the header under test.
#include "scg_bg_local.h"

#include <cstdio>
#include <vector>

using namespace scg;

constexpr int kEnvs = 3;
static int g_case = 0;

template <int L>
struct Inputs {
  int32_t net[L], bk[L], op[L], transit[L], last_demand;
};

template <int L>
static void print_row(const char* name, const int32_t (&v)[L]) {
  std::printf(" %s=", name);
  for (int l = 0; l < L; ++l) std::printf("%s%d", l ? "," : "", v[l]);
}

// Level l's row of weights and its bias go into env n's words; the features come from `in`.
template <int L>
static void run(const char* kind, const int32_t (&w)[L][kLocalFeatures], const int32_t (&b)[L], const Inputs<L>& in,
                const PolicyClamp& c) {
  const int n = g_case++ % kEnvs;
  std::vector<int32_t> block(static_cast<size_t>(local_words(L)) * kEnvs);
  for (size_t i = 0; i < block.size(); ++i) block[i] = static_cast<int32_t>(0x5bd1e995u * (i + 1));  // other envs' words
  for (int l = 0; l < L; ++l) {
    for (int j = 0; j < kLocalFeatures; ++j) block[local_param_index(kEnvs, n, l, j)] = w[l][j];
    block[local_param_index(kEnvs, n, l, kLocalFeatures)] = b[l];
  }
  int32_t p[L * kLocalRow], f[L][kLocalFeatures], act[L];
  local_load<L>(block.data(), kEnvs, n, p);
  local_features<L>(in.net, in.bk, in.op, in.transit, in.last_demand, f);
  local_act<L>(p, f, c, act);
  std::printf("%s L=%d n=%d shift=%d lo=%d hi=%d d=%d", kind, L, n, c.shift, c.lo, c.hi, in.last_demand);
  print_row<L>("net", in.net);
  print_row<L>("bk", in.bk);
  print_row<L>("op", in.op);
  print_row<L>("tr", in.transit);
  std::printf(" f=");
  for (int q = 0; q < L * kLocalFeatures; ++q) std::printf("%s%d", q ? "," : "", f[q / kLocalFeatures][q % kLocalFeatures]);
  std::printf(" p=");
  for (int q = 0; q < L * kLocalRow; ++q) std::printf("%s%d", q ? "," : "", p[q]);
  print_row<L>("a", act);
  std::printf("\n");
}

// A small state: every term of `line` non-zero where the level has it.
template <int L>
static Inputs<L> small_inputs() {
  Inputs<L> in;
  for (int l = 0; l < L; ++l) {
    in.net[l] = (l % 2 ? -1 : 1) * (37 + 11 * l);
    in.bk[l] = 3 + 2 * l;
    in.op[l] = 4 + 5 * l;
    in.transit[l] = 8 + 3 * l;
  }
  in.last_demand = 6;
  return in;
}

// Level l gets the pre-shift value z[l]: the weights follow a small pattern and the bias makes
// up the difference (it fits int32 for the targets used here).
template <int L>
static void targets(const char* kind, const int64_t (&z)[L], const PolicyClamp& c) {
  const Inputs<L> in = small_inputs<L>();
  int32_t f[L][kLocalFeatures], w[L][kLocalFeatures], b[L];
  local_features<L>(in.net, in.bk, in.op, in.transit, in.last_demand, f);
  for (int l = 0; l < L; ++l) {
    int64_t dot = 0;
    for (int j = 0; j < kLocalFeatures; ++j) {
      w[l][j] = (j == 0 ? -64 : 3 * l - 5 * j + 1);
      dot += static_cast<int64_t>(w[l][j]) * f[l][j];
    }
    b[l] = static_cast<int32_t>(z[l] - dot);
  }
  run<L>(kind, w, b, in, c);
}

template <int L>
static void level_cases() {
  const int32_t kMin = INT32_MIN, kMax = INT32_MAX;
  // negative pre-shift values that are no multiple of 2^shift: floor, not truncation
  {
    int64_t z[L];
    for (int l = 0; l < L; ++l) z[l] = -1 - 10 * l;
    targets<L>("floor", z, PolicyClamp{3, kMin, kMax});
  }
  // each clamp bound exactly and one past it, after a shift of 2; every level sees all four
  const int32_t lo = -5, hi = 7;
  const int64_t on[4] = {(lo - 1) * 4 + 3, lo * 4, hi * 4 + 3, (hi + 1) * 4};  // >> 2: lo - 1, lo, hi, hi + 1
  for (int t = 0; t < 4; ++t) {
    int64_t z[L];
    for (int l = 0; l < L; ++l) z[l] = on[(t + l) % 4];
    targets<L>("clamp", z, PolicyClamp{2, lo, hi});
  }
  // shift 0: the value itself, up to the int32 bounds and one past them (2 * 2^30 on `own`)
  const int64_t wide[4] = {static_cast<int64_t>(kMax), static_cast<int64_t>(kMax) + 1, static_cast<int64_t>(kMin),
                           static_cast<int64_t>(kMin) - 1};
  for (int t = 0; t < 4; ++t) {
    Inputs<L> in{};
    int32_t w[L][kLocalFeatures], b[L];
    for (int l = 0; l < L; ++l) {
      const int64_t z = wide[(t + l) % 4];
      for (int j = 0; j < kLocalFeatures; ++j) w[l][j] = 0;
      w[l][LOCAL_OWN] = z > 0 ? 2 : -2;
      b[l] = static_cast<int32_t>(z - (z > 0 ? 1 : -1) * (int64_t(1) << 31));
      in.op[l] = 1 << 30;
    }
    run<L>("shift0", w, b, in, PolicyClamp{0, kMin, kMax});
  }
  // shift 30 on products of 2^62 (INT32_MIN squared): every feature is INT32_MIN, and from two
  // such products on the int64 sum wraps
  for (int t = 0; t < 2; ++t) {
    Inputs<L> in{};
    int32_t w[L][kLocalFeatures], b[L];
    for (int l = 0; l < L; ++l) {
      in.net[l] = in.op[l] = kMin;  // line = op + 0 + 0, down = op[l-1] or last_demand, own = op
      for (int j = 0; j < kLocalFeatures; ++j) w[l][j] = (j <= l % kLocalFeatures) ? (t && j == l % kLocalFeatures ? kMax : kMin) : 0;
      b[l] = t ? -12345 - l : (1 << 30) * (l % 2) + l;
    }
    in.last_demand = kMin;
    run<L>("shift30", w, b, in, PolicyClamp{30, t ? -7 : kMin, t ? 6 : kMax});
  }
  // the supply line itself wraps: INT32_MAX orders plus an upstream backlog and a transit row
  {
    Inputs<L> in = small_inputs<L>();
    int32_t w[L][kLocalFeatures], b[L];
    for (int l = 0; l < L; ++l) {
      in.op[l] = kMax - l;
      in.transit[l] = 2 + l;
      for (int j = 0; j < kLocalFeatures; ++j) w[l][j] = j == LOCAL_LINE ? 1 : 0;
      b[l] = 0;
    }
    run<L>("wrapline", w, b, in, PolicyClamp{0, kMin, kMax});
  }
}

// local_param_index for every (l, j) of every env at N = 3, beside what local_load reads out of
// a block whose word i holds i.
template <int L>
static void index_cases() {
  std::vector<int32_t> block(static_cast<size_t>(local_words(L)) * kEnvs);
  for (size_t i = 0; i < block.size(); ++i) block[i] = static_cast<int32_t>(i);
  for (int n = 0; n < kEnvs; ++n) {
    int32_t p[L * kLocalRow];
    local_load<L>(block.data(), kEnvs, n, p);
    for (int l = 0; l < L; ++l)
      for (int j = 0; j <= kLocalFeatures; ++j)
        std::printf("index L=%d n=%d l=%d j=%d word=%d at=%lld loaded=%d\n", L, n, l, j, local_word(l, j),
                    static_cast<long long>(local_param_index(kEnvs, n, l, j)), p[local_word(l, j)]);
  }
}

// The live mask of a delay list ([d_0] + one delay per week) after every week w0 = 0..T.
static void mask_cases(const char* name, const std::vector<int32_t>& delays) {
  const int32_t T = static_cast<int32_t>(delays.size()) - 1;
  for (int32_t w0 = 0; w0 <= T; ++w0) {
    std::printf("mask name=%s T=%d w0=%d delays=", name, T, w0);
    for (size_t i = 0; i < delays.size(); ++i) std::printf("%s%d", i ? "," : "", delays[i]);
    std::printf(" live=%llu\n", static_cast<unsigned long long>(local_live_mask(delays.data(), T, w0)));
  }
}

int main() {
  level_cases<1>();
  level_cases<4>();
  level_cases<8>();
  index_cases<1>();
  index_cases<4>();
  index_cases<8>();
  // delay 0, colliding arrival weeks (weeks 3 and 5 both ship into week 6) and arrivals past T
  mask_cases("list", {2, 2, 0, 3, 1, 1, 4, 2, 0, 5, 1, 2, 3});
  mask_cases("d0-past-T", {7, 1, 2, 1});
  mask_cases("all-zero", {0, 0, 0, 0, 0});
  {
    std::vector<int32_t> d(101, 1);  // T = 100: delays of exactly 64, one arriving at T, one a week past it
    d[0] = 64;
    d[3] = 64;
    d[36] = 64;
    d[37] = 64;
    d[50] = 0;
    mask_cases("delay-64", d);
  }
  for (int32_t R : {1, 2, 5, 65})
    for (int32_t T : {1, 12, 100})
      for (int32_t w0 : {0, 1, T / 2, T - 1, T})
        std::printf("smask R=%d T=%d w0=%d live=%llu\n", R, T, w0,
                    static_cast<unsigned long long>(local_live_mask_stochastic(R, T, w0)));
  std::printf("valid ok=%d\n", (local_valid(SCG_BG_POLICY_LOCAL, 0, 0, 0) && local_valid(SCG_BG_POLICY_LOCAL, 30, -1, 1) &&
                                !local_valid(SCG_BG_POLICY_LOCAL, 31, 0, 1) && !local_valid(SCG_BG_POLICY_LOCAL, -1, 0, 1) &&
                                !local_valid(SCG_BG_POLICY_LOCAL, 0, 5, 4) && !local_valid(0, 0, 0, 1) &&
                                !local_valid(SCG_BG_POLICY_LINEAR, 0, 0, 1) && !local_valid(3, 0, 0, 1))
                                   ? 1
                                   : 0);
  return 0;
}
