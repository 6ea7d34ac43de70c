// The BeerGame linear policy (csrc/scg_bg_policy.h) on the host: a table of cases for L = 1, 4
// and 8, each with its parameters in env n of an [L*(L+1)][3] block, read back with
// policy_load and turned into actions with policy_act. One line per case, inputs and result;
// tests/test_bg_policy_host.py restates the formula in NumPy int64 and compares. Includes
// nothing but the header under test.
#include "scg_bg_policy.h"

#include <cstdio>
#include <vector>

using namespace scg;

constexpr int kEnvs = 3;
static int g_case = 0;

// Level l gets the pre-shift value z[l]: weights and observation follow a small pattern and
// the bias makes up the difference (it fits int32 for the targets used here).
template <int L>
static void run(const char* kind, const int32_t (&w)[L][L], const int32_t (&o)[L], const int32_t (&b)[L],
                const PolicyClamp& c) {
  const int n = g_case++ % kEnvs;
  std::vector<int32_t> block(static_cast<size_t>(policy_words(L)) * kEnvs);
  for (size_t i = 0; i < block.size(); ++i) block[i] = static_cast<int32_t>(0x5bd1e995u * (i + 1));  // other envs' words
  for (int l = 0; l < L; ++l) {
    for (int j = 0; j < L; ++j) block[policy_param_index(L, kEnvs, n, l, j)] = w[l][j];
    block[policy_param_index(L, kEnvs, n, l, L)] = b[l];
  }
  int32_t p[L * (L + 1)], act[L];
  policy_load<L>(block.data(), kEnvs, n, p);
  policy_act<L>(p, o, c, act);
  std::printf("%s L=%d n=%d shift=%d lo=%d hi=%d o=", kind, L, n, c.shift, c.lo, c.hi);
  for (int l = 0; l < L; ++l) std::printf("%s%d", l ? "," : "", o[l]);
  std::printf(" p=");
  for (int q = 0; q < L * (L + 1); ++q) std::printf("%s%d", q ? "," : "", p[q]);
  std::printf(" a=");
  for (int l = 0; l < L; ++l) std::printf("%s%d", l ? "," : "", act[l]);
  std::printf("\n");
}

template <int L>
static void targets(const char* kind, const int64_t (&z)[L], const PolicyClamp& c) {
  int32_t w[L][L], o[L], b[L];
  for (int j = 0; j < L; ++j) o[j] = (j % 2 ? -1 : 1) * (37 + 11 * j);
  for (int l = 0; l < L; ++l) {
    int64_t dot = 0;
    for (int j = 0; j < L; ++j) {
      w[l][j] = (l == j ? -64 : 3 * l - 5 * j + 1);
      dot += static_cast<int64_t>(w[l][j]) * o[j];
    }
    b[l] = static_cast<int32_t>(z[l] - dot);
  }
  run<L>(kind, w, o, b, c);
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
  // shift 0: the value itself, up to the int32 bounds and one past them
  const int64_t wide[4] = {static_cast<int64_t>(kMax), static_cast<int64_t>(kMax) + 1, static_cast<int64_t>(kMin),
                           static_cast<int64_t>(kMin) - 1};
  for (int t = 0; t < 4; ++t) {
    int32_t w[L][L], o[L], b[L];
    for (int l = 0; l < L; ++l) {  // z_l = 2 * 2^30 + b_l or -(2 * 2^30) + b_l
      const int64_t z = wide[(t + l) % 4];
      for (int j = 0; j < L; ++j) w[l][j] = 0;
      w[l][0] = z > 0 ? 2 : -2;
      b[l] = static_cast<int32_t>(z - (z > 0 ? 1 : -1) * (int64_t(1) << 31));
    }
    for (int j = 0; j < L; ++j) o[j] = 0;
    o[0] = 1 << 30;
    run<L>("shift0", w, o, b, PolicyClamp{0, kMin, kMax});
  }
  // shift 30 on products of 2^62 (INT32_MIN squared): from two of them on the int64 sum wraps
  for (int t = 0; t < 2; ++t) {
    int32_t w[L][L], o[L], b[L];
    for (int j = 0; j < L; ++j) o[j] = kMin;
    for (int l = 0; l < L; ++l) {
      for (int j = 0; j < L; ++j) w[l][j] = (j <= l) ? (t && j == l ? kMax : kMin) : 0;
      b[l] = t ? -12345 - l : (1 << 30) * (l % 2) + l;
    }
    run<L>("shift30", w, o, b, PolicyClamp{30, t ? -7 : kMin, t ? 6 : kMax});
  }
}

// policy_param_index for every (l, j) of every env at N = 3, beside what policy_load reads
// out of a block whose word i holds i.
template <int L>
static void index_cases() {
  std::vector<int32_t> block(static_cast<size_t>(policy_words(L)) * kEnvs);
  for (size_t i = 0; i < block.size(); ++i) block[i] = static_cast<int32_t>(i);
  for (int n = 0; n < kEnvs; ++n) {
    int32_t p[L * (L + 1)];
    policy_load<L>(block.data(), kEnvs, n, p);
    for (int l = 0; l < L; ++l)
      for (int j = 0; j <= L; ++j)
        std::printf("index L=%d n=%d l=%d j=%d word=%d at=%lld loaded=%d\n", L, n, l, j, policy_word(L, l, j),
                    static_cast<long long>(policy_param_index(L, kEnvs, n, l, j)), p[policy_word(L, l, j)]);
  }
}

int main() {
  level_cases<1>();
  level_cases<4>();
  level_cases<8>();
  index_cases<1>();
  index_cases<4>();
  index_cases<8>();
  std::printf("valid ok=%d\n", (policy_valid(SCG_BG_POLICY_LINEAR, 0, 0, 0) && policy_valid(SCG_BG_POLICY_LINEAR, 30, -1, 1) &&
                                !policy_valid(SCG_BG_POLICY_LINEAR, 31, 0, 1) && !policy_valid(SCG_BG_POLICY_LINEAR, -1, 0, 1) &&
                                !policy_valid(SCG_BG_POLICY_LINEAR, 0, 5, 4) && !policy_valid(0, 0, 0, 1) &&
                                !policy_valid(2, 0, 0, 1))
                                   ? 1
                                   : 0);
  return 0;
}
