// The BeerGame float32 MLP policy (csrc/scg_bg_mlp.h) on the host: a table of cases for L = 1, 4
// and 8, each one line with its inputs (features as integers, every float as its bit pattern)
// and its results u and act from bg_mlp_act; the word index of every parameter at H = 3; and the
// argument check. tests/test_bg_mlp_host.py restates all of it in NumPy float32 and compares
// bits. Includes nothing but the header under test; built with -ffp-contract=off.
#include "scg_bg_mlp.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace scg;

static uint32_t bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, sizeof u);
  return u;
}

static uint32_t g_rng = 0x9e3779b9u;
static uint32_t next_u32() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return g_rng;
}
// A float in [-scale, scale) with a full 24-bit significand.
static float next_float(float scale) { return (static_cast<int32_t>(next_u32() >> 7) - (1 << 24)) * (scale / (1 << 24)); }

template <int L>
struct Case {
  int32_t H = 1, lo = -10, hi = 10;
  int32_t f[L][kLocalFeatures];
  std::vector<float> p;
  bool sampled = false;
  float std[L], eps[L];
  explicit Case(int32_t hidden) : H(hidden), p(static_cast<size_t>(bg_mlp_words(L, hidden)), 0.0f) {
    for (int l = 0; l < L; ++l) {
      for (int j = 0; j < kLocalFeatures; ++j) f[l][j] = 3 + 5 * l + 2 * j;
      std[l] = eps[l] = 0.0f;
    }
  }
  float& w1(int i, int j) { return p[bg_mlp_word(L, H, 0, i, j)]; }
  float& b1(int i) { return p[bg_mlp_word(L, H, 0, i, L * kLocalFeatures)]; }
  float& w2(int a, int i) { return p[bg_mlp_word(L, H, 1, a, i)]; }
  float& b2(int a) { return p[bg_mlp_word(L, H, 1, a, H)]; }
};

template <int L>
static void run(const char* kind, const Case<L>& c) {
  float u[L];
  int32_t act[L];
  bg_mlp_act<L>(c.p.data(), c.H, c.f, c.sampled ? c.std : nullptr, c.sampled ? c.eps : nullptr, c.lo, c.hi, u, act);
  std::printf("%s L=%d H=%d lo=%d hi=%d sampled=%d f=", kind, L, c.H, c.lo, c.hi, c.sampled ? 1 : 0);
  for (int q = 0; q < L * kLocalFeatures; ++q) std::printf("%s%d", q ? "," : "", c.f[q / kLocalFeatures][q % kLocalFeatures]);
  std::printf(" p=");
  for (size_t q = 0; q < c.p.size(); ++q) std::printf("%s%08x", q ? "," : "", bits(c.p[q]));
  std::printf(" std=");
  for (int l = 0; l < L; ++l) std::printf("%s%08x", l ? "," : "", bits(c.std[l]));
  std::printf(" eps=");
  for (int l = 0; l < L; ++l) std::printf("%s%08x", l ? "," : "", bits(c.eps[l]));
  std::printf(" u=");
  for (int l = 0; l < L; ++l) std::printf("%s%08x", l ? "," : "", bits(u[l]));
  std::printf(" a=");
  for (int l = 0; l < L; ++l) std::printf("%s%d", l ? "," : "", act[l]);
  std::printf("\n");
}

// H = 1 with h = 1 exactly (W1 = 0, b1 = 1) and b2 = 0: z_a = W2[a][0] = target[a].
template <int L>
static Case<L> targets(const float (&t)[L], int32_t lo, int32_t hi) {
  Case<L> c(1);
  c.lo = lo;
  c.hi = hi;
  c.b1(0) = 1.0f;
  for (int a = 0; a < L; ++a) c.w2(a, 0) = t[a];
  return c;
}

template <int L>
static Case<L> random_case(int32_t H, float w1s, float w2s) {
  Case<L> c(H);
  c.lo = 0;
  c.hi = 30;
  for (int l = 0; l < L; ++l)
    for (int j = 0; j < kLocalFeatures; ++j) c.f[l][j] = static_cast<int32_t>(next_u32() % 161) - 20;
  for (int i = 0; i < H; ++i) {
    for (int j = 0; j < L * kLocalFeatures; ++j) c.w1(i, j) = next_float(w1s);
    c.b1(i) = next_float(1.0f);
  }
  for (int a = 0; a < L; ++a) {
    for (int i = 0; i < H; ++i) c.w2(a, i) = next_float(w2s);
    c.b2(a) = 8.0f + next_float(1.0f);
  }
  return c;
}

template <int L>
static void level_cases() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  // ties at k + 0.5 on both parities of k, either sign: every level sees all eight
  const float ties[8] = {0.5f, 1.5f, 2.5f, -0.5f, -1.5f, 3.5f, -2.5f, 6.5f};
  for (int t = 0; t < 8; ++t) {
    float z[L];
    for (int a = 0; a < L; ++a) z[a] = ties[(t + a) % 8];
    run<L>("tie", targets<L>(z, -10, 10));
  }
  // u on each bound and one ulp inside it, for a small clamp and for the widest one
  const int32_t clamps[2][2] = {{-5, 7}, {-kBgMlpMaxBound, kBgMlpMaxBound}};
  for (const auto& cl : clamps) {
    const float lo = static_cast<float>(cl[0]), hi = static_cast<float>(cl[1]);
    const float on[4] = {lo, __builtin_nextafterf(lo, inf), hi, __builtin_nextafterf(hi, -inf)};
    for (int t = 0; t < 4; ++t) {
      float z[L];
      for (int a = 0; a < L; ++a) z[a] = on[(t + a) % 4];
      run<L>("bound", targets<L>(z, cl[0], cl[1]));
    }
  }
  // +inf, -inf, NaN and a large finite value (through b2: W2 = 0)
  const float special[4] = {inf, -inf, nan, 3.0e38f};
  for (int t = 0; t < 4; ++t) {
    Case<L> c(1);
    c.b1(0) = 1.0f;
    for (int a = 0; a < L; ++a) c.b2(a) = special[(t + a) % 4];
    run<L>("special", c);
  }
  // a -0 pre-activation: b1 = -0 and W1 = -0 on positive inputs. The ReLU gives +0, so with
  // W2 = -1 and b2 = -0 the sum is -0 + (-1 * +0) = -0; a ReLU that kept -0 would give +0.
  {
    Case<L> c(1);
    c.b1(0) = -0.0f;
    for (int j = 0; j < L * kLocalFeatures; ++j) c.w1(0, j) = -0.0f;
    for (int a = 0; a < L; ++a) {
      c.w2(a, 0) = -1.0f;
      c.b2(a) = -0.0f;
    }
    run<L>("negzero", c);
  }
  // features above 2^24: the conversion rounds to nearest even. Hidden unit 0 picks one input,
  // W2 = 2^-8 keeps z inside the widest clamp.
  const int32_t big[4] = {(1 << 24) + 1, (1 << 24) + 3, INT32_MAX, INT32_MIN};
  for (int t = 0; t < 4; ++t) {
    Case<L> c(1);
    c.lo = -kBgMlpMaxBound;
    c.hi = kBgMlpMaxBound;
    const int q = (5 * t + 1) % (L * kLocalFeatures);
    c.f[q / kLocalFeatures][q % kLocalFeatures] = big[t];
    c.w1(0, q) = big[t] < 0 ? -1.0f : 1.0f;  // past the ReLU either way
    for (int a = 0; a < L; ++a) c.w2(a, 0) = (a % 2 ? -1.0f : 1.0f) / 256.0f;
    run<L>("big", c);
  }
  // the product of the sample is rounded before the add: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds
  // to 1 + 2^-11, so u = 0 exactly; a fused multiply-add would leave 2^-24
  {
    float z[L];
    for (int a = 0; a < L; ++a) z[a] = -(1.0f + 1.0f / 2048.0f);
    Case<L> c = targets<L>(z, -10, 10);
    c.sampled = true;
    for (int a = 0; a < L; ++a) c.std[a] = c.eps[a] = 1.0f + 1.0f / 4096.0f;
    run<L>("product", c);
  }
  // general parameters: H = 1, H = 64, H = 3 (every word of the layout carries its own value) and
  // H = 16 twice, deterministic and sampled
  run<L>("h1", random_case<L>(1, 1.0f / 16, 2.0f));
  run<L>("h64", random_case<L>(64, 1.0f / 16, 0.25f));
  run<L>("h3", random_case<L>(3, 1.0f / 16, 1.0f));
  run<L>("order", random_case<L>(16, 1.0f / 16, 2.0f));
  {
    Case<L> c = random_case<L>(16, 1.0f / 16, 0.5f);
    c.sampled = true;
    for (int a = 0; a < L; ++a) {
      c.std[a] = 2.0f + next_float(1.0f);
      c.eps[a] = next_float(2.0f);
    }
    run<L>("sampled", c);
  }
  // every word index at H = 3
  const int H = 3, I = L * kLocalFeatures;
  for (int i = 0; i < H; ++i)
    for (int j = 0; j <= I; ++j) std::printf("index L=%d H=%d layer=0 r=%d k=%d word=%d\n", L, H, i, j, bg_mlp_word(L, H, 0, i, j));
  for (int a = 0; a < L; ++a)
    for (int i = 0; i <= H; ++i) std::printf("index L=%d H=%d layer=1 r=%d k=%d word=%d\n", L, H, a, i, bg_mlp_word(L, H, 1, a, i));
  std::printf("words L=%d H=3 q=%d H=64 q64=%d\n", L, bg_mlp_words(L, 3), bg_mlp_words(L, 64));
}

int main() {
  level_cases<1>();
  level_cases<4>();
  level_cases<8>();
  const int32_t B = kBgMlpMaxBound, K = SCG_BG_POLICY_MLP;
  std::printf("valid ok=%d\n",
              (bg_mlp_valid(K, 1, 0, 0) && bg_mlp_valid(K, 64, -B, B) && !bg_mlp_valid(K, 0, 0, 1) && !bg_mlp_valid(K, 65, 0, 1) &&
               !bg_mlp_valid(K, 4, 5, 4) && !bg_mlp_valid(K, 4, -B - 1, 0) && !bg_mlp_valid(K, 4, 0, B + 1) &&
               !bg_mlp_valid(SCG_BG_POLICY_LOCAL, 4, 0, 1) && !bg_mlp_valid(SCG_BG_POLICY_LINEAR, 4, 0, 1) && !bg_mlp_valid(0, 4, 0, 1))
                  ? 1
                  : 0);
  return 0;
}
