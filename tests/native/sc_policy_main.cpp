// The SupplyChain linear policy (csrc/scg_sc_policy.h) on the host: action rows of a table of
// cases, each with its parameters in env n of a per-env [A*(O+1)][3] block or in a shared
// [A*(O+1)] row, read through sc_policy_view's strides. One line per case with the bits of
// every input and result; tests/test_sc_policy_host.py restates the formula as a NumPy float32
// loop and compares. Includes nothing but the header under test.
#include "scg_sc_policy.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace scg;

constexpr int kEnvs = 3;
static int g_case = 0;
static uint32_t g_rng = 0x9e3779b9u;

static uint32_t bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  return u;
}

// Uniform in [-scale, scale), on a 2^-16 grid.
static float draw(float scale) {
  g_rng = g_rng * 1664525u + 1013904223u;
  return (static_cast<float>(g_rng >> 15) / 65536.0f - 1.0f) * scale;
}

static void print_row(const char* key, const std::vector<float>& v) {
  std::printf(" %s=", key);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%08x", i ? "," : "", bits(v[i]));
}

// One case: weights w [A][O], bias b [A] and observation o [O] placed by the layout's index
// function, then read back by sc_policy_action, with two chunk sizes that must agree.
static int run(const char* kind, int A, int O, bool shared, const std::vector<float>& w, const std::vector<float>& b,
               const std::vector<float>& o, float lo, float hi) {
  const int n = shared ? 0 : g_case % kEnvs;
  ++g_case;
  const int N = shared ? 1 : kEnvs;
  std::vector<float> block(static_cast<size_t>(sc_policy_words(A, O)) * N);
  for (size_t i = 0; i < block.size(); ++i) block[i] = 1000.0f + static_cast<float>(i);  // other envs' words
  const ScPolicyView pv = sc_policy_view(block.data(), shared, kEnvs, lo, hi);
  for (int a = 0; a < A; ++a) {
    for (int j = 0; j < O; ++j) block[sc_policy_param_index(pv, O, n, a, j)] = w[a * O + j];
    block[sc_policy_param_index(pv, O, n, a, O)] = b[a];
  }
  auto obs = [&](int j) { return o[j]; };
  std::vector<float> act(A), p(sc_policy_words(A, O));
  int bad = 0;
  for (int a = 0; a < A; ++a) {
    act[a] = sc_policy_action<16>(pv, O, n, a, obs);
    const float again = sc_policy_action<32>(pv, O, n, a, obs);
    const float once = sc_policy_action<1>(pv, O, n, a, obs);
    if (bits(again) != bits(act[a]) || bits(once) != bits(act[a])) ++bad;
    for (int j = 0; j <= O; ++j) p[sc_policy_word(O, a, j)] = block[sc_policy_param_index(pv, O, n, a, j)];
  }
  std::printf("%s A=%d O=%d shared=%d n=%d chunks_differ=%d lo=%08x hi=%08x", kind, A, O, shared ? 1 : 0, n, bad, bits(lo),
              bits(hi));
  print_row("o", o);
  print_row("p", p);
  print_row("a", act);
  std::printf("\n");
  return bad;
}

static void random_case(const char* kind, int A, int O, bool shared, float wscale, float lo, float hi) {
  std::vector<float> w(static_cast<size_t>(A) * O), b(A), o(O);
  for (float& x : w) x = draw(wscale);
  for (float& x : b) x = draw(0.5f);
  for (float& x : o) x = draw(1.0f);
  run(kind, A, O, shared, w, b, o, lo, hi);
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const int shapes[][2] = {{14, 27}, {3, 5}, {1, 1}, {1, 7}, {5, 1}, {2, 40}, {14, 111}};
  for (const auto& s : shapes)
    for (int shared = 0; shared < 2; ++shared)
      for (int r = 0; r < 3; ++r) {
        random_case("random", s[0], s[1], shared, 0.25f, -1.0f, 1.0f);  // mostly inside the bounds
        random_case("clamp", s[0], s[1], shared, 3.0f, -1.0f, 1.0f);    // both clamps bind
      }
  for (int shared = 0; shared < 2; ++shared) {
    random_case("equal", 4, 6, shared, 1.0f, 0.375f, 0.375f);  // lo == hi
    random_case("narrow", 4, 6, shared, 1.0f, -0.125f, 0.0625f);
    // z = NaN (a NaN bias; inf * 0; inf - inf), +inf and -inf (a bias; an overflowing product)
    const std::vector<float> o = {0.0f, 1.0f, -1.0f};
    const std::vector<float> w = {0.0f, 0.0f, 0.0f,   inf, 0.0f, 0.0f,   0.0f, inf, inf,    0.0f,    0.0f, 0.0f,
                                  0.0f, 0.0f, 0.0f,   0.0f, 3.0e38f, 0.0f,   0.0f, 3.0e38f, 0.0f,   0.0f, 0.0f, 3.0e38f};
    const std::vector<float> b = {nan, 0.25f, 0.0f, inf, -inf, 3.0e38f, 0.5f, -3.0e38f};
    run("special", 8, 3, shared, w, b, o, -1.0f, 1.0f);
    run("special", 8, 3, shared, w, b, o, -0.5f, 0.5f);
  }
  // the word of every (a, j) and where each layout keeps it, for every env
  for (int shared = 0; shared < 2; ++shared) {
    const int A = 3, O = 4;
    const ScPolicyView pv = sc_policy_view(nullptr, shared, kEnvs, 0.0f, 0.0f);
    for (int n = 0; n < kEnvs; ++n)
      for (int a = 0; a < A; ++a)
        for (int j = 0; j <= O; ++j)
          std::printf("index A=%d O=%d shared=%d N=%d n=%d a=%d j=%d word=%d at=%lld\n", A, O, shared, kEnvs, n, a, j,
                      sc_policy_word(O, a, j), static_cast<long long>(sc_policy_param_index(pv, O, n, a, j)));
  }
  const bool ok = sc_policy_valid(SCG_SC_POLICY_LINEAR, -1.0f, 1.0f) && sc_policy_valid(SCG_SC_POLICY_LINEAR, 0.5f, 0.5f) &&
                  !sc_policy_valid(SCG_SC_POLICY_LINEAR, 1.0f, -1.0f) && !sc_policy_valid(SCG_SC_POLICY_LINEAR, nan, 1.0f) &&
                  !sc_policy_valid(SCG_SC_POLICY_LINEAR, -1.0f, nan) && !sc_policy_valid(SCG_SC_POLICY_LINEAR, -inf, 1.0f) &&
                  !sc_policy_valid(SCG_SC_POLICY_LINEAR, -1.0f, inf) && !sc_policy_valid(0, -1.0f, 1.0f) &&
                  !sc_policy_valid(2, -1.0f, 1.0f);
  std::printf("valid ok=%d words=%d\n", ok ? 1 : 0, sc_policy_words(14, 27));
  return 0;
}
