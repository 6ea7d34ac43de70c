// The sampled SupplyChain policies (csrc/scg_sc_policy.h sc_policy_sample, sc_policy_action_sampled;
// csrc/scg_sc_mlp.h sc_mlp_action_sampled) on the host: u and the action of a table of cases,
// each with its parameters in env n of a per-env [Q][3] block or in a shared [Q] row and its
// noise at (k, n, a) of a [2][3][A] block read through sc_sample_index. One line per case with
// the bits of every input and result; tests/test_sc_sampled_host.py restates the formulas as
// NumPy float32 loops and compares. Includes nothing but the headers under test.
#include "scg_sc_mlp.h"
#include "scg_sc_policy.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace scg;

constexpr int kEnvs = 3, kSteps = 2;
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

static std::vector<float> draws(size_t n, float scale) {
  std::vector<float> v(n);
  for (float& x : v) x = draw(scale);
  return v;
}

static void print_row(const char* key, const std::vector<float>& v) {
  std::printf(" %s=", key);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%08x", i ? "," : "", bits(v[i]));
}

// A policy's words in formula order (scg_sc_policy.h / scg_sc_mlp.h): H == 0 is the linear one.
struct Case {
  int A, O, H;
  std::vector<float> p, o, std, eps;  // [Q], [O], [A], [A]
  float lo, hi;
};

static void run(const char* kind, const Case& c, bool shared) {
  const int A = c.A, O = c.O, H = c.H;
  const int n = g_case % kEnvs, k = (g_case / kEnvs) % kSteps;  // the noise's place; the parameters' env when per env
  ++g_case;
  const int N = shared ? 1 : kEnvs;
  const int Q = H ? sc_mlp_words(A, O, H) : sc_policy_words(A, O);
  std::vector<float> block(static_cast<size_t>(Q) * N);
  for (size_t i = 0; i < block.size(); ++i) block[i] = 1000.0f + static_cast<float>(i);  // other envs' words
  const int64_t qs = shared ? 1 : kEnvs, ns = shared ? 0 : 1;
  const int pn = shared ? 0 : n;
  for (int q = 0; q < Q; ++q) block[q * qs + pn * ns] = c.p[q];
  std::vector<float> noise(static_cast<size_t>(kSteps) * kEnvs * A, 77.0f);  // other steps' and envs' noise
  for (int a = 0; a < A; ++a) noise[sc_sample_index(kEnvs, A, k, n, a)] = c.eps[a];
  auto obs = [&](int j) { return c.o[j]; };
  std::vector<float> u(A), act(A);
  int bad = 0;
  for (int a = 0; a < A; ++a) {
    const float e = noise[sc_sample_index(kEnvs, A, k, n, a)];
    float u1, u2;
    if (H) {
      const ScMlpView mv = sc_mlp_view(block.data(), shared, kEnvs, H, c.lo, c.hi);
      std::vector<float> hid(H);
      for (int i = 0; i < H; ++i) hid[i] = sc_mlp_hidden<16>(mv, O, pn, i, obs);
      auto h = [&](int i) { return hid[i]; };
      act[a] = sc_mlp_action_sampled<16>(mv, O, pn, a, h, c.std[a], e, &u[a]);
      if (bits(sc_mlp_action_sampled<32>(mv, O, pn, a, h, c.std[a], e, &u1)) != bits(act[a]) ||
          bits(sc_mlp_action_sampled<1>(mv, O, pn, a, h, c.std[a], e, &u2)) != bits(act[a]) || bits(u1) != bits(u[a]) ||
          bits(u2) != bits(u[a]))
        ++bad;
      // std 0 and noise 0 are the deterministic action up to the sign of a zero
      float u0;
      const float det = sc_mlp_action<16>(mv, O, pn, a, h);
      const float s0 = sc_mlp_action_sampled<16>(mv, O, pn, a, h, 0.0f, 0.0f, &u0);
      if (!(det == s0) && !(det != det && s0 != s0)) ++bad;
    } else {
      const ScPolicyView pv = sc_policy_view(block.data(), shared, kEnvs, c.lo, c.hi);
      act[a] = sc_policy_action_sampled<16>(pv, O, pn, a, obs, c.std[a], e, &u[a]);
      if (bits(sc_policy_action_sampled<32>(pv, O, pn, a, obs, c.std[a], e, &u1)) != bits(act[a]) ||
          bits(sc_policy_action_sampled<1>(pv, O, pn, a, obs, c.std[a], e, &u2)) != bits(act[a]) || bits(u1) != bits(u[a]) ||
          bits(u2) != bits(u[a]))
        ++bad;
      float u0;
      const float det = sc_policy_action<16>(pv, O, pn, a, obs);
      const float s0 = sc_policy_action_sampled<16>(pv, O, pn, a, obs, 0.0f, 0.0f, &u0);
      if (!(det == s0) && !(det != det && s0 != s0)) ++bad;
    }
  }
  std::printf("%s A=%d O=%d H=%d shared=%d n=%d k=%d differ=%d lo=%08x hi=%08x", kind, A, O, H, shared ? 1 : 0, n, k, bad,
              bits(c.lo), bits(c.hi));
  print_row("o", c.o);
  print_row("p", c.p);
  print_row("s", c.std);
  print_row("e", c.eps);
  print_row("u", u);
  print_row("a", act);
  std::printf("\n");
}

static Case random_case(int A, int O, int H, float wscale, float std_scale) {
  Case c{A, O, H, {}, draws(O, 1.0f), std::vector<float>(A), draws(A, 3.0f), -1.0f, 1.0f};
  if (H) {
    for (int i = 0; i < H; ++i) {
      for (int j = 0; j < O; ++j) c.p.push_back(draw(0.3f));
      c.p.push_back(draw(0.5f));
    }
    for (int a = 0; a < A; ++a) {
      for (int i = 0; i < H; ++i) c.p.push_back(draw(wscale));
      c.p.push_back(draw(0.5f));
    }
  } else {
    for (int a = 0; a < A; ++a) {
      for (int j = 0; j < O; ++j) c.p.push_back(draw(wscale));
      c.p.push_back(draw(0.5f));
    }
  }
  for (float& s : c.std) s = (draw(0.5f) + 0.5f) * std_scale;  // [0, std_scale)
  return c;
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const int shapes[][3] = {{14, 27, 0}, {14, 27, 16}, {1, 1, 0}, {3, 5, 2}, {2, 40, 0}, {5, 40, 33}};
  for (const auto& s : shapes)
    for (int shared = 0; shared < 2; ++shared)
      for (int r = 0; r < 3; ++r) {
        run("random", random_case(s[0], s[1], s[2], 0.15f, 0.3f), shared);  // mostly inside
        run("clamp", random_case(s[0], s[1], s[2], 0.3f, 1.5f), shared);    // both clamps bind, by z or by the noise
      }
  for (int shared = 0; shared < 2; ++shared)
    for (int H = 0; H < 6; H += 5) {
      Case z = random_case(6, 4, H, 0.2f, 0.3f);  // std = 0: u is z (+0 for a -0 z)
      for (float& s : z.std) s = 0.0f;
      run("std0", z, shared);
      Case e = random_case(6, 4, H, 0.2f, 0.3f);  // lo == hi
      e.lo = e.hi = 0.375f;
      run("equal", e, shared);
      // noise +inf, -inf and NaN; std 0 under an infinite noise (0 * inf = NaN); a NaN std
      Case x = random_case(6, 4, H, 0.2f, 0.3f);
      x.eps = {inf, -inf, nan, inf, -inf, 0.5f};
      x.std = {0.25f, 0.25f, 0.25f, 0.0f, 0.0f, nan};
      run("special", x, shared);
      x.lo = -0.25f, x.hi = 0.125f;
      run("special", x, shared);
      // a noise that only just binds each clamp, and one that stays inside by one ulp of the bound
      Case b = random_case(4, 3, H, 0.0f, 0.0f);
      for (float& w : b.p) w = 0.0f;  // z = 0 for every action
      b.std = {1.0f, 1.0f, 1.0f, 1.0f};
      b.eps = {1.0f, 1.0000001f, -1.0f, -1.0000001f};
      run("edge", b, shared);
    }
  std::printf("index at=%lld,%lld,%lld\n", static_cast<long long>(sc_sample_index(130, 14, 0, 0, 0)),
              static_cast<long long>(sc_sample_index(130, 14, 2, 129, 13)),
              static_cast<long long>(sc_sample_index(65536, 14, 4095, 65535, 13)));
  return 0;
}
