// The SupplyChain one-hidden-layer ReLU policy (csrc/scg_sc_mlp.h) on the host: action rows of a
// table of cases, each with its parameters in env n of a per-env [Q][3] block or in a shared
// [Q] row, read through sc_mlp_view's strides. One line per case with the bits of every input
// and result; tests/test_sc_mlp_host.py restates the formula as a NumPy float32 loop and
// compares. Includes nothing but the header under test.
#include "scg_sc_mlp.h"

#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace scg;

constexpr int kEnvs = 3;
static int g_case = 0;
static uint32_t g_rng = 0x2545f491u;

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

struct Mlp {
  int A, O, H;
  std::vector<float> w1, b1, w2, b2;  // [H][O], [H], [A][H], [A]
};

// One case: the parameters placed by the layout's index function, then read back by
// sc_mlp_hidden / sc_mlp_action, with three chunk sizes that must agree.
static void run(const char* kind, const Mlp& m, bool shared, const std::vector<float>& o, float lo, float hi) {
  const int A = m.A, O = m.O, H = m.H;
  const int n = shared ? 0 : g_case % kEnvs;
  ++g_case;
  const int N = shared ? 1 : kEnvs;
  const int Q = sc_mlp_words(A, O, H);
  std::vector<float> block(static_cast<size_t>(Q) * N);
  for (size_t i = 0; i < block.size(); ++i) block[i] = 1000.0f + static_cast<float>(i);  // other envs' words
  const ScMlpView mv = sc_mlp_view(block.data(), shared, kEnvs, H, lo, hi);
  for (int i = 0; i < H; ++i) {
    for (int j = 0; j < O; ++j) block[sc_mlp_param_index(mv, O, n, 0, i, j)] = m.w1[i * O + j];
    block[sc_mlp_param_index(mv, O, n, 0, i, O)] = m.b1[i];
  }
  for (int a = 0; a < A; ++a) {
    for (int i = 0; i < H; ++i) block[sc_mlp_param_index(mv, O, n, 1, a, i)] = m.w2[a * H + i];
    block[sc_mlp_param_index(mv, O, n, 1, a, H)] = m.b2[a];
  }
  auto obs = [&](int j) { return o[j]; };
  std::vector<float> hid(H), act(A), p(Q);
  int bad = 0;
  for (int i = 0; i < H; ++i) {
    hid[i] = sc_mlp_hidden<16>(mv, O, n, i, obs);
    if (bits(sc_mlp_hidden<32>(mv, O, n, i, obs)) != bits(hid[i]) || bits(sc_mlp_hidden<1>(mv, O, n, i, obs)) != bits(hid[i]))
      ++bad;
  }
  auto h = [&](int i) { return hid[i]; };
  for (int a = 0; a < A; ++a) {
    act[a] = sc_mlp_action<16>(mv, O, n, a, h);
    if (bits(sc_mlp_action<32>(mv, O, n, a, h)) != bits(act[a]) || bits(sc_mlp_action<1>(mv, O, n, a, h)) != bits(act[a])) ++bad;
  }
  for (int q = 0; q < Q; ++q) p[q] = block[static_cast<int64_t>(q) * mv.qstride + n * mv.nstride];
  std::printf("%s A=%d O=%d H=%d shared=%d n=%d chunks_differ=%d lo=%08x hi=%08x", kind, A, O, H, shared ? 1 : 0, n, bad,
              bits(lo), bits(hi));
  print_row("o", o);
  print_row("p", p);
  print_row("h", hid);
  print_row("a", act);
  std::printf("\n");
}

static Mlp random_mlp(int A, int O, int H, float w1s, float w2s) {
  Mlp m{A, O, H, std::vector<float>(static_cast<size_t>(H) * O), std::vector<float>(H),
        std::vector<float>(static_cast<size_t>(A) * H), std::vector<float>(A)};
  for (float& x : m.w1) x = draw(w1s);
  for (float& x : m.b1) x = draw(0.5f);
  for (float& x : m.w2) x = draw(w2s);
  for (float& x : m.b2) x = draw(0.5f);
  return m;
}

static std::vector<float> random_obs(int O) {
  std::vector<float> o(O);
  for (float& x : o) x = draw(1.0f);
  return o;
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const int shapes[][3] = {{14, 27, 16}, {1, 1, 1}, {3, 5, 2}, {2, 40, 33}, {14, 27, 64}};
  for (const auto& s : shapes)
    for (int shared = 0; shared < 2; ++shared)
      for (int r = 0; r < 3; ++r) {
        run("random", random_mlp(s[0], s[1], s[2], 0.3f, 0.2f), shared, random_obs(s[1]), -1.0f, 1.0f);  // mostly inside
        run("clamp", random_mlp(s[0], s[1], s[2], 0.5f, 2.0f), shared, random_obs(s[1]), -1.0f, 1.0f);   // both clamps bind
      }
  for (int shared = 0; shared < 2; ++shared) {
    run("equal", random_mlp(4, 6, 5, 1.0f, 1.0f), shared, random_obs(6), 0.375f, 0.375f);  // lo == hi
    run("narrow", random_mlp(4, 6, 5, 1.0f, 1.0f), shared, random_obs(6), -0.125f, 0.0625f);
    // a hidden layer wholly negative: every unit +0, the action clamp(b2)
    Mlp neg = random_mlp(5, 4, 7, 1.0f, 1.0f);
    for (float& x : neg.w1) x = 0.0f;
    for (float& x : neg.b1) x = -0.5f - (&x - neg.b1.data());
    neg.b2 = {-3.0f, -0.25f, 0.0f, 0.75f, 2.0f};
    run("negative", neg, shared, random_obs(4), -1.0f, 1.0f);
    // pre-activations NaN (a NaN bias; inf * 0; inf - inf), -0 and -inf: every such unit is +0
    const std::vector<float> o = {0.0f, 1.0f, -1.0f};
    Mlp z0{2, 3, 6, std::vector<float>(6 * 3, 0.0f), {nan, 0.25f, 0.0f, -0.0f, -inf, 0.5f},
           std::vector<float>(2 * 6, 0.0f), {0.125f, 0.125f}};
    z0.w1[1 * 3 + 0] = inf;                          // unit 1: inf * 0 = NaN
    z0.w1[2 * 3 + 1] = inf, z0.w1[2 * 3 + 2] = inf;  // unit 2: inf - inf = NaN
    z0.w1[3 * 3 + 0] = -0.0f, z0.w1[3 * 3 + 1] = -0.0f;  // unit 3: every term -0, the sum -0
    z0.w1[5 * 3 + 1] = 0.25f;                        // unit 5: 0.75
    for (int i = 0; i < 5; ++i) z0.w2[0 * 6 + i] = 1.0f;  // action 0: the +0 units, z = b2
    z0.w2[1 * 6 + 5] = 0.5f;                              // action 1: 0.125 + 0.375
    run("zeros", z0, shared, o, -1.0f, 1.0f);
    run("zeros", z0, shared, o, -0.25f, 0.25f);
    // +inf hidden units (a bias; an overflowing product): z = inf, -inf, inf - inf = NaN, 0 * inf = NaN
    Mlp in{5, 3, 3, std::vector<float>(3 * 3, 0.0f), {inf, 3.0e38f, 0.5f}, std::vector<float>(5 * 3, 0.0f),
           {0.125f, 0.125f, 0.125f, 0.125f, nan}};
    in.w1[1 * 3 + 1] = 3.0e38f;
    in.w2[0 * 3 + 0] = 1.0f, in.w2[0 * 3 + 1] = 1.0f;
    in.w2[1 * 3 + 0] = -1.0f, in.w2[1 * 3 + 1] = -1.0f;
    in.w2[2 * 3 + 0] = 1.0f, in.w2[2 * 3 + 1] = -1.0f;
    in.w2[4 * 3 + 0] = 1.0f, in.w2[4 * 3 + 1] = 1.0f;  // (action 3: every weight 0; action 4: a NaN bias)
    run("infs", in, shared, o, -1.0f, 1.0f);
    run("infs", in, shared, o, -0.25f, 0.25f);
  }
  // the word of every (layer, row, column) and where each layout keeps it, for every env
  for (int shared = 0; shared < 2; ++shared) {
    const int A = 3, O = 4, H = 2;
    const ScMlpView mv = sc_mlp_view(nullptr, shared, kEnvs, H, 0.0f, 0.0f);
    for (int n = 0; n < kEnvs; ++n)
      for (int layer = 0; layer < 2; ++layer)
        for (int r = 0; r < (layer ? A : H); ++r)
          for (int k = 0; k <= (layer ? H : O); ++k)
            std::printf("index A=%d O=%d H=%d shared=%d N=%d n=%d layer=%d r=%d k=%d word=%d at=%lld\n", A, O, H, shared, kEnvs,
                        n, layer, r, k, sc_mlp_word(O, H, layer, r, k),
                        static_cast<long long>(sc_mlp_param_index(mv, O, n, layer, r, k)));
  }
  const bool ok = sc_mlp_valid(1, SCG_SC_ACT_RELU, 0, -1.0f, 1.0f) && sc_mlp_valid(64, SCG_SC_ACT_RELU, 0, 0.5f, 0.5f) &&
                  !sc_mlp_valid(0, SCG_SC_ACT_RELU, 0, -1.0f, 1.0f) && !sc_mlp_valid(65, SCG_SC_ACT_RELU, 0, -1.0f, 1.0f) &&
                  !sc_mlp_valid(-1, SCG_SC_ACT_RELU, 0, -1.0f, 1.0f) && !sc_mlp_valid(16, 0, 0, -1.0f, 1.0f) &&
                  !sc_mlp_valid(16, 2, 0, -1.0f, 1.0f) && !sc_mlp_valid(16, SCG_SC_ACT_RELU, 1, -1.0f, 1.0f) &&
                  !sc_mlp_valid(16, SCG_SC_ACT_RELU, 0, 1.0f, -1.0f) && !sc_mlp_valid(16, SCG_SC_ACT_RELU, 0, nan, 1.0f) &&
                  !sc_mlp_valid(16, SCG_SC_ACT_RELU, 0, -1.0f, inf);
  std::printf("valid ok=%d words=%d fused_max=%d\n", ok ? 1 : 0, sc_mlp_words(14, 27, 16), sc_mlp_fused_hidden_max(12, 8));
  return 0;
}
