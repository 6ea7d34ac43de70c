// Host check of poisson_count_padded (scg_beergame_kernels.h): the count over the 40 padded
// thresholds of the slab kernel's constants block, then the table's tail, against the plain
// loop #{k < len : thr[k] <= u}. Built and run by tests/test_bg_poisson_count.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "scg_beergame_kernels.h"

static int32_t plain_count(const std::vector<uint32_t>& thr, uint32_t u) {
  int32_t x = 0;
  for (uint32_t t : thr) x += t <= u ? 1 : 0;
  return x;
}

// the block's thresholds as bg_slab_consts_kernel writes them
static void pad(const std::vector<uint32_t>& thr, uint32_t (&fast)[scg::kFastThr]) {
  for (int q = 0; q < scg::kFastThr; ++q) fast[q] = q < static_cast<int>(thr.size()) ? thr[q] : 0xffffffffu;
}

static long check(const std::vector<uint32_t>& thr, const char* kind, long* bad) {
  uint32_t fast[scg::kFastThr];
  pad(thr, fast);
  std::vector<uint32_t> us = {0u, 1u, 0xfffffffeu, 0xffffffffu};
  for (uint32_t t : thr) {
    us.push_back(t - 1u);
    us.push_back(t);
    us.push_back(t + 1u);
  }
  const int32_t len = static_cast<int32_t>(thr.size());
  for (uint32_t u : us) {
    const int32_t want = plain_count(thr, u), got = scg::poisson_count_padded(fast, thr.data(), len, u);
    if (want != got) {
      if (++*bad <= 20) std::printf("MISMATCH %s len=%d u=%u want=%d got=%d\n", kind, len, u, want, got);
    }
  }
  return static_cast<long>(us.size());
}

int main() {
  const int lens[] = {1, 7, 8, 9, 39, 40, 41, 64};
  long n = 0, bad = 0;
  uint32_t s = 0x9E3779B9u;
  for (int len : lens) {
    // a CDF as scg_poisson_table gives it: increasing, the last entry saturated
    std::vector<uint32_t> cdf(len);
    for (int k = 0; k < len; ++k)
      cdf[k] = k + 1 == len ? 0xffffffffu : static_cast<uint32_t>((static_cast<uint64_t>(k + 1) << 32) / (len + 1));
    n += check(cdf, "cdf", &bad);
    // arbitrary words, none saturated, unsorted, with repeats and the extremes
    std::vector<uint32_t> any(len);
    for (int k = 0; k < len; ++k) {
      s = s * 1664525u + 1013904223u;
      any[k] = k % 5 == 4 ? any[k - 1] : (s == 0xffffffffu ? 7u : s);
    }
    any[0] = 0u;
    if (len > 1) any[len - 1] = 0xfffffffeu;
    n += check(any, "any", &bad);
    // every entry saturated: all count only at u == 0xffffffff, like the pads
    n += check(std::vector<uint32_t>(len, 0xffffffffu), "sat", &bad);
  }
  std::printf("checked %ld mismatches %ld\n", n, bad);
  return bad ? 1 : 0;
}
