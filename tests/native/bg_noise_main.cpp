// The noise row a BeerGame lane computes for itself (csrc/scg_normal.h bg_noise_row<L>) on the
// host: for L = 1..8, three rows, four env ids and three seeds, the bits of the row's L elements.
// tests/test_bg_noise_host.py recomputes every word from tests/noise_ref.py. Includes nothing but
// the header under test.
#include "scg_normal.h"

#include <cstdio>
#include <cstring>

using namespace scg;

static uint32_t bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  return u;
}

template <int L>
static void print_rows() {
  for (uint64_t seed : {uint64_t(0), uint64_t(1), ~uint64_t(0)})
    for (uint32_t k : {0u, 1u, 0xffffffffu})
      for (uint32_t e : {0u, 63u, 64u, 0xffffffffu}) {
        float eps[L];
        bg_noise_row<L>(static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), k, e, eps);
        std::printf("row L=%d seed=%llu k=%u e=%u x=", L, static_cast<unsigned long long>(seed), k, e);
        for (int a = 0; a < L; ++a) std::printf("%s%08x", a ? "," : "", bits(eps[a]));
        std::printf("\n");
      }
}

int main() {
  print_rows<1>();
  print_rows<2>();
  print_rows<3>();
  print_rows<4>();
  print_rows<5>();
  print_rows<6>();
  print_rows<7>();
  print_rows<8>();
  return 0;
}
