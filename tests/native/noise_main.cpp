// The project's float32 normal (csrc/scg_normal.h) on the host: the radius over all 2^24 m, cos
// and sin over all 2^24 v, each as a checksum (the sum over i of bits_i * (2 i + 1) mod 2^64, i
// the index in the sweep) and every 4,099th value; the edge words; and elements (k, e, a) of
// three seeds through Philox. tests/test_noise_host.py recomputes every line from
// tests/noise_ref.py and compares the bits. Includes nothing but the header under test.
#include "scg_normal.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace scg;

static uint32_t bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  return u;
}

struct Sweep {
  uint64_t sum = 0, i = 0;
  std::vector<uint32_t> every;
  void add(float x) {
    const uint32_t b = bits(x);
    sum += static_cast<uint64_t>(b) * (2 * i + 1);
    if (i % 4099 == 0) every.push_back(b);
    ++i;
  }
  void print(const char* name) const {
    std::printf("sweep name=%s n=%llu sum=%016llx every=", name, static_cast<unsigned long long>(i),
                static_cast<unsigned long long>(sum));
    for (size_t j = 0; j < every.size(); ++j) std::printf("%s%08x", j ? "," : "", every[j]);
    std::printf("\n");
  }
};

int main() {
  constexpr uint32_t kN = 1u << 24;
  Sweep r, c, s;
  for (uint32_t m = 1; m <= kN; ++m) r.add(normal_radius(m));
  for (uint32_t v = 0; v < kN; ++v) {
    const NormalPair p = normal_cos_sin(v);
    c.add(p.c);
    s.add(p.s);
  }
  r.print("radius");
  c.print("cos");
  s.print("sin");

  for (uint32_t m : {1u, 2u, 1u << 23, kN - 1, kN}) std::printf("edge_m m=%u r=%08x\n", m, bits(normal_radius(m)));
  for (uint32_t oct = 0; oct <= 8; ++oct)  // v at 0, every octant (and so quadrant) boundary, and +-1 around each
    for (int d = -1; d <= 1; ++d) {
      const uint32_t v = ((oct << 21) + static_cast<uint32_t>(d)) & (kN - 1);
      const NormalPair p = normal_cos_sin(v);
      std::printf("edge_v v=%u c=%08x s=%08x\n", v, bits(p.c), bits(p.s));
    }
  // the pairs through the whole transform: the radius' edges against the angle's
  for (uint32_t w1 : {0u, 0x100u, 0x7fffff00u, 0xfffffe00u, 0xffffffffu})
    for (uint32_t w2 : {0u, 0xffu, 0x1fffff00u, 0x20000000u, 0x40000100u, 0xbfffffffu, 0xffffffffu}) {
      const NormalPair p = normal_from_words(w1, w2);
      std::printf("words w1=%u w2=%u c=%08x s=%08x one=%08x,%08x\n", w1, w2, bits(p.c), bits(p.s),
                  bits(normal_from_words_one(w1, w2, false)), bits(normal_from_words_one(w1, w2, true)));
    }

  for (uint64_t seed : {uint64_t(0), uint64_t(1), ~uint64_t(0)})
    for (uint32_t k : {0u, 1u, 0xffffffffu})
      for (uint32_t e : {0u, 129u, 0xffffffffu})
        for (uint32_t a : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u, 13u, 27u})
          std::printf("elem seed=%llu k=%u e=%u a=%u x=%08x\n", static_cast<unsigned long long>(seed), k, e, a,
                      bits(sc_noise_element(static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), k, e, a)));
  return 0;
}
