// The project's float32 standard normal, host and device (no HIP runtime header: a host program
// can include this alone). It is the one definition of the exploration noise a closed loop draws
// itself (include/scgpu.h scg_sc_noise_draw, scg_sc_noise_fill, scg_bg_noise_draw,
// scg_bg_noise_fill), restated in NumPy by tests/noise_ref.py. The stream serves both env
// families (a BeerGame action a is level a): a BeerGame and a SupplyChain env given the same seed
// draw the same numbers. Element (row k, env id e, action a) of a 64-bit seed:
//
//   blk      = philox4x32_10(ctr = (e, k, a >> 2, SCG_STREAM_SC_NOISE), key = (seed & 0xffffffff, seed >> 32))
//   (w1, w2) = (blk.x, blk.y) for pair (a >> 1) & 1 == 0, (blk.z, blk.w) for pair 1
//   m = (w1 >> 8) + 1      in [1, 2^24]:  u = m * 2^-24 in (0, 1]
//   v = w2 >> 8            in [0, 2^24):  theta = 2 pi v * 2^-24
//   eps = r cos(theta) for even a, r sin(theta) for odd a,  r = sqrt(-2 ln u)     (Box-Muller)
//
// r, cos and sin are computed with float32 adds, subtracts, multiplies, divides and square roots
// alone, each rounded on its own in IEEE arithmetic (the units that include this are built with
// -ffp-contract=off and correctly rounded device divide and sqrt; no value here is subnormal),
// and with integer work that is exact: no libm / OCML function and no fast intrinsic, so the
// host, the device and NumPy give the same bits.
//
//   ln u:  x = float(m) = 2^e f; f is folded into [sqrt 1/2, sqrt 2) on its mantissa bits;
//          s = (f - 1) / (f + 1);  ln f = 2s + 2s (s^2 P(s^2)),  P Horner over 1/9, 1/7, 1/5, 1/3;
//          ln u = (e - 24) LN2_HI + ((e - 24) LN2_LO + ln f)     (the first product is exact)
//   theta: the quadrant is the top 2 bits of v; the other 22 are reflected at 2^21 into
//          t * 2^21, t in [0, 1], the angle pi/4 t (t exact);
//          sin = t S_HI + t (S_LO + t^2 (S1 + t^2 (S2 + t^2 S3)))
//          cos = 1 + t^2 (C0 + t^2 (C1 + t^2 (C2 + t^2 C3)))
//          (interpolants at the Chebyshev nodes of t^2), swapped by the reflection and swapped or
//          negated by the quadrant.
//
// Against float64 over all 2^24 values of m and of v: |r - r64| <= 3.53e-7 and |sin - sin64|,
// |cos - cos64| <= 7.57e-8 (tests/test_noise_host.py holds the exact maxima), so
// |eps - eps64| <= 3.53e-7 + sqrt(48 ln 2) * 7.57e-8 = 7.9e-7. m = 2^24 gives r = -0.0.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SCG_NORMAL_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define SCG_NORMAL_HD inline
#endif

namespace scg {

struct NormalPair {
  float c, s;
};

// r = sqrt(-2 ln(m * 2^-24)), m in [1, 2^24].
SCG_NORMAL_HD float normal_radius(uint32_t m) {
  constexpr float kLn2Hi = 0x1.62e3p-1f, kLn2Lo = 0x1.2fefa2p-17f;
  constexpr float kP3 = 0x1.555556p-2f, kP5 = 0x1.99999ap-3f, kP7 = 0x1.24924ap-3f, kP9 = 0x1.c71c72p-4f;
  const uint32_t bits = __builtin_bit_cast(uint32_t, static_cast<float>(m));  // exact: m <= 2^24
  const uint32_t mant = bits & 0x7fffffu;
  const bool fold = mant > 0x3504f3u;  // f > sqrt 2: halve it
  const int32_t e = static_cast<int32_t>(bits >> 23) - (127 + 24) + (fold ? 1 : 0);
  const float f = __builtin_bit_cast(float, mant | (fold ? 0x3f000000u : 0x3f800000u));
  const float ef = static_cast<float>(e);
  const float s = (f - 1.0f) / (f + 1.0f);
  const float s2 = s * s;
  float p = kP9;
  p = p * s2 + kP7;
  p = p * s2 + kP5;
  p = p * s2 + kP3;
  const float two_s = s + s;
  const float lnf = two_s + two_s * (s2 * p);
  const float lnu = ef * kLn2Hi + (ef * kLn2Lo + lnf);
  return __builtin_sqrtf(-2.0f * lnu);
}

// (cos, sin) of 2 pi v * 2^-24, v in [0, 2^24).
SCG_NORMAL_HD NormalPair normal_cos_sin(uint32_t v) {
  constexpr float kSHi = 0x1.921fb6p-1f, kSLo = -0x1.a1114ap-26f;
  constexpr float kS1 = -0x1.4abbbap-4f, kS2 = 0x1.465ec4p-9f, kS3 = -0x1.2d9b4p-15f;
  constexpr float kC0 = -0x1.3bd3ccp-2f, kC1 = 0x1.03c1eap-6f, kC2 = -0x1.55cb98p-12f, kC3 = 0x1.db6492p-19f;
  const uint32_t quad = v >> 22;
  uint32_t rem = v & 0x3fffffu;
  const bool refl = rem > 0x200000u;
  rem = refl ? 0x400000u - rem : rem;
  const float t = static_cast<float>(rem) * 0x1p-21f;  // exact
  const float t2 = t * t;
  float ps = kS3;
  ps = ps * t2 + kS2;
  ps = ps * t2 + kS1;
  ps = ps * t2 + kSLo;
  const float sn = t * kSHi + t * ps;
  float pc = kC3;
  pc = pc * t2 + kC2;
  pc = pc * t2 + kC1;
  pc = pc * t2 + kC0;
  const float cs = 1.0f + t2 * pc;
  const float sa = refl ? cs : sn;  // of the angle within the quadrant
  const float ca = refl ? sn : cs;
  NormalPair r;
  r.c = quad == 0 ? ca : quad == 1 ? -sa : quad == 2 ? -ca : sa;
  r.s = quad == 0 ? sa : quad == 1 ? ca : quad == 2 ? -sa : -ca;
  return r;
}

// (r cos theta, r sin theta) of a pair of Philox words.
SCG_NORMAL_HD NormalPair normal_from_words(uint32_t w1, uint32_t w2) {
  const float r = normal_radius((w1 >> 8) + 1u);
  const NormalPair cs = normal_cos_sin(w2 >> 8);
  NormalPair out;
  out.c = r * cs.c;
  out.s = r * cs.s;
  return out;
}

// Member a & 1 of a pair's normals alone: the one product.
SCG_NORMAL_HD float normal_from_words_one(uint32_t w1, uint32_t w2, bool odd) {
  const float r = normal_radius((w1 >> 8) + 1u);
  const NormalPair cs = normal_cos_sin(w2 >> 8);
  return r * (odd ? cs.s : cs.c);
}

}  // namespace scg

// The elements, where Philox is at hand (csrc/scg_philox.h includes the HIP runtime header).
#if defined(__HIPCC__)
#include "scg_philox.h"
#include "scgpu.h"

namespace scg {

// The Philox block of actions 4g .. 4g + 3 of (row, env).
__host__ __device__ __forceinline__ U4 sc_noise_block(uint32_t k0, uint32_t k1, uint32_t row, uint32_t env, uint32_t g) {
  return philox4x32_10(U4{env, row, g, SCG_STREAM_SC_NOISE}, k0, k1);
}

// Element (row, env, a) of the noise of key (k0, k1) = (seed & 0xffffffff, seed >> 32).
__host__ __device__ __forceinline__ float sc_noise_element(uint32_t k0, uint32_t k1, uint32_t row, uint32_t env, uint32_t a) {
  const U4 b = sc_noise_block(k0, k1, row, env, a >> 2);
  const bool second = (a >> 1) & 1u;
  return normal_from_words_one(second ? b.z : b.x, second ? b.w : b.y, a & 1u);
}

// Elements (row, env, 0 .. L-1) at once, as a lane that owns all L actions of its env computes
// them: ceil(L/4) Philox blocks and ceil(L/2) whole pairs (one radius, one cos/sin each); the
// last level of an odd L takes its pair's cosine alone. Element a is sc_noise_element(.., a).
template <int L>
__host__ __device__ __forceinline__ void bg_noise_row(uint32_t k0, uint32_t k1, uint32_t row, uint32_t env, float (&eps)[L]) {
#pragma unroll
  for (int g = 0; g < (L + 3) / 4; ++g) {
    const U4 b = sc_noise_block(k0, k1, row, env, static_cast<uint32_t>(g));
    const uint32_t w[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int a = 4 * g + 2 * p;
      if (a + 1 < L) {
        const NormalPair n = normal_from_words(w[2 * p], w[2 * p + 1]);
        eps[a] = n.c;
        eps[a + 1] = n.s;
      } else if (a < L) {
        eps[a] = normal_from_words_one(w[2 * p], w[2 * p + 1], false);
      }
    }
  }
}

}  // namespace scg
#endif
