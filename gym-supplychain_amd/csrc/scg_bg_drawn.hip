// The closed-loop BeerGame rollout kernels with the float32 MLP policy sampled from noise the
// lanes compute themselves (scg_normal.h bg_noise_row; bg_rollout_kernel with MlpDrawnArgs as its
// source), and the kernel that writes the same rows out as a tensor: a unit of its own, compiled
// beside the per-level units.
#include "scg_bg_closed_launch.h"

namespace scg {

// out[k][n][0 .. L) = elements (row0 + k, env0 + n, 0 .. L-1), one (row, env) per thread: the
// function, the blocks and the pairs of the rollout's lanes.
template <int L>
__global__ __launch_bounds__(kBlock) void bg_noise_fill_kernel(float* __restrict__ out, int64_t rows, int64_t N, uint32_t k0,
                                                               uint32_t k1, uint32_t row0, uint32_t env0) {
  const int64_t id = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (id >= rows * N) return;
  const int64_t k = id / N, n = id - k * N;
  float eps[L];
  bg_noise_row<L>(k0, k1, row0 + static_cast<uint32_t>(k), env0 + static_cast<uint32_t>(n), eps);
  int32_t bits[L];
#pragma unroll
  for (int l = 0; l < L; ++l) bits[l] = __float_as_int(eps[l]);
  store_row<L>(reinterpret_cast<int32_t*>(out) + id * L, bits);
}

int bg_launch_noise_fill(hipStream_t s, int L, int64_t N, int64_t rows, uint32_t k0, uint32_t k1, uint32_t row0,
                         uint32_t env0, float* out) {
  const int64_t blocks = (rows * N + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffff) return fail(SCG_ERR_INVALID, "noise fill: %lld blocks", static_cast<long long>(blocks));
  const dim3 grid(static_cast<unsigned>(blocks));
  switch (L) {
#define X(l)                                                                                                  \
  case l:                                                                                                     \
    hipLaunchKernelGGL(bg_noise_fill_kernel<l>, grid, dim3(kBlock), 0, s, out, rows, N, k0, k1, row0, env0); \
    break;
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#undef X
    default: return fail(SCG_ERR_INVALID, "noise fill: levels=%d outside 1..%d", L, SCG_BG_POLICY_MAX_LEVELS);
  }
  return check_launch("bg_noise_fill_kernel");
}

template int bg_launch_closed<MlpDrawnArgs>(int, int, dim3, hipStream_t, const BgArgs&, int32_t, const RolloutWeeks&,
                                            const MlpDrawnArgs&);

}  // namespace scg
