// Node-parallel SupplyChain step kernel for gfx950 (scg_supplychain_nodes.h).
//
// A block is 64 envs x W waves. Wave w owns nodes w, w + W, ... of all 64 envs, lane l env
// blockIdx.x * 64 + l: every wave runs one node's code (no divergence between node kinds)
// and every state access is a 64-env row of the env-fastest layout (coalesced). The lane
// kernel walks an env's whole chain on one lane, a chain of dependent LDS and FP64
// latencies at one or two waves per SIMD; here the chain is cut into W waves that run at
// once, so the same work hides its latencies behind W times as many waves.
//
// LDS per block (doubles first): the block's heaps [NP][H][64], released sums [NP][64],
// shipment inbox [E][64], node costs [NN][64], the observation tile [64][O|1] (float or
// double); then the int32 heap times/kinds, heap sizes, inbox times/kinds, cost kinds, the
// per-wave "order not provable" flags [W][64] and the action tile [64][A|1].
//   stage  (wave w, its nodes)  heaps HBM -> LDS, released sums, flags; every thread
//                               loads a share of the block's action rows (one contiguous
//                               span) into the action tile                    | barrier
//   act    (wave w, its nodes)  stock, costs, shipments -> inbox, stock obs   | barrier
//   heaps  (wave w, its nodes)  inbox pushes, pops, supply push, bins, copy back
//   reward (wave 0)             -(costs in node order), return, demand / time obs
//                                                                             | barrier
//   out    (every thread)       the observation tile -> HBM, one contiguous span per block;
//                               wave 0 resets its envs at an auto-reset step
// The grid is persistent: as many blocks as the device holds at once (two per CU), each
// stepping tiles of 64 envs in turn, with the launch arguments re-read per tile through a
// pointer the compiler cannot carry across tiles (nothing derived from them is held, or
// spilled, across the loop).
// An env any wave flagged skips act and heaps; wave 0 steps it alone on its staged heaps,
// node after node in the reference's order (sc_nodes_serial). Observations and actions go
// through LDS tiles so HBM sees whole rows; the state pointers stay the batch's base
// pointers (ScEnv soff/hoff) so they live in SGPRs.
// The same tile code runs under three more drivers: the rollout kernel (a step loop inside the
// tile loop, the state in LDS between a launch's steps), the closed-loop rollout kernel (the
// same, with each step's action tile computed from the previous step's observation tile by a
// linear policy, scg_sc_policy.h, or a one-hidden-layer ReLU policy, scg_sc_mlp.h, deterministic
// or with the caller's noise added: four instantiations per (MAXD, F64)) and the step server
// (one resident block serving a drop-in env's steps).
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

#include "scg_common.h"
#include "scg_mailbox.h"
#if defined(SCG_NODES_STAMPS) && defined(__HIP_DEVICE_COMPILE__)
// Diagnostic build only: every stamp (the phase boundaries NSTAMP below, and the end of each
// section of the act and heaps phases, SCG_ACCP(ptr, k) in scg_supplychain_core.h / _nodes.h)
// goes to the wave's slots in a static LDS array, and lane 0 copies them to HBM once, at the
// tile's end: a global store per stamp would make the next wait on the vector memory counter
// (loads and stores share it on gfx950) sit out that store's latency.
// LDS slots per wave: 0-7 phase stamps, 8 real-time clock at the start, 9 + j section j
// (sections k = 0..3 -> j = k, k = 7..13 -> j = k - 3).
constexpr int kNLdsSlots = 20;
__shared__ unsigned long long s_nodes_stamps[8 * kNLdsSlots];
#define SCG_STAMP(k)
#define SCG_ACC_DECL
#define SCG_ACC(k)
#define SCG_ACC_STORE
namespace scg {
struct ScAcc {  // a marker: a non-null ScEnv::dbg turns the section stamps on
  int unused;
};
}  // namespace scg
#define SCG_ACCP(ptr, k)                                                                              \
  do {                                                                                                \
    if (ptr) {                                                                                        \
      const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                   \
      if ((threadIdx.x & 63u) == 0)                                                                   \
        s_nodes_stamps[(threadIdx.x / 64u) * kNLdsSlots + 9 + ((k) < 4 ? (k) : (k) - 3)] = now_;      \
    }                                                                                                 \
  } while (0)
#endif
#include "scg_supplychain_core.h"
#include "scg_supplychain_args.h"
#include "scg_supplychain_nodes.h"
#include "scg_sc_nodes_launch.h"

// Diagnostic build only (-DSCG_NODES_STAMPS, tools/nodes_stamps.py): lane 0 of every wave
// records the shader clock at the phase boundaries (0 start, 5 heaps staged, 6 past the first
// barrier, 1 acted, 2 past the second, 3 heaps done, 7 past the third, 4 end) into a buffer of its own that scg_nodes_debug_stamps copies
// out; nothing else reads it. In the product build NSTAMP is empty.
#ifdef SCG_NODES_STAMPS
// Global record per wave: slots 0-7 the phase stamps, 8 and 9 the real-time clock (100 MHz,
// one clock for the chip) at start and end, 10 and 11 the wave's HW_ID and XCC_ID registers
// (where the block was placed), 12 + k the end of section k of the act and heaps phases.
constexpr int kNStampSlots = 28;
constexpr int kNStampWaves = 1 << 14;
__device__ unsigned long long g_nodes_stamps[kNStampWaves * kNStampSlots];
#if defined(__HIP_DEVICE_COMPILE__)
#define NSTAMP(k)                                                                                   \
  do {                                                                                              \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                   \
    unsigned long long* l_ = s_nodes_stamps + (threadIdx.x / 64u) * kNLdsSlots;                     \
    if ((threadIdx.x & 63u) == 0) {                                                                 \
      l_[(k)] = now_;                                                                               \
      if ((k) == 0) l_[8] = __builtin_amdgcn_s_memrealtime();                                       \
    }                                                                                               \
    if ((k) == 4) {                                                                                 \
      const unsigned long long rt_ = __builtin_amdgcn_s_memrealtime();                              \
      const unsigned w_ = blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u;                      \
      if ((threadIdx.x & 63u) == 0 && w_ < static_cast<unsigned>(kNStampWaves)) {                   \
        unsigned long long* s_ = g_nodes_stamps + w_ * kNStampSlots;                                \
        for (int j_ = 0; j_ < 9; ++j_) s_[j_] = l_[j_];                                             \
        s_[9] = rt_;                                                                                \
        s_[10] = __builtin_amdgcn_s_getreg((31 << 11) | 4);                                         \
        s_[11] = __builtin_amdgcn_s_getreg((31 << 11) | 20);                                        \
        for (int j_ = 0; j_ < 4; ++j_) s_[12 + j_] = l_[9 + j_];                                    \
        for (int j_ = 4; j_ < 11; ++j_) s_[12 + 3 + j_] = l_[9 + j_];                               \
      }                                                                                             \
    }                                                                                               \
  } while (0)
#else
#define NSTAMP(k)
#endif
#else
#define NSTAMP(k)
#endif

namespace scg {

constexpr int kNodesMaxWaves = 8;

// Row and column (r, k) of element q = r * width + k of a row-major tile, walked from q0 in
// steps of `step` with one division up front (the step's share is wave-uniform).
struct TileWalk {
  int r, k, dr, dk, width;
  __device__ __forceinline__ TileWalk(int q0, int step, int w) : width(w) {
    r = q0 / w;
    k = q0 - r * w;
    dr = step / w;
    dk = step - dr * w;
  }
  __device__ __forceinline__ void next() {
    r += dr;
    k += dk;
    if (k >= width) {
      k -= width;
      ++r;
    }
  }
};

// One tile of 64 envs (tile * 64 ...): the step described at the top, on the kernel arguments
// `a`, except the step's time, flags and episode, which come from `sp` (sp.t(), sp.flags(),
// sp.episode(): the batch kernel's launch arguments, read where used as before; the step
// server's request), and the action rows (sp.act(a)). With sp.keep_state() the stage reads no
// state: the step server's block stepped this env last and its LDS still holds the stocks,
// sizes, heaps and episode return that step left. lane is the thread's lane, opaque to the
// compiler; w the wave index.
// The step's outputs go where the policy says as well (sp.obs<T>(a), sp.rew(a), sp.term_obs(a):
// the launch arguments' buffers for the batch kernel and the step server, step k's slices of
// them for the rollout kernel), and sp.write_back() says whether the step leaves the env's
// heaps, sizes, stocks and episode return in HBM (always, but for the rollout kernel's steps
// whose successor finds them in LDS). kStreamOut: observation rows with write-through stores
// (device memory) rather than plain ones (the step server's host-mapped rows). kObsOptional:
// sp.obs may be null (a step whose observation nobody asked for).
struct NodesLaunchStep {  // the batch kernel: the step fields of the launch arguments
  static constexpr bool kKeepsState = false;
  static constexpr bool kStreamOut = true;
  static constexpr bool kObsOptional = false;
  static constexpr bool kPolicy = false;
  const ScArgs& a;
  __device__ __forceinline__ int t() const { return a.t; }
  __device__ __forceinline__ int flags() const { return a.flags; }
  __device__ __forceinline__ uint32_t episode() const { return a.episode; }
  __device__ __forceinline__ const float* act(const ScArgs& x) const { return x.act; }
  __device__ __forceinline__ bool keep_state() const { return false; }
  template <class T>
  __device__ __forceinline__ T* obs(const ScArgs& x) const { return static_cast<T*>(x.obs); }
  __device__ __forceinline__ void* term_obs(const ScArgs& x) const { return x.term_obs; }
  __device__ __forceinline__ double* rew(const ScArgs& x) const { return x.rew; }
  __device__ __forceinline__ bool write_back() const { return true; }
};

// Step k of a rollout launch (sc_rollout_nodes_kernel): its time, episode and flags, counted
// on from the launch's first step by the kernel's step loop (wave-uniform: SGPRs), and the
// k-th slices of the launch's action, observation and reward buffers.
struct NodesRolloutStep {
  static constexpr bool kKeepsState = true;  // the episode return travels in LDS (ret0)
  static constexpr bool kStreamOut = true;
  static constexpr bool kObsOptional = true;
  static constexpr bool kPolicy = false;
  int32_t t_, flags_;
  uint32_t episode_;
  int32_t k_;        // the step's index in the launch
  int32_t obs_row_;  // the row block of the observation buffer it writes, -1: none
  bool keep_, write_back_;
  __device__ __forceinline__ int t() const { return t_; }
  __device__ __forceinline__ int flags() const { return flags_; }
  __device__ __forceinline__ uint32_t episode() const { return episode_; }
  __device__ __forceinline__ const float* act(const ScArgs& x) const { return x.act + static_cast<int64_t>(k_) * x.n * x.c.A; }
  __device__ __forceinline__ bool keep_state() const { return keep_; }
  template <class T>
  __device__ __forceinline__ T* obs(const ScArgs& x) const {
    return obs_row_ < 0 ? nullptr : static_cast<T*>(x.obs) + static_cast<int64_t>(obs_row_) * x.n * x.c.O;
  }
  __device__ __forceinline__ void* term_obs(const ScArgs& x) const { return x.term_obs; }
  __device__ __forceinline__ double* rew(const ScArgs& x) const { return x.rew + static_cast<int64_t>(k_) * x.n; }
  __device__ __forceinline__ bool write_back() const { return write_back_; }
};

// Step k of a closed-loop launch (sc_closed_rollout_nodes_kernel): a rollout step whose action
// tile is not loaded but computed, from the observation tile the previous step left (kPolicy:
// the parts of sc_nodes_tile that differ), by the policy Launch carries (its pv an ScPolicyView:
// linear; an ScMlpView, kMlp: one hidden layer). Every output is optional;
// first() / last(): the tile's first and last step in the launch, where obs_io is read and
// obs_io, act_work and reward_sum are written. A sampled launch (ScSampledLaunch, kSampled)
// adds the caller's noise to every action before its clamp: noise(x, n, row) is env n's part of
// noise row `row` of the launch, the row of the step the actions are computed for.
struct NodesNoise {
  const float* std;  // [A]
  const float* eps;  // the env's noise row [A]
  float* out;        // the env's row of samples_out [A], or null
};
// A drawn launch (ScDrawnLaunch, kDrawn): the env's noise row is not in memory but computed,
// element (row, env, q) of the launch's key (csrc/scg_normal.h).
struct NodesDrawn {
  const float* std;  // [A]
  float* out;        // the env's row of samples_out [A], or null
  uint32_t k0, k1, row, env;
  __device__ __forceinline__ float eps(int q) const { return sc_noise_element(k0, k1, row, env, static_cast<uint32_t>(q)); }
};
template <class Launch>
struct NodesClosedStep {
  static constexpr bool kKeepsState = true;
  static constexpr bool kStreamOut = true;
  static constexpr bool kObsOptional = true;
  static constexpr bool kPolicy = true;
  static constexpr bool kMlp = Launch::kMlp;
  static constexpr bool kSampled = Launch::kSampled;
  static constexpr bool kDrawn = Launch::kDrawn;
  const Launch& p;
  int32_t t_, flags_;
  uint32_t episode_;
  int32_t k_;
  bool keep_, write_back_, last_;
  __device__ __forceinline__ int t() const { return t_; }
  __device__ __forceinline__ int flags() const { return flags_; }
  __device__ __forceinline__ uint32_t episode() const { return episode_; }
  __device__ __forceinline__ const float* act(const ScArgs&) const { return nullptr; }  // never loaded
  __device__ __forceinline__ bool keep_state() const { return keep_; }
  template <class T>
  __device__ __forceinline__ T* obs(const ScArgs& x) const {
    return x.obs ? static_cast<T*>(x.obs) + static_cast<int64_t>(k_) * x.n * x.c.O : nullptr;
  }
  __device__ __forceinline__ void* term_obs(const ScArgs& x) const { return x.term_obs; }
  __device__ __forceinline__ double* rew(const ScArgs& x) const {
    return x.rew ? x.rew + static_cast<int64_t>(k_) * x.n : nullptr;
  }
  __device__ __forceinline__ float* actions(const ScArgs& x) const {
    return p.actions_out ? p.actions_out + static_cast<int64_t>(k_) * x.n * x.c.A : nullptr;
  }
  __device__ __forceinline__ bool write_back() const { return write_back_; }
  __device__ __forceinline__ bool first() const { return k_ == 0; }
  __device__ __forceinline__ bool last() const { return last_; }
  __device__ __forceinline__ auto noise(const ScArgs& x, int64_t n, int row) const {
    const int64_t at = sc_sample_index(x.n, x.c.A, row, n, 0);
    if constexpr (kDrawn) {
      return NodesDrawn{p.drw.std, p.drw.samples ? p.drw.samples + at : nullptr, p.drw.k0, p.drw.k1,
                        p.drw.row0 + static_cast<uint32_t>(row), p.drw.env0 + static_cast<uint32_t>(n)};
    } else {
      return NodesNoise{p.smp.std, p.smp.noise + at, p.smp.samples ? p.smp.samples + at : nullptr};
    }
  }
  // what noise() returns: what a step's act holds between its request and its actions
  using Noise = std::conditional_t<kDrawn, NodesDrawn, NodesNoise>;
};

// The closed loop's product: wave w computes actions w, w + W, ... of its lane's env (n) from
// the env's row of the observation tile into its row of the action tile. The observation
// elements are LDS reads at an odd row stride (lanes on distinct banks); an action's parameter
// words (O weights and the bias) are requested together, up to kNodesPolicyChunk per round.
constexpr int kNodesPolicyChunk = 32;

// The sampled closed loop (kSampled steps): the same products with the caller's noise added
// before the clamp (scg_sc_policy.h sc_policy_sample). The thread that computes action q of its
// env reads the env's noise element q itself and, where samples are asked for, writes u to the
// same index: per-thread strided accesses (lane stride A floats), no LDS and no barrier, and
// samples_out may be the noise buffer. The block's threads together read every byte of the
// tile's contiguous span [64][A], so each cache line is fetched from HBM once. The noise does
// not depend on the step before it: a thread requests its first kNodesNoiseAhead elements ahead
// of the first parameter words (the MLP: ahead of the hidden layer's), in the round the
// deterministic loop already waits for; an env with more than kNodesNoiseAhead * W actions
// reads the rest as it comes to them. (Requesting them a phase or a whole step earlier, or
// reading the span coalesced through the action tile, measured no faster: DESIGN §6.13.)
constexpr int kNodesNoiseAhead = 2;
__device__ __forceinline__ void sc_nodes_noise_request(const NodesNoise& nz, int A, int w, int W, float (&ev)[kNodesNoiseAhead]) {
#pragma unroll
  for (int u = 0; u < kNodesNoiseAhead; ++u) ev[u] = w + u * W < A ? nz.eps[w + u * W] : 0.0f;
}
// The drawn step's: no load; the same elements are computed here, ahead of the first parameter
// words, which they do not depend on (one Philox block and one pair per element: a block's other
// pair belongs to another wave's thread, and sharing it would cost LDS and a barrier).
__device__ __forceinline__ void sc_nodes_noise_request(const NodesDrawn& nz, int A, int w, int W, float (&ev)[kNodesNoiseAhead]) {
#pragma unroll
  for (int u = 0; u < kNodesNoiseAhead; ++u) ev[u] = w + u * W < A ? nz.eps(w + u * W) : 0.0f;
}

// Actions w, w + W, ... of the lane's env into its row of the action tile, each the finish
// (scg_sc_policy.h) of z(q), the policy's value of action q before its clamp: the clamp to
// pv.lo .. pv.hi, or for a sampled step the clamp of the sample, with the noise nz and its
// elements requested ahead, ev (neither is read when !kSampled).
template <bool kSampled, class View, class Z>
__device__ __forceinline__ void sc_nodes_actions(const View& pv, int A, int w, int W, float* arow, const Z& z,
                                                 const NodesNoise& nz, const float (&ev)[kNodesNoiseAhead]) {
  if constexpr (kSampled) {
    auto one = [&](int q, float eps) {
      const float sd = nz.std[q];
      float u;
      arow[q] = sc_policy_clamp_sampled(z(q), sd, eps, pv.lo, pv.hi, &u);
      if (nz.out) __hip_atomic_store(&nz.out[q], u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
#pragma unroll
    for (int u = 0; u < kNodesNoiseAhead; ++u)
      if (w + u * W < A) one(w + u * W, ev[u]);
    for (int q = w + kNodesNoiseAhead * W; q < A; q += W) one(q, nz.eps[q]);
  } else {
    for (int q = w; q < A; q += W) arow[q] = sc_policy_clamp(z(q), pv.lo, pv.hi);
  }
}
// The drawn step's (always sampled): elements past those computed ahead are drawn as it comes to them.
template <bool kSampled, class View, class Z>
__device__ __forceinline__ void sc_nodes_actions(const View& pv, int A, int w, int W, float* arow, const Z& z,
                                                 const NodesDrawn& nz, const float (&ev)[kNodesNoiseAhead]) {
  static_assert(kSampled, "a drawn step is a sampled one");
  auto one = [&](int q, float eps) {
    const float sd = nz.std[q];
    float u;
    arow[q] = sc_policy_clamp_sampled(z(q), sd, eps, pv.lo, pv.hi, &u);
    if (nz.out) __hip_atomic_store(&nz.out[q], u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
#pragma unroll
  for (int u = 0; u < kNodesNoiseAhead; ++u)
    if (w + u * W < A) one(w + u * W, ev[u]);
  for (int q = w + kNodesNoiseAhead * W; q < A; q += W) one(q, nz.eps(q));
}

// The linear policy's act, for step sp.k_ + ahead of the launch (its noise row).
template <class Step, class ObsT>
__device__ __forceinline__ void sc_nodes_policy_act(const Step& sp, const ScArgs& a, int ahead, int64_t n, int w, int W,
                                                    const ObsT* orow, float* arow) {
  const ScPolicyView& pv = sp.p.pv;
  const int A = a.c.A, O = a.c.O;
  // the sampled step's alone: a deterministic step sets neither, and sc_nodes_actions<false>
  // reads neither
  [[maybe_unused]] typename Step::Noise nz{};
  [[maybe_unused]] float ev[kNodesNoiseAhead];
  if constexpr (Step::kSampled) {
    nz = sp.noise(a, n, sp.k_ + ahead);
    sc_nodes_noise_request(nz, A, w, W, ev);
  }
  auto o = [&](int j) { return static_cast<float>(orow[j]); };
  sc_nodes_actions<Step::kSampled>(pv, A, w, W, arow,
                                   [&](int q) { return sc_policy_z<kNodesPolicyChunk>(pv, O, n, q, o); }, nz, ev);
}

// The MLP's act (kMlp steps): wave w computes hidden units w, w + W, ... of its lane's env from
// the env's row of the observation tile into the hidden tile [H][64] (float, unit-major, lane
// fastest: the lanes of a wave on consecutive banks; `hid` is the lane's column); past a
// barrier it computes actions w, w + W, ... from that column into the env's row of the action
// tile. Every thread of the block calls it (live: the lane has an env). The hidden tile lies
// over the inbox values and the cost rows, idle where this runs (the note at the end of
// sc_nodes_tile); the launcher admits only H <= 2 * (E + NN).
template <class Step, class ObsT>
__device__ __forceinline__ void sc_nodes_mlp_act(const Step& sp, const ScArgs& a, int ahead, int64_t n, bool live, int w, int W,
                                                 const ObsT* orow, float* arow, float* hid) {
  const ScMlpView& mv = sp.p.pv;
  const int A = a.c.A, O = a.c.O;
  // the sampled step's alone: a deterministic step sets neither, and sc_nodes_actions<false>
  // reads neither
  [[maybe_unused]] typename Step::Noise nz{};
  [[maybe_unused]] float ev[kNodesNoiseAhead];
  if constexpr (Step::kSampled) nz = sp.noise(a, n, sp.k_ + ahead);
  if (live) {
    if constexpr (Step::kSampled) sc_nodes_noise_request(nz, A, w, W, ev);
    auto o = [&](int j) { return static_cast<float>(orow[j]); };
    for (int i = w; i < mv.H; i += W) hid[i * 64] = sc_mlp_hidden<kNodesPolicyChunk>(mv, O, n, i, o);
  }
  __syncthreads();
  if (live) {
    auto h = [&](int i) { return hid[i * 64]; };
    sc_nodes_actions<Step::kSampled>(mv, A, w, W, arow,
                                     [&](int q) { return sc_mlp_z<kNodesPolicyChunk>(mv, O, n, q, h); }, nz, ev);
  }
}

// A closed-loop step's act, whichever of the six its launch is: the actions of every live env
// of the tile for step sp.k_ + ahead of the launch (ahead 0: this step's own, at the launch's
// first step; 1: the next step's), from the observation tile (orow: the lane's row) into the
// action tile act_t; `idle` is the LDS the MLP's hidden tile lies over. Every thread of the block
// calls it (the MLP's barrier). Two things are left to the callees because done by the caller they
// moved pinned instruction counts: the lane's action row is addressed here, for
// the linear policy under `live`, and the noise row is counted from sp.k_ where the noise is
// looked up.
template <class Step, class ObsT>
__device__ __forceinline__ void sc_nodes_closed_act(const Step& sp, const ScArgs& a, int ahead, int64_t n, int lane, bool live,
                                                    int w, int W, const ObsT* orow, float* act_t, double* idle) {
  const int Ap = a.c.A | 1;
  if constexpr (Step::kMlp) {
    sc_nodes_mlp_act(sp, a, ahead, n, live, w, W, orow, act_t + lane * Ap, reinterpret_cast<float*>(idle) + lane);
  } else if (live) {
    sc_nodes_policy_act(sp, a, ahead, n, w, W, orow, act_t + lane * Ap);
  }
}

template <int MAXD, bool F64, bool LED, class Step>
__device__ __forceinline__ void sc_nodes_tile(const ScArgs& a, int64_t tile, int lane, int w, int W, int E,
                                              const Step& sp) {
  using ObsT = typename std::conditional<F64, double, float>::type;
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr bool ledgers = LED;
  const ScCtx& c = a.c;
  const int NN = c.n_nodes, P = c.P, NP = NN * P, H = c.H;
  const int Ap = c.A | 1, Op = c.O | 1;  // odd row strides: lanes hit distinct banks
  double* hval = reinterpret_cast<double*>(smem);
  double* recv = hval + static_cast<int64_t>(NP) * H * 64;  // released sums [NP][64]
  double* ibval = recv + NP * 64;
  double* cost_v = ibval + static_cast<int64_t>(E) * 64;
  double* stk = cost_v + NN * 64;  // the tile's stocks [NP][64] for the step
  double* ret0 = stk + NP * 64;    // episode returns [64] (wave 0's prefetch)
  ObsT* obs_t = reinterpret_cast<ObsT*>(ret0 + 64);
  int32_t* htk = reinterpret_cast<int32_t*>(obs_t + 64 * Op);
  int32_t* hsz = htk + static_cast<int64_t>(NP) * H * 64;
  int32_t* ibtk = hsz + NP * 64;
  int32_t* cost_k = ibtk + static_cast<int64_t>(E) * 64;
  int32_t* amb = cost_k + NN * 64;
  uint64_t* lword = reinterpret_cast<uint64_t*>(amb + W * 64);  // ledger entry marks and types [NP][64]
  float* act_t = reinterpret_cast<float*>(lword + NP * 64);
  const bool terminal = sp.flags() & 1;
  const bool autoreset = sp.flags() & 2;
  const int64_t n0 = tile * 64;
  const int64_t n = n0 + lane;
  const int nb = a.n - n0 < 64 ? static_cast<int>(a.n - n0) : 64;  // envs of this tile
  const bool live = lane < nb;
  auto lheap = [&](int hp) { return HeapView{htk + hp * H * 64 + lane, hval + hp * H * 64 + lane, 64}; };
  // heaps and sizes in HBM (the batch's base pointers, column n); stocks in the LDS copy
  ScEnv g{stk, a.tk, a.val, a.size, 64, a.n, static_cast<uint32_t>(a.env_offset + n), n, sp.episode(), 0};
  g.soff = lane;
  g.hoff = n;
  if (ledgers) {  // the nodes' entries to their slots (column n = base + n0 + soff), reduced below
    g.led_v = a.ledp_v + n0;
    g.led_stride = a.n;
    g.led_word = lword + lane;
    g.led_word_stride = 64;
  }
  NSTAMP(0);
#if defined(SCG_NODES_STAMPS) && defined(__HIP_DEVICE_COMPILE__)
  ScAcc acc_{};
  g.dbg = &acc_;
#define NACC(k) SCG_ACCP(&acc_, k)
#else
#define NACC(k)
#endif

  // the step's observation row, whichever buffer(s) it goes to (chosen at the copy-out)
  ObsT* const orow = obs_t + lane * Op;
  auto sink = [&](int o, double x) { orow[o] = static_cast<ObsT>(x); };
  const NodesInbox in{ibtk + lane, ibval + lane, 64};
  const float* act = act_t + lane * Ap;
  // closed loop: the call's rewards of wave 0's envs, added step by step (the ledger words'
  // rows: a closed-loop launch keeps no ledgers)
  [[maybe_unused]] double* const rsum = reinterpret_cast<double*>(lword);

  if constexpr (Step::kPolicy) {
    if (sp.first()) {  // the observation the envs last produced into the tile, then the first actions
      __syncthreads();  // the block's previous tile is read (its last copy-out) until here
      const ObsT* const src = static_cast<const ObsT*>(sp.p.obs_io) + n0 * c.O;
      TileWalk tw(threadIdx.x, blockDim.x, c.O);
      for (int q = threadIdx.x; q < nb * c.O; q += blockDim.x, tw.next()) obs_t[tw.r * Op + tw.k] = src[q];
      if (w == 0 && live) rsum[lane] = sp.p.sum_add ? sp.p.reward_sum[n] : 0.0;
      __syncthreads();
      // (the noise row of this step: the launch's first)
      sc_nodes_closed_act(sp, a, 0, n, lane, live, w, W, orow, act_t, ibval);
    }
  }

  // stage, one memory round: every thread requests its share of the tile's action rows
  // (one contiguous span), every wave its node's stocks, heap sizes and the first kStage
  // slots of each heap, wave 0 the episode returns; nothing is waited for until all are in
  // flight. Then everything to LDS, the rest of a longer heap, and what each heap releases.
  bool bad = false;
  {
    constexpr int kAct = 4;  // action elements per thread per round
    const float* src = sp.act(a) + n0 * c.A;
    const int na = nb * c.A;
    // the step server's state kept in LDS since its previous request (NodesServerStep)
    const bool keep = sp.keep_state();
    float av[kAct];
    if constexpr (!Step::kPolicy) {  // (the closed loop's action tile is computed, not loaded)
#pragma unroll
      for (int u = 0; u < kAct; ++u)
        if (static_cast<int>(threadIdx.x) + u * static_cast<int>(blockDim.x) < na) av[u] = src[threadIdx.x + u * blockDim.x];
    }
    const double r0 = (w == 0 && live && a.ep_ret && !keep) ? a.ep_ret[n] : 0.0;
    for (int i = w; i < NN; i += W)
      for (int p = 0; p < P; ++p) {
        const int hp = i * P + p;
        if (!live) continue;
        if (keep) {  // stocks, sizes and heaps are this env's, as the last step left them
          bad |= !sc_recv_scan(lheap(hp), hsz[hp * 64 + lane], sp.t(), recv[hp * 64 + lane]);
          continue;
        }
        const int64_t r = static_cast<int64_t>(hp) * a.n + n;
        const double st = a.stock[r];
        const int32_t sz = a.size[r];
        stk[hp * 64 + lane] = st;
        hsz[hp * 64 + lane] = sz;
        const HeapView lh = lheap(hp);
        // the heap's first slots are requested with the size (sc_nodes_copy_heap, shared
        // with the host harness); a longer heap costs a round more
        sc_nodes_copy_heap(HeapView{a.tk + static_cast<int64_t>(hp) * H * a.n + n,
                                    a.val + static_cast<int64_t>(hp) * H * a.n + n, a.n},
                           lh, H, sz);
        bad |= !sc_recv_scan(lh, sz, sp.t(), recv[hp * 64 + lane]);
      }
    if constexpr (!Step::kPolicy) {
      TileWalk tw(threadIdx.x, blockDim.x, c.A);
#pragma unroll
      for (int u = 0; u < kAct; ++u, tw.next())
        if (static_cast<int>(threadIdx.x) + u * static_cast<int>(blockDim.x) < na) act_t[tw.r * Ap + tw.k] = av[u];
      for (int q = threadIdx.x + kAct * blockDim.x; q < na; q += blockDim.x, tw.next()) act_t[tw.r * Ap + tw.k] = src[q];
    }
    if (w == 0 && live && a.ep_ret && !keep) ret0[lane] = r0;
  }
  amb[w * 64 + lane] = bad ? 1 : 0;
  NSTAMP(5);
  __syncthreads();
  NSTAMP(6);
  bool flagged = (sp.flags() & 4) != 0;
  for (int v = 0; v < W; ++v) flagged |= amb[v * 64 + lane] != 0;
  const bool go = live && !flagged;

  if constexpr (Step::kPolicy) {
    // closed loop: the step's action rows out where asked (actions_out[k]; act_work at the
    // launch's last step), one contiguous span per block like the observation rows; the
    // barrier above published the tile, and nothing writes it before the step's third
    float* const adst0 = sp.actions(a);
    float* const adst1 = sp.last() ? sp.p.act_work : nullptr;
    if (adst0 || adst1) {
      TileWalk tw(threadIdx.x, blockDim.x, c.A);
      for (int q = threadIdx.x; q < nb * c.A; q += blockDim.x, tw.next()) {
        const float x = act_t[tw.r * Ap + tw.k];
        if (adst0) __hip_atomic_store(&adst0[n0 * c.A + q], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (adst1) __hip_atomic_store(&adst1[n0 * c.A + q], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }

  // act: every node at once (a node's act needs only what its own heaps release)
  if (go)
    for (int i = w; i < NN; i += W) {
      const Num cst = sc_nodes_act<MAXD, !LED>(c, g, in, recv + i * P * 64 + lane, 64, act, sp.t(), i);
      NACC(12);
      cost_v[i * 64 + lane] = cst.v;
      cost_k[i * 64 + lane] = cst.k;
      for (int p = 0; p < P; ++p) sc_observe_stock(c, g, i, p, sink);
      NACC(13);
    }
  NSTAMP(1);
  __syncthreads();
  NSTAMP(2);

  // heaps
  if (go)
    for (int i = w; i < NN; i += W) {
      WordCache ltc{0, U4{0, 0, 0, 0}, false};
      int a_i = 0, lt_i = 0;
      for (int p = 0; p < P; ++p) {
        const int hp = i * P + p;
        sc_nodes_heap<true>(c, g, lheap(hp), hsz[hp * 64 + lane], in, ltc, act, sp.t(), i, p, a_i, lt_i, sink, false,
                            sp.write_back());
      }
    }
  NSTAMP(3);

  // ledgers: entry q of an env, the nodes' entries added in node order (:750-760); at an
  // auto-reset the finished episode's ledger is kept and the new one starts at int 0
  auto ledger_put = [&](int q, double lv, int32_t lk) {
    const int64_t at = q * a.n + n;
    if (autoreset) {
      if (a.led_fv) {
        a.led_fv[at] = lv;
        a.led_fk[at] = lk;
      }
      lv = 0.0;
      lk = np_kind_abi(NK_INT);
    }
    a.led_v[at] = lv;
    a.led_k[at] = lk;
  };
  // entries first, first + step, ... of an env, two at a time (their loads in flight together)
  auto ledger_entries = [&](int first, int step) {
    const int nq = 2 * SCG_SC_LEDGER_KEYS * P;
    for (int q0 = first; q0 < nq; q0 += 2 * step) {
      const int q1 = q0 + step < nq ? q0 + step : -1;
      const int64_t at0 = q0 * a.n + n, at1 = (q1 >= 0 ? q1 : q0) * a.n + n;
      double lv0 = a.led_v[at0], lv1 = a.led_v[at1];
      int32_t lk0 = a.led_k[at0], lk1 = a.led_k[at1];
      sc_ledger_reduce_pair(c, q0, q1, a.ledp_v + n, a.n, lword + lane, 64, lv0, lk0, lv1, lk1);
      ledger_put(q0, lv0, lk0);
      if (q1 >= 0) ledger_put(q1, lv1, lk1);
    }
  };
  // Every slot and mark of an acted env is in place since the act barrier, so each wave
  // reduces its share of the entries as soon as its heaps are done: the slot loads overlap
  // the other waves' heaps and wave 0's reward instead of forming a phase of their own after
  // the last barrier (A/B in DESIGN §6.7). A flagged env's slots are written by wave 0's
  // serial walk below, which then reduces that env's entries itself.
  if (ledgers && live && !flagged) ledger_entries(w, W);

  // reward
  if (w == 0 && live) {
    double reward;
    if (flagged) {  // untouched by act and heaps: the serial walk on its staged heaps
      reward = sc_nodes_serial<MAXD, !LED>(c, g, lheap, hsz + lane, 64, in, act, sp.t(), sink, sp.write_back());
      if (ledgers) ledger_entries(0, 1);
    } else {
      Num total = pyint(0);
      for (int i = 0; i < NN; ++i) total = np_add(total, Num{cost_v[i * 64 + lane], cost_k[i * 64 + lane]});
      reward = np_neg(total).v;
    }
    if constexpr (Step::kPolicy) {
      if (double* const rw = sp.rew(a)) rw[n] = reward;
      rsum[lane] = rsum[lane] + reward;
    } else {
      sp.rew(a)[n] = reward;
    }
    if (a.ep_ret) {
      const double r = ret0[lane] + reward;  // episode_rewards += current_reward (:739)
      if (terminal && a.final_ret) a.final_ret[n] = r;
      if (sp.write_back()) a.ep_ret[n] = autoreset ? 0.0 : r;
      if constexpr (Step::kKeepsState) ret0[lane] = autoreset ? 0.0 : r;  // the next request's
    }
    for (int k = 0; k < c.R * c.P; ++k) sc_observe_demand(c, g, sp.t(), k, sink);  // (:771)
    sc_observe_tail(c, sp.t(), sink);                                               // (:786)
  }
  __syncthreads();
  NSTAMP(7);

  // out: the tile is this step's observation — obs, or the terminal observation when the
  // env resets now (then wave 0 writes the reset observation to obs), or both
  ObsT* const dst0 = autoreset ? static_cast<ObsT*>(sp.term_obs(a)) : sp.template obs<ObsT>(a);
  ObsT* const dst1 = (terminal && !autoreset) ? static_cast<ObsT*>(sp.term_obs(a)) : nullptr;
  TileWalk tw(threadIdx.x, blockDim.x, c.O);
  for (int q = threadIdx.x; q < nb * c.O; q += blockDim.x, tw.next()) {
    const ObsT x = obs_t[tw.r * Op + tw.k];
    // rows written once per step and read by the next: streaming rather than plain stores
    // (sc-2perstage 37.4 -> 36.7 us, profiles/r05j_nodes_nt_ab.log), write-through like the heap
    // copy-back (sc_nodes_heap); the step server's rows go to host-mapped memory: plain stores there
    if constexpr (Step::kStreamOut) {
      if (dst0) __hip_atomic_store(&dst0[n0 * c.O + q], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (dst1) __hip_atomic_store(&dst1[n0 * c.O + q], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      if (dst0) dst0[n0 * c.O + q] = x;
      if (dst1) dst1[n0 * c.O + q] = x;
    }
  }
  if (autoreset) {  // after the barrier every wave's heap copy-back has landed
    // closed loop: wave 0 puts the reset observation into the tile as well (the policy's next
    // input), once every thread has copied the terminal one out of it
    if constexpr (Step::kPolicy) __syncthreads();
    if (w == 0 && live) {
      g.episode = sp.episode() + 1;
      g.led_v = nullptr;   // the ledger was restarted above
      sc_reset_env(c, g);  // heaps in HBM, stocks in the LDS copy
      ObsT* const robs = sp.template obs<ObsT>(a);
      if constexpr (Step::kPolicy) {
        auto both = [&](int o, double x) {
          orow[o] = static_cast<ObsT>(x);
          if (robs) robs[n * c.O + o] = static_cast<ObsT>(x);
        };
        sc_observe(c, g, 0, both);
      } else if (!Step::kObsOptional || robs) {
        ObsRow out{robs, n * c.O, F64 ? 1 : 0};
        sc_observe(c, g, 0, out);
      }
      // The rollout kernel's next step stages the new episode's heap and size rows from HBM,
      // every wave its own nodes' — rows wave 0 wrote just above with plain stores. The
      // barrier below orders them: __syncthreads() is a workgroup-scope release fence (this
      // wave waits until its stores have completed), the barrier, and a workgroup-scope
      // acquire fence. No cache action is needed on top: the waves of a workgroup run on one
      // CU (the kernels are not built for threadgroup-split mode) and share its vector L1,
      // through which both the stores (write-through) and the loads go — the LLVM AMDGPU
      // memory model for gfx90a/gfx942 ("no special action is required for coherence between
      // wavefronts in the same work-group" outside tgsplit mode). The explicit wait keeps the
      // stores' completion from depending on what the fence lowers to.
      if constexpr (Step::kObsOptional) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
  }
  if constexpr (Step::kPolicy) {
    // closed loop: the tile now holds the observation the envs produced (past the third
    // barrier; at an auto-reset step the reset one, past the barrier just above) and no one
    // reads this step's action tile any more: every wave computes its share of the next
    // step's, which that step's first barrier publishes. The launch's last step writes the
    // tile to obs_io instead, and wave 0 the rewards' sums.
    if (sp.last()) {
      ObsT* const dst = static_cast<ObsT*>(sp.p.obs_io) + n0 * c.O;
      TileWalk tw2(threadIdx.x, blockDim.x, c.O);
      for (int q = threadIdx.x; q < nb * c.O; q += blockDim.x, tw2.next())
        __hip_atomic_store(&dst[q], obs_t[tw2.r * Op + tw2.k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (w == 0 && live) sp.p.reward_sum[n] = rsum[lane];
    } else {  // the next step's noise row (this is not the launch's last step)
      sc_nodes_closed_act(sp, a, 1, n, lane, live, w, W, orow, act_t, ibval);
    }
  }
  if (live) {  // the stocks of this wave's nodes back, one 64-env row per instruction (the
               // next tile's stage rewrites these rows: the same wave)
    if (sp.write_back())
      for (int i = w; i < NN; i += W)
        for (int p = 0; p < P; ++p)
          __hip_atomic_store(&a.stock[(i * P + p) * a.n + n], stk[(i * P + p) * 64 + lane], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    if (g.overflow) atomicOr(a.err, 1);
  }
  NSTAMP(4);
#undef NACC
  // the next tile's stage rewrites the action tile, ret0 and, per wave, only the stock, size
  // and heap rows of its own nodes (whose stocks it copied back just above); the rows other
  // waves read (the observation tile) are next written after that tile's first barrier.
  // The same holds when the next "tile" is these envs one step later (the step server, the
  // rollout kernel): every read of the action tile, the inbox, the cost rows and — by wave
  // 0's serial walk and reset — of other waves' heap, size and stock rows lies before this
  // step's last barrier, which every thread has passed before it stages the next step; a
  // kept step's stage writes only the wave's own released sums and flag row and the action
  // tile, a reloading one also its own stock, size and heap rows (the stock rows it stored
  // just above itself: same thread, same address, program order) and wave 0 ret0, which only
  // wave 0 reads.
  // The closed loop (kPolicy) adds one writer and one reader to that picture: the next action
  // tile is written past this step's last barrier (after every read of the current one) and
  // read past the next step's first; the observation tile is read here, before that same
  // barrier, past which the next step's act phase first writes it. A tile's first step in a
  // launch opens with a barrier of its own before it overwrites the observation tile the
  // block's previous tile may still be copying out.
  // All four instantiations of the closed-loop kernel (linear or MLP, deterministic or sampled)
  // share that picture; the noise of a sampled step touches no LDS. The two MLP instantiations
  // keep their hidden tile [H][64] (float) over ibval and cost_v, which are adjacent:
  // (E + NN) * 512 bytes, H <= 2 * (E + NN) units (sc_mlp_fused_hidden_max; the launcher
  // refuses more). It is written and read only inside sc_nodes_mlp_act, i.e. at
  // first() past the obs_io load's barrier and after a step's last barrier (the auto-reset
  // one included). That is safe because
  //  - the region's last read in a step lies before that step's last barrier: ibval by the
  //    heaps phase (sc_nodes_heap's inbox pushes) and wave 0's serial walk, cost_v by wave 0's
  //    reward sum; nothing after the barrier (copy-out, reset, obs_io / reward_sum stores,
  //    stock write-back) names either;
  //  - no stage writes it: a kept or reloading stage writes recv, amb, the action tile (not
  //    even that in a closed loop), the wave's own stk / hsz / heap rows and ret0;
  //  - its next write is the next step's act phase (in.ship's values, cost_v), past that
  //    step's first barrier, which no wave passes before every wave has left
  //    sc_nodes_mlp_act; an inbox value is read only under a time word (ibtk, not
  //    overlaid) >= 0, and every time word is cleared and every shipped value written in the
  //    same act phase (or serial walk) before it is read, so no stale value under the hidden
  //    tile is ever used;
  //  - the reset path (sc_reset_env, sc_observe) touches the HBM heaps and sizes, stk and the
  //    observation tile only.
  // stk starts right behind cost_v: a hidden tile wider than the bound would overwrite stocks.
}

// Four waves per SIMD (<= 128 VGPRs): two blocks of eight waves per CU, which is also what
// their LDS allows.
constexpr int kNodesWavesPerEu = 4;
// F64: float64 observations; LED: build_info ledgers (a separate instantiation, so the
// ledger code costs the common run nothing).
// Persistent: block b steps tiles b, b + gridDim.x, ... (64 envs each); the launch sizes the
// grid to the blocks the device holds at once, so the second round of tiles needs no new
// blocks and each block's next tile follows its last without a dispatch.
template <int MAXD, bool F64, bool LED>
__global__ __launch_bounds__(64 * kNodesMaxWaves) __attribute__((amdgpu_waves_per_eu(kNodesWavesPerEu)))
void sc_step_nodes_kernel(const ScArgs a_arg, int W, int E) {
  // the wave index is wave-uniform: said so, node records are read with scalar loads
  const int lane0 = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_tiles = (a_arg.n + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    // the lane index, opaque to the compiler inside each tile: the per-lane LDS and HBM
    // addresses derived from it are computed where used, not hoisted out of the tile loop
    // and held in registers across it (which spilled the kernel at its 128-VGPR budget)
    int lane;
    asm volatile("v_mov_b32 %0, %1" : "=v"(lane) : "v"(lane0));
    // the launch arguments through a pointer the compiler cannot see across tiles: each tile
    // reads them (scalar loads) and derives its addresses itself, instead of every derived
    // value being hoisted out of the loop and held in scalar registers across it
    typedef const __attribute__((address_space(4))) ScArgs* KArgPtr;
    KArgPtr ap = (KArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ap));
    const ScArgs& a = *(const ScArgs*)ap;
    sc_nodes_tile<MAXD, F64, LED>(a, tile, lane, w, W, E, NodesLaunchStep{a});
  }
}

// ---- rollout: K steps per launch, the state in LDS between them (scg_sc_rollout) ----------
// The batch kernel's block, LDS layout and persistent tile loop, with a step loop inside: a
// block takes a tile of 64 envs through all K steps of the launch before its next tile, and
// between two steps the tile's stocks, heap sizes, heaps and episode returns stay in LDS
// (keep_state(), as the step server's between two requests). Step k of the launch reads the
// action rows [k][N][A] and writes reward row [k][N] and, by obs_mode, observation rows
// [k][N][O] (0), the one [N][O] buffer at the launch's last step only (1), or none (2).
// Launch arguments: a.t the first step's time (1..T), a.episode its episode, a.flags bit1
// "reset at every terminal step" (else the launcher lets no step follow a terminal one),
// bit2 the serial walk. Step k's time, episode and flags are counted on from those: all
// wave-uniform, in SGPRs.
// HBM sees the state only where a later reader needs it there (write_back()): at the
// launch's last step, and at an auto-reset step — sc_reset_env writes the new episode's
// heaps and sizes to HBM (wave 0, every node's), not to the other waves' LDS rows, so the
// step after a reset stages from HBM like a launch's first (keep_state() false; the barrier
// that orders it: the end of sc_nodes_tile). A kept step neither loads nor stores state:
// its memory rounds are the action rows in, the reward and observation rows out.
template <int MAXD, bool F64>
__global__ __launch_bounds__(64 * kNodesMaxWaves) __attribute__((amdgpu_waves_per_eu(kNodesWavesPerEu)))
void sc_rollout_nodes_kernel(const ScArgs a_arg, int W, int E, int K, int obs_mode) {
  const int lane0 = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_tiles = (a_arg.n + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    int32_t t = a_arg.t;
    uint32_t episode = a_arg.episode;
    bool keep = false;  // the tile's first step in the launch stages from HBM
    for (int k = 0; k < K; ++k) {
      // lane and launch arguments opaque per step, as per tile in the batch kernel: nothing
      // derived from them is carried from one step's code into the next
      int lane;
      asm volatile("v_mov_b32 %0, %1" : "=v"(lane) : "v"(lane0));
      typedef const __attribute__((address_space(4))) ScArgs* KArgPtr;
      KArgPtr ap = (KArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
      asm volatile("" : "+s"(ap));
      const ScArgs& a = *(const ScArgs*)ap;
      const bool terminal = t == a.c.T;
      const bool autoreset = terminal && (a.flags & 2);
      const bool last = k == K - 1;
      NodesRolloutStep sp;
      sp.t_ = t;
      sp.flags_ = (terminal ? 1 : 0) | (autoreset ? 2 : 0) | (a.flags & 4);
      sp.episode_ = episode;
      sp.k_ = k;
      sp.obs_row_ = obs_mode == 0 ? k : (obs_mode == 1 && last) ? 0 : -1;
      sp.keep_ = keep;
      sp.write_back_ = last || autoreset;
      sc_nodes_tile<MAXD, F64, false>(a, tile, lane, w, W, E, sp);
      keep = !autoreset;
      if (autoreset) {
        t = 1;
        ++episode;
      } else {
        ++t;
      }
    }
  }
}

// ---- closed-loop rollout: the rollout kernel with the action tile computed on chip --------
// (scg_sc_rollout_policy, scg_sc_rollout_mlp, scg_sc_rollout_sampled, scg_sc_rollout_drawn;
// csrc/scg_sc_policy.h, csrc/scg_sc_mlp.h, csrc/scg_normal.h.) The rollout kernel's block, LDS layout, persistent tile loop and step loop
// under NodesClosedStep<Launch>: a tile's first step in the launch loads its envs' last
// observation rows (obs_io) into the observation tile and computes the first action tile from
// it; after every other step each wave computes its share of the next action tile from the
// observation tile the step just completed, so between two kept steps nothing crosses HBM but
// the policy's parameter words (and the outputs asked for, and a sampled launch's noise). The
// launch's last step leaves obs_io, act_work, reward_sum and the state in HBM.
// One kernel template, six instantiations per (MAXD, F64), one per launch type: the linear
// policy or the one-hidden-layer policy, deterministic (ScClosedLaunch), sampled from the caller's
// noise (ScSampledLaunch) or from noise computed here (ScDrawnLaunch, scg_sc_rollout_drawn). Where the linear step computes its action tile, every wave of an MLP step
// first computes its share of the hidden units into a tile over LDS the step leaves idle there
// (sc_nodes_mlp_act; the note at the end of sc_nodes_tile), so the block's LDS is the same for
// all six; what a launch type does not use (the hidden stage, the noise) is not in its code.
// The step loop is this kernel's body and, once more, the open-loop rollout kernel's: as the
// body of a kernel template it compiles for every launch type to the code of a kernel written
// out for that type alone (instruction counts, registers and scratch compared per
// instantiation), whereas moved into an inline function that separate kernels
// call it compiled to other code for the linear kernel. The counter the two loops share (t,
// episode, keep, the flag word) stays written out in both as well: as a small struct advanced
// by both loops it left the 24 closed-loop kernels as they were but moved all three open-loop
// kernels tried (sc_rollout_nodes_kernel<4, true> from 16,867 to 16,718 instructions, <2, false>
// 13,247 to 13,233, <8, true> 26,609 to 26,605), whose counts are pinned.
template <class Launch>
struct ScClosedKArgs {
  ScArgs a;
  Launch p;
};

template <int MAXD, bool F64, class Launch>
__global__ __launch_bounds__(64 * kNodesMaxWaves) __attribute__((amdgpu_waves_per_eu(kNodesWavesPerEu)))
void sc_closed_rollout_nodes_kernel(const ScClosedKArgs<Launch> k_arg, int W, int E, int K) {
  const int lane0 = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_tiles = (k_arg.a.n + 63) / 64;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    int32_t t = k_arg.a.t;
    uint32_t episode = k_arg.a.episode;
    bool keep = false;
    for (int k = 0; k < K; ++k) {
      // lane and launch arguments opaque per step, as in the rollout kernel
      int lane;
      asm volatile("v_mov_b32 %0, %1" : "=v"(lane) : "v"(lane0));
      typedef const __attribute__((address_space(4))) ScClosedKArgs<Launch>* KArgPtr;
      KArgPtr ap = (KArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
      asm volatile("" : "+s"(ap));
      const ScClosedKArgs<Launch>& ka = *(const ScClosedKArgs<Launch>*)ap;
      const ScArgs& a = ka.a;
      const bool terminal = t == a.c.T;
      const bool autoreset = terminal && (a.flags & 2);
      const bool last = k == K - 1;
      NodesClosedStep<Launch> sp{ka.p};
      sp.t_ = t;
      sp.flags_ = (terminal ? 1 : 0) | (autoreset ? 2 : 0) | (a.flags & 4);
      sp.episode_ = episode;
      sp.k_ = k;
      sp.keep_ = keep;
      sp.write_back_ = last || autoreset;
      sp.last_ = last;
      sc_nodes_tile<MAXD, F64, false>(a, tile, lane, w, W, E, sp);
      keep = !autoreset;
      if (autoreset) {
        t = 1;
        ++episode;
      } else {
        ++t;
      }
    }
  }
}

// ---- step server for the drop-in SupplyChainEnv (include/scgpu.h scg_sc_server_*) --------
// One block of the batch kernel's shape, resident: wave 0 polls the mailbox's request lines
// (the request and the inline action row, lanes 0-31, system scope, with the exit word) and
// puts what it found in LDS; after a barrier every wave either exits, sleeps and polls again,
// or runs tile 0 of the step with the request's time, flags, episode and action row
// (NodesServerStep) — the batch kernel's code, minus the state loads when the block's LDS
// still holds the state of this env's previous step — and then, past a barrier, thread 0
// publishes the request number with a system-scope release store (wave 0 acquired when it
// found the request: one cache invalidation and one L2 write-back per step for the block). At launch the
// last request served is the answer word, so a request posted while no block ran is served
// first. It exits when exit_req changes or after idle_ticks of the 100 MHz real-time clock
// without a request, and writes the exit word it saw as it goes.
__shared__ int32_t s_srv_req[5];  // t, flags, episode, command (0 none, 1 / 3 step, 2 exit), keep
__shared__ float s_srv_act[16];   // env 0's action row when it travelled in the request
#ifdef SCG_NODES_STAMPS
// Diagnostic build only (tools/sc_server_phase_probe.py): per wave, the shader clocks of each
// phase of every served step summed — [0] request seen -> tile start, then the tile's phases
// in order (stamps 0 -> 5 -> 6 -> 1 -> 2 -> 3 -> 7 -> 4), [8] tile end -> past the closing
// barrier, [9] the steps served — read without a device sync by scg_sc_server_debug_phases.
__device__ unsigned long long g_srv_phases[kNodesMaxWaves][10];
__shared__ unsigned long long s_srv_seen;
#endif
struct NodesServerStep {
  static constexpr bool kKeepsState = true;
  static constexpr bool kStreamOut = false;  // host-mapped rows
  static constexpr bool kObsOptional = false;
  static constexpr bool kPolicy = false;
  bool inline_act;
  template <class T>
  __device__ __forceinline__ T* obs(const ScArgs& x) const { return static_cast<T*>(x.obs); }
  __device__ __forceinline__ void* term_obs(const ScArgs& x) const { return x.term_obs; }
  __device__ __forceinline__ double* rew(const ScArgs& x) const { return x.rew; }
  __device__ __forceinline__ bool write_back() const { return true; }
  __device__ __forceinline__ int t() const { return s_srv_req[0]; }
  __device__ __forceinline__ int flags() const { return s_srv_req[1]; }
  __device__ __forceinline__ uint32_t episode() const { return static_cast<uint32_t>(s_srv_req[2]); }
  __device__ __forceinline__ const float* act(const ScArgs& x) const { return inline_act ? s_srv_act : x.act; }
  __device__ __forceinline__ bool keep_state() const { return s_srv_req[4] != 0; }
};

template <int MAXD>
__global__ __launch_bounds__(64 * kNodesMaxWaves) void sc_nodes_server_kernel(const ScArgs a, int W, int E,
                                                                               scg_sc_server_box* box,
                                                                               uint32_t exit_seen, uint32_t idle_ticks) {
  const int lane0 = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t* line = reinterpret_cast<const uint32_t*>(box);
  uint32_t last = __hip_atomic_load(&box->done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  uint32_t ex = exit_seen;
  uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  // wave 0: whether the LDS holds an env state this block stepped, and that step's episode
  // and time (a request for the next time of the same episode finds its state there)
  bool have = false;
  uint32_t last_ep = 0;
  int32_t last_t = 0;
  for (;;) {
    if (w == 0) {
      // the request (line 0) and the inline action row (line 1) in one load, with the exit word
      const uint32_t v = lane0 < 32 ? __hip_atomic_load(line + lane0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0u;
      ex = __hip_atomic_load(&box->exit_req, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      uint32_t q[32];
#pragma unroll
      for (int i = 0; i < 32; ++i) q[i] = __builtin_amdgcn_readlane(v, i);
      int cmd = 0;
      if (ex != exit_seen) {
        cmd = 2;
      } else if (q[0] != last && q[7] == mailbox_check(q)) {
        cmd = (q[5] & 1u) ? 3 : 1;  // 3: a step whose action row came in line 1
        last = q[0];
        const int32_t t = static_cast<int32_t>(q[2]);
        const bool keep = have && !(q[5] & 2u) && q[4] == last_ep && t == last_t + 1;
        if (lane0 == 0) {
          s_srv_req[0] = t;
          s_srv_req[1] = static_cast<int32_t>(q[3]);
          s_srv_req[2] = static_cast<int32_t>(q[4]);
          s_srv_req[4] = keep ? 1 : 0;
        }
        if (lane0 >= 16 && lane0 < 32) s_srv_act[lane0 - 16] = __uint_as_float(v);
        // the acquire for the whole block: one wave's invalidation of the CU's caches and the
        // L2 serves every wave, which the barrier below orders after it
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
#ifdef SCG_NODES_STAMPS
        if (lane0 == 0) s_srv_seen = __builtin_amdgcn_s_memtime();
#endif
        have = true;
        last_ep = q[4];
        last_t = t;
      } else if (__builtin_amdgcn_s_memrealtime() - t0 > idle_ticks) {
        cmd = 2;
      }
      if (lane0 == 0) s_srv_req[3] = cmd;
    }
    __syncthreads();
    const int cmd = __builtin_amdgcn_readfirstlane(s_srv_req[3]);
    __syncthreads();  // every wave has read the command before wave 0 writes the next one
    if (cmd == 2) break;
    if (cmd == 0) {
      __builtin_amdgcn_s_sleep(2);
      continue;
    }
    int lane;
    asm volatile("v_mov_b32 %0, %1" : "=v"(lane) : "v"(lane0));
    sc_nodes_tile<MAXD, true, false>(a, 0, lane, w, W, E, NodesServerStep{cmd == 3});
    // every wave's stores happen before thread 0's system-scope release store through the
    // barrier, so one write-back of the L2 (the store's release) publishes them all; a fence in
    // each of the W waves would write the L2 back W times (2.5 us per step for W = 8)
    __syncthreads();
#if defined(SCG_NODES_STAMPS) && defined(__HIP_DEVICE_COMPILE__)
    {
      const unsigned long long past = __builtin_amdgcn_s_memtime();
      const unsigned long long* l_ = s_nodes_stamps + w * kNLdsSlots;
      if (lane0 == 0 && w < kNodesMaxWaves) {
        const int order[8] = {0, 5, 6, 1, 2, 3, 7, 4};
        unsigned long long* acc = g_srv_phases[w];
        acc[0] += l_[0] - s_srv_seen;
        for (int k = 1; k < 8; ++k) acc[k] += l_[order[k]] - l_[order[k - 1]];
        acc[8] += past - l_[4];
        acc[9] += 1;
      }
    }
#endif
    if (threadIdx.x == 0) __hip_atomic_store(&box->done_seq, last, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    t0 = __builtin_amdgcn_s_memrealtime();
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  if (threadIdx.x == 0) __hip_atomic_store(&box->exit_seq, ex, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// LDS bytes of one block (the layout above); obs_bytes 4 (float) or 8 (double).
size_t sc_nodes_lds_bytes(int n_nodes, int P, int H, int E, int W, int A, int O, int obs_bytes) {
  const size_t NP = static_cast<size_t>(n_nodes) * P;
  return 64 * ((NP * H + 2 * NP + E + n_nodes + 1) * 8 + static_cast<size_t>(O | 1) * obs_bytes +
               (NP * H + NP + E + n_nodes + W) * 4 + NP * 8 + static_cast<size_t>(A | 1) * 4);
}

// Widest destination list the kernel is instantiated for (its split runs in registers).
int sc_nodes_max_dests() { return 8; }

// Waves per block for a chain: one per node up to kNodesMaxWaves.
int sc_nodes_waves(int n_nodes) { return n_nodes < kNodesMaxWaves ? n_nodes : kNodesMaxWaves; }

// A block may use up to the CU's whole LDS (gfx950: 160 KiB; asked of the device once, the
// gfx950 figure when no device answers, e.g. scg_sc_prepare on a host without a GPU); past
// 64 KiB the kernel is told once per device that it may.
constexpr size_t kNodesLdsGfx950 = 160 * 1024;
size_t sc_nodes_lds_max() {
  static std::atomic<size_t> cached{0};
  size_t v = cached.load(std::memory_order_relaxed);
  if (v) return v;
  int dev = 0, bytes = 0;
  v = (hipGetDevice(&dev) == hipSuccess &&
       hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) == hipSuccess && bytes > 0)
          ? static_cast<size_t>(bytes)
          : kNodesLdsGfx950;
  cached.store(v, std::memory_order_relaxed);
  return v;
}

// Blocks the device holds at once for this kernel instantiation (occupancy x CUs), asked once
// per device and shape; the persistent grid is that many blocks, or one per tile when fewer.
template <auto kKernel>
int64_t sc_nodes_resident_blocks(int dev, int W, size_t lds) {
  struct Entry {
    int dev, W;
    size_t lds;
    int64_t blocks;
  };
  static std::mutex mu;
  static std::vector<Entry> cache;
  std::lock_guard<std::mutex> lock(mu);
  for (const Entry& e : cache)
    if (e.dev == dev && e.W == W && e.lds == lds) return e.blocks;
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kKernel), 64 * W, lds) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || per_cu < 1 || cus < 1)
    return 0;  // unknown: one block per tile
  cache.push_back(Entry{dev, W, lds, static_cast<int64_t>(per_cu) * cus});
  return cache.back().blocks;
}

std::atomic<int> g_nodes_max_blocks{0};  // scg_sc_nodes_max_blocks (tests)
#ifdef SCG_NODES_STAMPS
constexpr size_t kNodesStaticLds = 8 * 20 * sizeof(unsigned long long);  // s_nodes_stamps
#else
constexpr size_t kNodesStaticLds = 0;
#endif

// Past 64 KiB of dynamic LDS a kernel is told, once per device, how much it may use.
template <auto kKernel>
bool sc_nodes_allow_lds(size_t lds, size_t limit, int& dev) {
  static std::atomic<bool> raised[64] = {};  // per device
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (lds <= 64 * 1024 || raised[dev].load(std::memory_order_acquire)) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kKernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(limit)) != hipSuccess)
    return false;
  raised[dev].store(true, std::memory_order_release);
  return true;
}

template <int MAXD, bool F64, bool LED>
int sc_launch_nodes_d(const ScArgs& a, int W, int E, hipStream_t s) {
  const size_t lds = sc_nodes_lds_bytes(a.c.n_nodes, a.c.P, a.c.H, E, W, a.c.A, a.c.O, F64 ? 8 : 4);
  if (lds > sc_nodes_lds_max()) return fail(SCG_ERR_INVALID, "node-parallel kernel: %zu B of LDS per block", lds);
  int dev = 0;
  if (!sc_nodes_allow_lds<&sc_step_nodes_kernel<MAXD, F64, LED>>(lds, sc_nodes_lds_max() - kNodesStaticLds, dev))
    return fail(SCG_ERR_HIP, "node-parallel kernel: cannot raise its LDS limit");
  const int64_t tiles = (a.n + 63) / 64;
  int64_t blocks = tiles;
  // the ledger instantiation keeps one block per tile (persistent measured 55.4 -> 56.7 us,
  // profiles/r05f_nodes_persistent_ab.log)
  if (!LED) {
    const int64_t resident = sc_nodes_resident_blocks<&sc_step_nodes_kernel<MAXD, F64, LED>>(dev, W, lds);
    if (resident > 0 && resident < tiles) blocks = resident;
  }
  const int cap = g_nodes_max_blocks.load(std::memory_order_relaxed);
  if (cap > 0 && cap < blocks) blocks = cap;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(sc_step_nodes_kernel<MAXD, F64, LED>), dim3(static_cast<unsigned>(blocks)),
                     dim3(64 * W), lds, s, a, W, E);
  return check_launch("sc_step_nodes_kernel");
}

int sc_launch_nodes(const ScArgs& a, int maxd_bucket, int W, int E, hipStream_t s) {
  if (W < 1 || W > kNodesMaxWaves) return fail(SCG_ERR_INVALID, "node-parallel kernel: %d waves per block", W);
  const int v = (a.obs_f64 ? 1 : 0) | (a.led_v && a.ledp_v ? 2 : 0);
  int rc = SCG_OK;
  const bool found = sc_dispatch_maxd<8>(maxd_bucket, [&](auto d) {
    constexpr int D = decltype(d)::value;
    switch (v) {
      case 0: rc = sc_launch_nodes_d<D, false, false>(a, W, E, s); break;
      case 1: rc = sc_launch_nodes_d<D, true, false>(a, W, E, s); break;
      case 2: rc = sc_launch_nodes_d<D, false, true>(a, W, E, s); break;
      default: rc = sc_launch_nodes_d<D, true, true>(a, W, E, s); break;
    }
  });
  if (!found) return fail(SCG_ERR_INVALID, "node-parallel kernel: nodes ship to at most 8 destinations");
  return rc;
}

// K steps of every env in one launch (sc_rollout_nodes_kernel): the batch kernel's block, LDS
// and persistent grid. a.t / a.episode / a.flags describe the launch's first step; obs_mode as
// the kernel's. No ledgers.
template <int MAXD, bool F64>
int sc_launch_nodes_rollout_d(const ScArgs& a, int W, int E, int K, int obs_mode, hipStream_t s) {
  const size_t lds = sc_nodes_lds_bytes(a.c.n_nodes, a.c.P, a.c.H, E, W, a.c.A, a.c.O, F64 ? 8 : 4);
  if (lds > sc_nodes_lds_max()) return fail(SCG_ERR_INVALID, "node-parallel rollout: %zu B of LDS per block", lds);
  int dev = 0;
  if (!sc_nodes_allow_lds<&sc_rollout_nodes_kernel<MAXD, F64>>(lds, sc_nodes_lds_max() - kNodesStaticLds, dev))
    return fail(SCG_ERR_HIP, "node-parallel rollout: cannot raise its LDS limit");
  const int64_t tiles = (a.n + 63) / 64;
  int64_t blocks = tiles;
  const int64_t resident = sc_nodes_resident_blocks<&sc_rollout_nodes_kernel<MAXD, F64>>(dev, W, lds);
  if (resident > 0 && resident < tiles) blocks = resident;
  const int cap = g_nodes_max_blocks.load(std::memory_order_relaxed);
  if (cap > 0 && cap < blocks) blocks = cap;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(sc_rollout_nodes_kernel<MAXD, F64>), dim3(static_cast<unsigned>(blocks)),
                     dim3(64 * W), lds, s, a, W, E, K, obs_mode);
  return check_launch("sc_rollout_nodes_kernel");
}

int sc_launch_nodes_rollout(const ScArgs& a, int maxd_bucket, int W, int E, int K, int obs_mode, hipStream_t s) {
  if (W < 1 || W > kNodesMaxWaves) return fail(SCG_ERR_INVALID, "node-parallel rollout: %d waves per block", W);
  if (a.led_v) return fail(SCG_ERR_INVALID, "node-parallel rollout: no ledgers");
  if (K < 1 || obs_mode < 0 || obs_mode > 2) return fail(SCG_ERR_INVALID, "node-parallel rollout: steps / observation mode");
  int rc = SCG_OK;
  const bool found = sc_dispatch_maxd<8>(maxd_bucket, [&](auto d) {
    constexpr int D = decltype(d)::value;
    rc = a.obs_f64 ? sc_launch_nodes_rollout_d<D, true>(a, W, E, K, obs_mode, s)
                   : sc_launch_nodes_rollout_d<D, false>(a, W, E, K, obs_mode, s);
  });
  if (!found) return fail(SCG_ERR_INVALID, "node-parallel rollout: nodes ship to at most 8 destinations");
  return rc;
}

// K closed-loop steps of every env in one launch (sc_closed_rollout_nodes_kernel of the launch's
// type): the rollout's block, LDS, persistent grid and block cap. a.act is unused; a.obs and
// a.rew may be null (outputs nobody asked for).
template <int MAXD, bool F64, class Launch>
int sc_launch_nodes_closed_d(const ScArgs& a, const Launch& p, int W, int E, int K, hipStream_t s) {
  constexpr auto kKernel = &sc_closed_rollout_nodes_kernel<MAXD, F64, Launch>;
  const size_t lds = sc_nodes_lds_bytes(a.c.n_nodes, a.c.P, a.c.H, E, W, a.c.A, a.c.O, F64 ? 8 : 4);
  if (lds > sc_nodes_lds_max()) return fail(SCG_ERR_INVALID, "closed-loop rollout: %zu B of LDS per block", lds);
  int dev = 0;
  if (!sc_nodes_allow_lds<kKernel>(lds, sc_nodes_lds_max() - kNodesStaticLds, dev))
    return fail(SCG_ERR_HIP, "closed-loop rollout: cannot raise its LDS limit");
  const int64_t tiles = (a.n + 63) / 64;
  int64_t blocks = tiles;
  const int64_t resident = sc_nodes_resident_blocks<kKernel>(dev, W, lds);
  if (resident > 0 && resident < tiles) blocks = resident;
  const int cap = g_nodes_max_blocks.load(std::memory_order_relaxed);
  if (cap > 0 && cap < blocks) blocks = cap;
  hipLaunchKernelGGL(kKernel, dim3(static_cast<unsigned>(blocks)), dim3(64 * W), lds, s, ScClosedKArgs<Launch>{a, p}, W, E, K);
  // the error says which policy, and whether sampled
  if constexpr (Launch::kDrawn)
    return check_launch(Launch::kMlp ? "sc_closed_rollout_nodes_kernel (mlp, drawn)" : "sc_closed_rollout_nodes_kernel (linear, drawn)");
  return check_launch(Launch::kMlp ? (Launch::kSampled ? "sc_closed_rollout_nodes_kernel (mlp, sampled)"
                                                       : "sc_closed_rollout_nodes_kernel (mlp)")
                                   : (Launch::kSampled ? "sc_closed_rollout_nodes_kernel (linear, sampled)"
                                                       : "sc_closed_rollout_nodes_kernel (linear)"));
}

// (scg_sc_nodes_launch.h.) The MLP's hidden tile lies over the inbox values and cost rows of the
// block's LDS (sc_nodes_tile): a wider one would run into the stocks behind them.
template <class Launch>
int sc_launch_nodes_closed(const ScArgs& a, const Launch& p, int maxd_bucket, int W, int E, int K, hipStream_t s) {
  if constexpr (Launch::kDrawn) {
    if (!p.drw.std) return fail(SCG_ERR_INVALID, "drawn closed-loop rollout: std is required");
  } else if constexpr (Launch::kSampled) {
    if (!p.smp.std || !p.smp.noise) return fail(SCG_ERR_INVALID, "sampled closed-loop rollout: std and noise are required");
  }
  if constexpr (Launch::kMlp)
    if (p.pv.H < 1 || p.pv.H > sc_mlp_fused_hidden_max(E, a.c.n_nodes))
      return fail(SCG_ERR_INVALID, "closed-loop rollout: %d hidden units do not fit the block's idle LDS", p.pv.H);
  if (W < 1 || W > kNodesMaxWaves) return fail(SCG_ERR_INVALID, "closed-loop rollout: %d waves per block", W);
  if (a.led_v) return fail(SCG_ERR_INVALID, "closed-loop rollout: no ledgers");
  if (K < 1) return fail(SCG_ERR_INVALID, "closed-loop rollout: steps");
  int rc = SCG_OK;
  const bool found = sc_dispatch_maxd<8>(maxd_bucket, [&](auto d) {
    constexpr int D = decltype(d)::value;
    rc = a.obs_f64 ? sc_launch_nodes_closed_d<D, true>(a, p, W, E, K, s) : sc_launch_nodes_closed_d<D, false>(a, p, W, E, K, s);
  });
  if (!found) return fail(SCG_ERR_INVALID, "closed-loop rollout: nodes ship to at most 8 destinations");
  return rc;
}
template int sc_launch_nodes_closed(const ScArgs&, const ScClosedLaunch<ScPolicyView>&, int, int, int, int, hipStream_t);
template int sc_launch_nodes_closed(const ScArgs&, const ScClosedLaunch<ScMlpView>&, int, int, int, int, hipStream_t);
template int sc_launch_nodes_closed(const ScArgs&, const ScSampledLaunch<ScPolicyView>&, int, int, int, int, hipStream_t);
template int sc_launch_nodes_closed(const ScArgs&, const ScSampledLaunch<ScMlpView>&, int, int, int, int, hipStream_t);
template int sc_launch_nodes_closed(const ScArgs&, const ScDrawnLaunch<ScPolicyView>&, int, int, int, int, hipStream_t);
template int sc_launch_nodes_closed(const ScArgs&, const ScDrawnLaunch<ScMlpView>&, int, int, int, int, hipStream_t);

// The step server's block for a config the batch kernel runs (float64 observations, no
// ledgers): one block of W waves with the batch kernel's LDS.
int sc_launch_nodes_server(const ScArgs& a, int maxd_bucket, int W, int E, hipStream_t s, scg_sc_server_box* box,
                           uint32_t exit_seen, uint32_t idle_ticks) {
  if (W < 1 || W > kNodesMaxWaves) return fail(SCG_ERR_INVALID, "node-parallel server: %d waves per block", W);
  if (!a.obs_f64 || a.led_v) return fail(SCG_ERR_INVALID, "the SupplyChain step server runs float64 observations, no ledgers");
  const size_t lds = sc_nodes_lds_bytes(a.c.n_nodes, a.c.P, a.c.H, E, W, a.c.A, a.c.O, 8);
  const size_t cap = sc_nodes_lds_max() - kNodesStaticLds - 1024;  // room for the static request words and action row
  if (lds > cap) return fail(SCG_ERR_INVALID, "node-parallel server: %zu B of LDS per block", lds);
  bool raised = true;
  const bool found = sc_dispatch_maxd<8>(maxd_bucket, [&](auto d) {
    constexpr int D = decltype(d)::value;
    int dev = 0;
    raised = sc_nodes_allow_lds<&sc_nodes_server_kernel<D>>(lds, cap, dev);
    if (raised)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(sc_nodes_server_kernel<D>), dim3(1), dim3(64 * W), lds, s, a, W, E, box,
                         exit_seen, idle_ticks);
  });
  if (!found) return fail(SCG_ERR_INVALID, "node-parallel server: nodes ship to at most 8 destinations");
  if (!raised) return fail(SCG_ERR_HIP, "node-parallel server: cannot raise its LDS limit");
  return check_launch("sc_nodes_server_kernel");
}

}  // namespace scg

extern "C" __attribute__((visibility("default"))) int scg_sc_nodes_max_blocks(int32_t blocks) {
  return scg::g_nodes_max_blocks.exchange(blocks < 0 ? 0 : blocks);
}

#ifdef SCG_NODES_STAMPS
// Diagnostic build only: copy the stamps of the first `waves` waves to host memory.
extern "C" __attribute__((visibility("default"))) int scg_nodes_debug_stamps(unsigned long long* host, int waves) {
  if (waves > kNStampWaves) waves = kNStampWaves;
  if (hipDeviceSynchronize() != hipSuccess) return scg::fail(SCG_ERR_HIP, "sync");
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_nodes_stamps), sizeof(unsigned long long) * kNStampSlots * waves) !=
      hipSuccess)
    return scg::fail(SCG_ERR_HIP, "stamp copy");
  return SCG_OK;
}

// Diagnostic build only: the step server's per-wave phase sums (g_srv_phases) to host memory
// (8 x 10 words), on a stream of its own, without waiting for the resident server block;
// reset != 0 clears them afterwards.
extern "C" __attribute__((visibility("default"))) int scg_sc_server_debug_phases(unsigned long long* host, int reset) {
  (void)hipGetLastError();  // an error an earlier call left behind is not this probe's
  static unsigned long long* pinned = nullptr;
  if (!pinned && hipHostMalloc(reinterpret_cast<void**>(&pinned), sizeof(scg::g_srv_phases), 0) != hipSuccess)
    return scg::fail(SCG_ERR_HIP, "phase probe: pinned buffer");
  void* dev = nullptr;
  if (hipGetSymbolAddress(&dev, HIP_SYMBOL(scg::g_srv_phases)) != hipSuccess) return scg::fail(SCG_ERR_HIP, "symbol");
  hipStream_t s;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return scg::fail(SCG_ERR_HIP, "stream");
  int rc = SCG_OK;
  hipError_t e = hipMemcpyAsync(pinned, dev, sizeof(scg::g_srv_phases), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) rc = scg::fail(SCG_ERR_HIP, "phase copy: %s", hipGetErrorString(e));
  if (rc == SCG_OK) {
    std::memcpy(host, pinned, sizeof(scg::g_srv_phases));
    if (reset) {
      e = hipMemsetAsync(dev, 0, sizeof(scg::g_srv_phases), s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) rc = scg::fail(SCG_ERR_HIP, "phase reset: %s", hipGetErrorString(e));
    }
  }
  (void)hipStreamDestroy(s);
  return rc;
}
#endif
