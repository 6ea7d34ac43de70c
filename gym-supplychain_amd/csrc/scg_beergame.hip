// BeerGame hot path for gfx950: reset / step / rollout kernels + their C-ABI launchers.
//
// Reference: gym_supplychain/envs/beergame_env.py (BeerGameEnv), snapshot 2024-08-07.
// One lane owns one env for the whole launch; every per-env array is env-major [N][L]
// int32, so for the default L = 4 each state row is one 16-byte global_load_dwordx4 /
// global_store_dwordx4 per lane and a wavefront moves 1 KiB per instruction, fully
// coalesced. The path is HBM/launch bound integer work (≈35 int ops per env-step);
// there is no contraction, so no MFMA and no LDS tiling — see DESIGN.md.
//
// The reference keeps an absolute-week shipment table (beergame_env.py:46-52) that is
// never shifted (:73-74). Here it is a ring of R = max delay + 1 week slots; the host
// plan (scg_bg_prepare) decides per week whether the due slot holds deliveries and
// whether the scheduled slot is written fresh (store) or accumulated (read-modify-write),
// so the common constant-delay case moves exactly one due row in and one row out.

#include <cstdarg>
#include <cstdio>
#include <ctime>
#include <vector>

#include "scg_beergame_kernels.h"
#include "scg_server_host.h"

namespace scg {

// Philox draws for tests/benchmarks ------------------------------------------------------
__global__ __launch_bounds__(kBlock) void poisson_demand_kernel(const BgArgs a, int32_t weeks,
                                                                int32_t* __restrict__ out) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (n >= a.n) return;
  for (int32_t w = 1; w <= weeks; ++w) out[(int64_t)(w - 1) * a.n + n] = week_demand(a, n, w, a.episode);
}

__global__ __launch_bounds__(kBlock) void uniform_ints_kernel(uint32_t k0, uint32_t k1, int64_t env_offset,
                                                              int64_t n_envs, int32_t rows, int32_t width,
                                                              uint32_t tag, int32_t lo, uint32_t range,
                                                              int32_t* __restrict__ out) {
  const int64_t n = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (n >= n_envs) return;
  const uint32_t env = static_cast<uint32_t>(env_offset + n);
  const int32_t words = rows * width;
  for (int32_t j0 = 0; j0 < words; j0 += 4) {
    const scg::U4 r = scg::philox4x32_10(scg::U4{env, tag, static_cast<uint32_t>(j0 >> 2), SCG_STREAM_ACTION}, k0, k1);
    const uint32_t w4[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int32_t j = j0 + s;
      if (j < words) {
        const uint32_t v = static_cast<uint32_t>((static_cast<uint64_t>(w4[s]) * range) >> 32);
        const int32_t rrow = j / width, col = j - rrow * width;
        out[((int64_t)rrow * n_envs + n) * width + col] = lo + static_cast<int32_t>(v);
      }
    }
  }
}

// Fills the slab kernel's constants block: the scalars travel by value, the thresholds are
// copied on the device (0xffffffff past the table's end).
__global__ __launch_bounds__(64) void bg_slab_consts_kernel(BgSlabConst* __restrict__ dst, const BgSlabConst v) {
  const int q = threadIdx.x;
  if (q < kFastThr) dst->thr[q] = (v.pthr && q < v.pthr_len) ? v.pthr[q] : 0xffffffffu;
  if (q < SCG_BG_MAX_LEVELS) dst->init_inv[q] = v.init_inv[q];
  if (q != 63) return;
  dst->env_base = v.env_base;
  dst->pthr_len = v.pthr_len;
  dst->h = v.h;
  dst->b = v.b;
  dst->guard = v.guard;
  dst->demand_lo = v.demand_lo;
  dst->demand_hi = v.demand_hi;
  dst->ship_value = v.ship_value;
  dst->orders_value = v.orders_value;
  dst->init_slots = v.init_slots;
  dst->err_host = v.err_host;
  dst->demand_table = v.demand_table;
  dst->pthr = v.pthr;
}

// ---- host helpers: run-time dispatch on the level count ----------------------------------
// f(the launchers of level L), or the error for a level count outside the table.
template <class F>
int with_level(int L, F&& f) {
#define X(l) bg_launchers<l>,
  static const BgLaunchers* (*const kLevels[])() = {SCG_LEVEL_CASES(X)};
#undef X
  if (L < 1 || L > SCG_BG_MAX_LEVELS) return fail(SCG_ERR_INVALID, "levels=%d outside 1..%d", L, SCG_BG_MAX_LEVELS);
  return f(*kLevels[L - 1]());
}

// Word offsets of a state slab (scg_bg_slab_layout); the slab kernel derives the same ones
// from (N, L, R) and the wpack option bits.
int slab_layout(int L, int64_t N, int32_t R, int32_t T, bool history, int64_t* off) {
  const int64_t NL = N * L;
  if (NL % 4 != 0) return fail(SCG_ERR_INVALID, "slab layout needs n_envs * levels %% 4 == 0 (got %lld)", (long long)NL);
  if (R < 1 || R > static_cast<int32_t>(kSlabRingMax)) return fail(SCG_ERR_INVALID, "slab layout needs 1 <= ring_slots <= 127");
  off[SCG_SLAB_ERROR] = 0;
  for (int f = 0; f < 6; ++f) off[SCG_SLAB_INVENTORY + f] = kSlabHeader + f * NL;
  off[SCG_SLAB_RING] = kSlabHeader + 6 * NL;
  off[SCG_SLAB_EPISODE_RETURN] = kSlabHeader + (6 + R) * NL;
  off[SCG_SLAB_FINAL_RETURN] = off[SCG_SLAB_EPISODE_RETURN] + 2 * N;
  off[SCG_SLAB_HISTORY] = off[SCG_SLAB_FINAL_RETURN] + 2 * N;
  off[SCG_SLAB_TOTAL] = off[SCG_SLAB_HISTORY] + (history ? static_cast<int64_t>(T + 1) * NL : 0);
  return SCG_OK;
}

// The slab kernel runs when st->slab and st->step_consts are set, the slab's views are where
// the layout puts them and the rewards follow the observation rows in one allocation.
bool slab_ready(const scg_bg_config* cfg, const scg_bg_state* st, const int32_t* obs, const int32_t* reward,
                const int32_t* terminal_obs) {
  if (!st->slab || !st->step_consts || cfg->variant != 1) return false;
  int64_t off[SCG_SLAB_FIELDS];
  const bool hist = st->orders_history != nullptr;
  if (slab_layout(cfg->levels, st->n_envs, cfg->ring_slots, cfg->max_weeks, hist, off) != SCG_OK) return false;
  int32_t* b = st->slab;
  const bool ledgers = st->inventory_costs != nullptr, returns = st->episode_return != nullptr;
  return st->inventory == b + off[SCG_SLAB_INVENTORY] && st->backlog == b + off[SCG_SLAB_BACKLOG] &&
         st->orders_placed == b + off[SCG_SLAB_ORDERS] && st->shipments == b + off[SCG_SLAB_RING] &&
         (!ledgers || (st->inventory_costs == b + off[SCG_SLAB_INV_COSTS] &&
                       st->backlog_costs == b + off[SCG_SLAB_BACKLOG_COSTS])) &&
         ledgers == (st->backlog_costs != nullptr) &&
         (!returns || (reinterpret_cast<int32_t*>(st->episode_return) == b + off[SCG_SLAB_EPISODE_RETURN] &&
                       reinterpret_cast<int32_t*>(st->final_return) == b + off[SCG_SLAB_FINAL_RETURN])) &&
         (!hist || st->orders_history == b + off[SCG_SLAB_HISTORY]) &&
         st->error_flags == b + off[SCG_SLAB_ERROR] && reward == obs + st->n_envs * cfg->levels &&
         (!terminal_obs || terminal_obs == b + off[SCG_SLAB_TERMINAL_OBS]);
}

int check_state(const scg_bg_config* cfg, const scg_bg_state* st) {
  if (!cfg || !st) return fail(SCG_ERR_INVALID, "null config/state");
  if (!cfg->plan || cfg->ring_slots <= 0) return fail(SCG_ERR_INVALID, "config not prepared (call scg_bg_prepare)");
  if (st->n_envs <= 0) return fail(SCG_ERR_INVALID, "n_envs must be > 0");
  if (st->n_envs > INT32_MAX) return fail(SCG_ERR_INVALID, "n_envs must be <= %d per shard", INT32_MAX);
  if (st->env_offset < 0 || st->env_offset + st->n_envs > (int64_t(1) << 32))
    return fail(SCG_ERR_INVALID, "global env ids must fit in 32 bits");
  if (!st->inventory || !st->backlog || !st->orders_placed || !st->shipments)
    return fail(SCG_ERR_INVALID, "state buffers inventory/backlog/orders_placed/shipments are required");
  if (cfg->demand_mode == SCG_DEMAND_TABLE && !cfg->demand_table)
    return fail(SCG_ERR_INVALID, "TABLE demand mode needs demand_table");
  if (cfg->demand_mode == SCG_DEMAND_POISSON && !cfg->poisson_thresholds)
    return fail(SCG_ERR_INVALID, "POISSON demand mode needs poisson_thresholds");
  return SCG_OK;
}

// Weeks 1..init_slots hold the initial pipeline (beergame_env.py:52); the ring keeps those
// within the horizon, a full table all of them.
inline int32_t init_slots(const scg_bg_config* cfg) {
  const int32_t d0 = cfg->shipment_delays ? cfg->shipment_delays[0] : 0;
  return cfg->full_table ? d0 : std::min(d0, cfg->max_weeks);
}

// The launch constants BgArgs and BgSlabConst both carry, under the same names.
template <class Consts>
void fill_shared_consts(Consts& c, const scg_bg_config* cfg, const scg_bg_state* st) {
  c.h = cfg->inv_cost;
  c.b = cfg->backlog_cost;
  c.guard = week_guard(cfg->levels, cfg->inv_cost, cfg->backlog_cost);
  c.demand_lo = cfg->demand_lo;
  c.demand_hi = cfg->demand_hi;
  c.ship_value = cfg->initial_shipment_value;
  c.orders_value = cfg->initial_orders_value;
  c.init_slots = init_slots(cfg);
  c.err_host = st->error_host;
  c.demand_table = cfg->demand_table;
  for (int l = 0; l < cfg->levels; ++l) c.init_inv[l] = cfg->initial_inventory[l];
}

BgArgs make_args(const scg_bg_config* cfg, const scg_bg_state* st) {
  BgArgs a;
  std::memset(&a, 0, sizeof(a));
  fill_shared_consts(a, cfg, st);
  a.inv = st->inventory;
  a.bk = st->backlog;
  a.op = st->orders_placed;
  a.ring = st->shipments;
  a.inv_acc = st->inventory_costs;
  a.bk_acc = st->backlog_costs;
  a.hist = st->orders_history;
  a.ep_ret = st->episode_return;
  a.final_ret = st->final_return;
  a.pthr = cfg->poisson_thresholds;
  a.n = st->n_envs;
  a.env_offset = st->env_offset;
  a.key0 = static_cast<uint32_t>(st->seed & 0xffffffffu);
  a.key1 = static_cast<uint32_t>(st->seed >> 32);
  a.episode = st->episode;
  a.demand_mode = cfg->demand_mode;
  a.pthr_len = cfg->poisson_len;
  a.ring_slots = cfg->ring_slots;
  a.max_weeks = cfg->max_weeks;
  a.err = st->error_flags;
  if (cfg->variant == 2) {
    a.pen_acc = st->penalty_costs;
    a.max_stock = cfg->max_stock;
    a.penalty = cfg->exceeded_capacity_penalty;
    a.stochastic_delays = cfg->stochastic_delays;
    a.delay_lo = cfg->delay_lo;
    a.delay_hi = cfg->delay_hi;
  }
  return a;
}

inline dim3 grid_for(int64_t n) { return dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)); }

// What the slab kernel's constants block holds for (cfg, st): every scalar, and the
// thresholds by pointer and length (the fill kernel copies them on the device).
BgSlabConst slab_consts(const scg_bg_config* cfg, const scg_bg_state* st) {
  BgSlabConst v;
  std::memset(&v, 0, sizeof(v));
  fill_shared_consts(v, cfg, st);
  v.env_base = static_cast<uint32_t>(st->env_offset);
  v.pthr_len = cfg->demand_mode == SCG_DEMAND_POISSON ? cfg->poisson_len : 0;
  v.pthr = cfg->demand_mode == SCG_DEMAND_POISSON ? cfg->poisson_thresholds : nullptr;
  return v;
}

// Fingerprint of a block's contents and address (never 0: 0 is "nothing uploaded").
uint64_t slab_consts_tag(const BgSlabConst& v, const void* block) {
  static_assert(offsetof(BgSlabConst, thr) % 8 == 0, "hashed as 64-bit words");
  uint64_t w[offsetof(BgSlabConst, thr) / 8];
  std::memcpy(w, &v, sizeof(w));
  uint64_t h = 0x9E3779B97F4A7C15ull ^ reinterpret_cast<uintptr_t>(block);
  for (uint64_t x : w) {
    h = (h ^ x) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 29;
  }
  return h | 1u;
}

// Uploads the block, in stream order ahead of the step, when it does not hold what this
// step needs (first step, or cfg / st edited since).
int sync_slab_consts(const scg_bg_config* cfg, scg_bg_state* st, hipStream_t s) {
  const BgSlabConst v = slab_consts(cfg, st);
  const uint64_t tag = slab_consts_tag(v, st->step_consts);
  if (tag == st->step_consts_tag) return SCG_OK;
  if (reinterpret_cast<uintptr_t>(st->step_consts) % alignof(BgSlabConst) != 0)
    return fail(SCG_ERR_INVALID, "step_consts must be %d-byte aligned", static_cast<int>(alignof(BgSlabConst)));
  hipLaunchKernelGGL(bg_slab_consts_kernel, dim3(1), dim3(64), 0, s, static_cast<BgSlabConst*>(st->step_consts), v);
  if (int rc = check_launch("bg_slab_consts_kernel")) return rc;
  st->step_consts_tag = tag;
  return SCG_OK;
}

}  // namespace scg

using namespace scg;

// ========================================================================================
extern "C" {

int scg_bg_struct_sizes(size_t* config_size, size_t* state_size) {
  if (config_size) *config_size = sizeof(scg_bg_config);
  if (state_size) *state_size = sizeof(scg_bg_state);
  return SCG_OK;
}

int scg_poisson_table(double lam, uint32_t* out, int32_t cap) {
  if (!(lam >= 0.0) || std::isinf(lam)) return -fail(SCG_ERR_INVALID, "poisson lambda must be finite and >= 0");
  if (!out || cap <= 0) return -fail(SCG_ERR_INVALID, "null/empty threshold buffer");
  double p = std::exp(-lam);
  double c = p;
  for (int32_t k = 0; k < cap; ++k) {
    const double t = c * 4294967296.0;
    const uint32_t v = t >= 4294967295.0 ? 0xffffffffu : static_cast<uint32_t>(t);
    out[k] = v;
    if (v == 0xffffffffu) return k + 1;
    p = p * lam / static_cast<double>(k + 1);
    c = c + p;
  }
  return -fail(SCG_ERR_INVALID, "poisson lambda %g needs more than %d thresholds", lam, cap);
}

int scg_bg_prepare(scg_bg_config* cfg) {
  if (!cfg) return fail(SCG_ERR_INVALID, "null config");
  const int32_t L = cfg->levels, T = cfg->max_weeks;
  if (L < 1 || L > SCG_BG_MAX_LEVELS) return fail(SCG_ERR_INVALID, "levels=%d outside 1..%d", L, SCG_BG_MAX_LEVELS);
  if (T < 1 || T > SCG_BG_MAX_WEEKS) return fail(SCG_ERR_INVALID, "max_weeks=%d outside 1..%d", T, SCG_BG_MAX_WEEKS);
  if (!cfg->shipment_delays || !cfg->plan) return fail(SCG_ERR_INVALID, "shipment_delays and plan are required");
  if (cfg->variant == 0) cfg->variant = 1;
  if (cfg->variant != 1 && cfg->variant != 2) return fail(SCG_ERR_INVALID, "variant must be 1 or 2");
  if (cfg->demand_mode < SCG_DEMAND_FIXED || cfg->demand_mode > SCG_DEMAND_UNIFORM)
    return fail(SCG_ERR_INVALID, "unknown demand_mode %d", cfg->demand_mode);
  if (cfg->demand_mode == SCG_DEMAND_UNIFORM && !(cfg->demand_hi > cfg->demand_lo))
    return fail(SCG_ERR_INVALID, "uniform demand needs demand_lo < demand_hi");
  if (cfg->variant == 1 && cfg->stochastic_delays)
    return fail(SCG_ERR_INVALID, "stochastic shipment delays are a BeerGameEnv2 option");
  if (cfg->demand_mode == SCG_DEMAND_FIXED && !cfg->customer_demand)
    return fail(SCG_ERR_INVALID, "FIXED demand mode needs customer_demand");
  if (cfg->demand_mode == SCG_DEMAND_POISSON && (cfg->poisson_len < 1 || cfg->poisson_len > SCG_POISSON_MAX))
    return fail(SCG_ERR_INVALID, "poisson_len=%d outside 1..%d", cfg->poisson_len, SCG_POISSON_MAX);
  int32_t max_delay = 0;
  for (int32_t w = 0; w <= T; ++w) {
    const int32_t d = cfg->shipment_delays[w];
    if (d < 0 || d > SCG_BG_MAX_DELAY)
      return fail(SCG_ERR_INVALID, "shipment_delays[%d]=%d outside 0..%d", w, d, SCG_BG_MAX_DELAY);
    max_delay = std::max(max_delay, d);
  }
  int32_t R = max_delay + 1;
  if (cfg->stochastic_delays) {  // per-lane randint(lo, hi) delays: ring covers hi - 1 and the initial 2
    if (cfg->delay_lo < 0 || cfg->delay_hi <= cfg->delay_lo || cfg->delay_hi > SCG_BG_MAX_DELAY + 1)
      return fail(SCG_ERR_INVALID, "stochastic delays need 0 <= delay_lo < delay_hi <= %d", SCG_BG_MAX_DELAY + 1);
    R = std::max(R, cfg->delay_hi);
  }
  const bool full = cfg->full_table != 0;
  if (full) {  // the reference's table: rows max(T+1, max_w(w+d_w+1)) + 1 (:46-50), slot s = week s
    if (cfg->variant != 1) return fail(SCG_ERR_INVALID, "full_table is a BeerGameEnv (variant 1) option");
    int32_t last = T + 1;
    for (int32_t w = 0; w <= T; ++w) last = std::max(last, w + cfg->shipment_delays[w] + 1);
    R = last + 1;  // <= T + SCG_BG_MAX_DELAY + 2: fits pack_week's slot fields
  }
  // Which arrival weeks have been written, in week order (writes only target later weeks).
  // (a full table also keeps the rows past T: week T + 1 + max delay at most)
  std::vector<uint8_t> written(static_cast<size_t>(T) + SCG_BG_MAX_DELAY + 2, 0);
  for (int32_t t = 1; t <= init_slots(cfg); ++t) written[t] = 1;  // initial pipeline (:52)
  cfg->plan[0] = 0;
  for (int32_t w = 1; w <= T; ++w) {
    const int32_t d = cfg->shipment_delays[w];
    int32_t mode;
    if (d == 0) {
      mode = MODE_DIRECT;                 // :93-94, :111-112
    } else if (w + d > T && !full) {
      mode = MODE_DROP;                   // lands after the last step: never received
    } else if (written[w + d]) {
      mode = MODE_ADD;                    // several weeks ship into one arrival week
    } else {
      mode = MODE_STORE;
      written[w + d] = 1;
    }
    cfg->plan[w] = plan_word(mode, written[w] != 0, d);
  }
  cfg->ring_slots = R;
  return SCG_OK;
}

int scg_bg_slab_layout(const scg_bg_config* cfg, int64_t n_envs, int32_t with_history,
                       int64_t offsets[SCG_SLAB_FIELDS]) {
  if (!cfg || !offsets) return fail(SCG_ERR_INVALID, "null config/offsets");
  if (cfg->ring_slots <= 0) return fail(SCG_ERR_INVALID, "config not prepared (call scg_bg_prepare)");
  if (n_envs <= 0 || n_envs > INT32_MAX) return fail(SCG_ERR_INVALID, "n_envs must be in 1..%d", INT32_MAX);
  return slab_layout(cfg->levels, n_envs, cfg->ring_slots, cfg->max_weeks, with_history != 0, offsets);
}

int scg_bg_reset(const scg_bg_config* cfg, scg_bg_state* st, int32_t* obs, void* stream) {
  if (int rc = check_state(cfg, st)) return rc;
  if (st->week >= 0) st->episode += 1;  // the previous episode (finished or not) is discarded
  BgArgs a = make_args(cfg, st);
  a.obs = obs;
  if (int rc = with_level(cfg->levels, [&](const BgLaunchers& k) {
        return k.reset(grid_for(st->n_envs), static_cast<hipStream_t>(stream), a);
      }))
    return rc;
  st->week = 0;
  return SCG_OK;
}

// Per-week launch info for week w of the current episode.
static scg::WeekInfo week_info(const scg_bg_config* cfg, int32_t w, uint32_t flags) {
  const int32_t p = cfg->plan[w];
  const int32_t R = cfg->ring_slots;
  WeekInfo wk;
  wk.week = w;
  wk.read_slot = plan_arrive(p) ? w % R : -1;
  wk.write_slot = (w + plan_delay(p)) % R;
  wk.mode = plan_mode(p);
  wk.demand_fixed = cfg->demand_mode == SCG_DEMAND_FIXED ? cfg->customer_demand[w - 1] : 0;
  const bool terminal = (w == cfg->max_weeks);
  wk.flags = (terminal ? WEEK_TERMINAL : 0) | ((terminal && (flags & SCG_BG_AUTORESET)) ? WEEK_AUTORESET : 0);
  return wk;
}

// The host's week and episode counters after week wk.
static void advance_week(scg_bg_state* st, const WeekInfo& wk) {
  if (wk.flags & WEEK_AUTORESET) {
    st->week = 0;
    st->episode += 1;
  } else {
    st->week = wk.week;
  }
}

static int check_step(const scg_bg_config* cfg, const scg_bg_state* st) {
  if (st->week < 0) return fail(SCG_ERR_NOT_RESET, "step() before reset()");
  if (st->week >= cfg->max_weeks)
    return fail(SCG_ERR_PAST_HORIZON, "step() after the terminal week %d (customer_demand has %d weeks)",
                cfg->max_weeks, cfg->max_weeks);
  return SCG_OK;
}

int scg_bg_step(const scg_bg_config* cfg, scg_bg_state* st, const int32_t* action, int32_t* obs,
                int32_t* reward, int32_t* terminal_obs, uint32_t flags, int32_t* done, void* stream) {
  return scg_bg_step_timed(cfg, st, action, obs, reward, terminal_obs, flags, done, nullptr, nullptr, stream);
}

int scg_bg_step_timed(const scg_bg_config* cfg, scg_bg_state* st, const int32_t* action, int32_t* obs,
                      int32_t* reward, int32_t* terminal_obs, uint32_t flags, int32_t* done, void* start_event,
                      void* stop_event, void* stream) {
  if (int rc = check_state(cfg, st)) return rc;
  if (!action || !obs || !reward) return fail(SCG_ERR_INVALID, "action/obs/reward buffers are required");
  if (int rc = check_step(cfg, st)) return rc;
  const int32_t w = st->week + 1;
  const WeekInfo wk = week_info(cfg, w, flags);
  const dim3 grid = grid_for(st->n_envs);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const hipEvent_t ev0 = static_cast<hipEvent_t>(start_event), ev1 = static_cast<hipEvent_t>(stop_event);
  if (slab_ready(cfg, st, obs, reward, terminal_obs)) {
    if (int rc = sync_slab_consts(cfg, st, s)) return rc;
    const uint32_t wpack = pack_week_slab(wk, cfg->ring_slots, st->inventory_costs != nullptr,  // R <= 127 (slab_layout)
                                          st->episode_return != nullptr, st->orders_history != nullptr);
    const SlabLaunch sl{st->slab, action, obs, static_cast<const BgSlabConst*>(st->step_consts), st->seed,
                        static_cast<uint32_t>(st->n_envs), wpack, static_cast<uint32_t>(w), st->episode,
                        wk.demand_fixed};
    if (int rc = with_level(cfg->levels, [&](const BgLaunchers& k) { return k.slab(cfg->demand_mode, grid, s, sl, ev0, ev1); }))
      return rc;
  } else {
    BgArgs a = make_args(cfg, st);
    a.act = action;
    a.obs = obs;
    a.rew = reward;
    a.term_obs = terminal_obs;
    if (int rc = with_level(cfg->levels, [&](const BgLaunchers& k) {
          return cfg->variant == 2 ? k.step2(grid, s, a, wk) : k.step(grid, s, a, wk, ev0, ev1);
        }))
      return rc;
  }
  advance_week(st, wk);
  if (done) *done = (wk.flags & WEEK_TERMINAL) ? 1 : 0;
  return SCG_OK;
}

// ---- step server (include/scgpu.h: scg_bg_server_*) -------------------------------------
// the layouts the Python binding (_native.py) mirrors
static_assert(sizeof(scg_bg_server_line) == 64, "request line");
static_assert(sizeof(scg_bg_server_box) == 17 * 64 + 64 + SCG_BG_SERVER_SLOTS * SCG_BG_SERVER_ARGS_BYTES, "mailbox");
static_assert(offsetof(scg_bg_server_box, done_seq) == 16 * 64 && offsetof(scg_bg_server_box, args) == 18 * 64,
              "mailbox lines");
static_assert(sizeof(scg_bg_server) == 72 && sizeof(scg_bg_server_slot) == 64, "server structs");
// The server's host bookkeeping (launch, retire, slots, argument blocks) under a spin lock in
// the struct itself: posts and waits of different slots may come from different threads.
struct ServerLock {
  int32_t* w;
  explicit ServerLock(scg_bg_server* sv) : w(&sv->lock) {
    for (;;) {
      int32_t z = 0;
      if (__atomic_compare_exchange_n(w, &z, 1, false, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED)) return;
      cpu_relax();
    }
  }
  ~ServerLock() { __atomic_store_n(w, 0, __ATOMIC_RELEASE); }
};

static bool server_ok(const scg_bg_server* sv) { return sv && sv->box_host && sv->box_dev; }

static const ServerNames kServerNames{"step server", "the wave's stream", "wave", "week"};

// Launch the wave (lock held). It serves, first, every slot whose request is newer than its answer.
static int server_launch_locked(scg_bg_server* sv) {
  return server_launch(sv, [sv](uint32_t exit_seen, uint32_t idle_ticks) {
    return with_level(sv->levels, [&](const BgLaunchers& k) {
      return k.server(static_cast<hipStream_t>(sv->stream), sv->demand_mode, sv->box_dev, exit_seen, idle_ticks);
    });
  });
}

static int server_stop_locked(scg_bg_server* sv) {
  return server_retire(sv, [sv] { return stream_wait(sv->stream); }, kServerNames.who);
}

// The wave polls slots 0 .. n_slots - 1: up to the highest attached one (lock held).
static void server_publish_n_slots(scg_bg_server* sv) {
  uint32_t ns = 0;
  for (int j = 0; j < kServerSlots; ++j)
    if (sv->slots_used >> j & 1u) ns = j + 1;
  __atomic_store_n(&sv->box_host->n_slots, ns, __ATOMIC_RELEASE);
}

int scg_bg_server_stop(scg_bg_server* sv) {
  if (!server_ok(sv)) return fail(SCG_ERR_INVALID, "null server/mailbox");
  ServerLock lk(sv);
  return server_stop_locked(sv);
}

uint32_t scg_bg_server_line_check(const scg_bg_server_line* line) {
  uint32_t w[16];
  std::memcpy(w, line, sizeof(w));
  return server_line_check(w);
}

int scg_bg_server_attach(scg_bg_server* sv, scg_bg_server_slot* slot) {
  if (!server_ok(sv) || !slot) return fail(SCG_ERR_INVALID, "null server/mailbox/slot");
  if (!slot->action || !slot->obs || !slot->reward) return fail(SCG_ERR_INVALID, "step server: slot action, obs and reward are required");
  if (!sv->stream) return fail(SCG_ERR_INVALID, "step server: needs a (non-blocking) stream of its own, not the null stream");
  if (sv->levels < 1 || sv->levels > SCG_BG_MAX_LEVELS) return fail(SCG_ERR_INVALID, "step server: levels=%d", sv->levels);
  if (sv->demand_mode < SCG_DEMAND_FIXED || sv->demand_mode > SCG_DEMAND_UNIFORM)
    return fail(SCG_ERR_INVALID, "step server: unknown demand_mode %d", sv->demand_mode);
  if (sv->idle_us < 100 || sv->idle_us > 10000000) return fail(SCG_ERR_INVALID, "idle_us outside 100..10^7");
  ServerLock lk(sv);
  int k = 0;
  while (k < kServerSlots && (sv->slots_used >> k & 1u)) ++k;
  if (k == kServerSlots) return fail(SCG_ERR_INVALID, "step server: all %d slots are taken", kServerSlots);
  scg_bg_server_box* b = sv->box_host;
  sv->slots_used |= 1u << k;
  slot->server = sv;
  slot->index = k;
  // a slot taken again continues its line's numbering; its arguments are published on the
  // first post (cleared here, they differ from any real ones: a new generation)
  slot->seq = __atomic_load_n(&b->req[k].req_seq, __ATOMIC_RELAXED);
  slot->gen = b->req[k].gen;
  std::memset(b->args[k], 0, sizeof(b->args[k]));
  slot->week = 0;
  slot->done = 0;
  slot->relaunches = 0;
  __atomic_store_n(&b->done_seq[k], slot->seq, __ATOMIC_RELEASE);
  server_publish_n_slots(sv);
  return SCG_OK;
}

int scg_bg_server_detach(scg_bg_server_slot* slot) {
  if (!slot || !server_ok(slot->server)) return fail(SCG_ERR_INVALID, "null slot or server");
  scg_bg_server* sv = slot->server;
  if (slot->index < 0) return SCG_OK;
  scg_bg_server_box* b = sv->box_host;
  const int k = slot->index;
  if (__atomic_load_n(&b->done_seq[k], __ATOMIC_ACQUIRE) != slot->seq)
    return fail(SCG_ERR_INVALID, "step server: detach with a request of slot %d unanswered", k);
  ServerLock lk(sv);
  sv->slots_used &= ~(1u << k);
  server_publish_n_slots(sv);
  slot->index = -1;
  return SCG_OK;
}

int scg_bg_server_post(const scg_bg_config* cfg, scg_bg_state* st, scg_bg_server_slot* slot) {
  if (int rc = check_state(cfg, st)) return rc;
  if (!slot || !server_ok(slot->server) || slot->index < 0 || slot->index >= kServerSlots)
    return fail(SCG_ERR_INVALID, "step server: the slot is not attached");
  scg_bg_server* sv = slot->server;
  if (st->n_envs > kServerBlock) return fail(SCG_ERR_INVALID, "the step server runs up to %d envs per slot", kServerBlock);
  if (cfg->variant != 1) return fail(SCG_ERR_INVALID, "the step server runs BeerGameEnv (variant 1)");
  if (st->slab) return fail(SCG_ERR_INVALID, "the step server runs on separate state buffers (no slab)");
  if (cfg->levels != sv->levels || cfg->demand_mode != sv->demand_mode)
    return fail(SCG_ERR_INVALID, "step server: the config (levels %d, demand mode %d) is not the server's (%d, %d)",
                cfg->levels, cfg->demand_mode, sv->levels, sv->demand_mode);
  if (int rc = check_step(cfg, st)) return rc;
  scg_bg_server_box* b = sv->box_host;
  const int k = slot->index;
  if (__atomic_load_n(&b->done_seq[k], __ATOMIC_ACQUIRE) != slot->seq)
    return fail(SCG_ERR_INVALID, "step server: slot %d posts while its last request is unanswered", k);
  const int32_t w = st->week + 1;
  const WeekInfo wk = week_info(cfg, w, 0);
  BgArgs a = make_args(cfg, st);
  a.act = slot->action;
  a.obs = slot->obs;
  a.rew = slot->reward;
  a.term_obs = nullptr;
  ServerLock lk(sv);
  // the slot's arguments: a new generation whenever they differ from the published ones (the
  // wave reloads them only then; nothing of the slot is in flight, so rewriting is safe)
  if (std::memcmp(b->args[k], &a, sizeof(a)) != 0) {
    std::memcpy(b->args[k], &a, sizeof(a));
    slot->gen = slot->gen + 1 ? slot->gen + 1 : 1;  // 0 is the wave's "none loaded"
  }
  // a wave idle for more than half its time-out may be exiting: retire it before posting
  if (server_stale(sv, mono_ns()))
    if (int rc = server_stop_locked(sv)) return rc;
  uint32_t line[16] = {0};
  const uint32_t seq = slot->seq + 1;
  const int32_t n_inline = (slot->action_host && st->n_envs == 1 && cfg->levels <= 8) ? cfg->levels : 0;
  line[0] = seq;
  line[2] = pack_week(wk);
  line[3] = static_cast<uint32_t>(w);
  line[4] = static_cast<uint32_t>(wk.demand_fixed);
  line[5] = static_cast<uint32_t>(n_inline);
  line[6] = slot->gen;
  for (int l = 0; l < n_inline; ++l) line[8 + l] = static_cast<uint32_t>(slot->action_host[l]);
  line[7] = server_line_check(line);
  server_publish(reinterpret_cast<uint32_t*>(&b->req[k]), line);
  slot->seq = seq;
  slot->week = w;
  slot->done = (wk.flags & WEEK_TERMINAL) ? 1 : 0;
  sv->last_ns = mono_ns();
  if (!sv->running)
    if (int rc = server_launch_locked(sv)) return rc;
  return SCG_OK;
}

int scg_bg_server_wait(scg_bg_state* st, scg_bg_server_slot* slot, int64_t spin_us, int32_t* done) {
  if (!st || !slot || !server_ok(slot->server) || slot->index < 0 || slot->index >= kServerSlots)
    return fail(SCG_ERR_INVALID, "step server: the slot is not attached");
  scg_bg_server* sv = slot->server;
  if (int rc = server_await<ServerLock>(
          sv, &sv->box_host->done_seq[slot->index], slot->seq, spin_us, &slot->relaunches,
          [sv](const char** text) { return stream_state(sv->stream, text); },
          [sv] { return server_launch_locked(sv); }, kServerNames, slot->week))
    return rc;  // SCG_PENDING or an error
  st->week = slot->week;  // no auto-reset on this path
  if (done) *done = slot->done;
  return SCG_OK;
}

int scg_bg_server_step(const scg_bg_config* cfg, scg_bg_state* st, scg_bg_server_slot* slot, int32_t* done) {
  if (int rc = scg_bg_server_post(cfg, st, slot)) return rc;
  return scg_bg_server_wait(st, slot, -1, done);
}

// ---- rollouts ---------------------------------------------------------------------------
static int check_horizon(const scg_bg_config* cfg, const scg_bg_state* st, int32_t n_weeks, uint32_t flags) {
  if (!(flags & SCG_BG_AUTORESET) && st->week + static_cast<int64_t>(n_weeks) > cfg->max_weeks)
    return fail(SCG_ERR_PAST_HORIZON, "rollout of %d weeks from week %d passes the terminal week %d", n_weeks,
                st->week, cfg->max_weeks);
  return SCG_OK;
}

// A call of n_weeks as launches of up to SCG_BG_ROLLOUT_MAX weeks: launch(done_k, K, args, weeks)
// runs weeks done_k .. done_k + K of the call; the state's week and episode follow each launch.
extern "C++" {
template <class Launch>
static int rollout_launches(const scg_bg_config* cfg, scg_bg_state* st, int32_t n_weeks, uint32_t flags,
                            Launch&& launch) {
  int32_t done_k = 0;
  while (done_k < n_weeks) {
    RolloutWeeks weeks;
    int32_t K = 0;
    scg_bg_state probe = *st;
    const BgArgs a = make_args(cfg, st);
    while (K < SCG_BG_ROLLOUT_MAX && done_k + K < n_weeks) {
      weeks.wk[K] = week_info(cfg, probe.week + 1, flags);
      advance_week(&probe, weeks.wk[K]);
      ++K;
    }
    if (int rc = launch(done_k, K, a, weeks)) return rc;
    st->week = probe.week;
    st->episode = probe.episode;
    done_k += K;
  }
  return SCG_OK;
}
}  // extern "C++"

int scg_bg_rollout(const scg_bg_config* cfg, scg_bg_state* st, int32_t n_weeks, const int32_t* actions,
                   int32_t* obs, int32_t* rewards, uint32_t flags, void* stream) {
  if (int rc = check_state(cfg, st)) return rc;
  if (!actions || n_weeks < 0) return fail(SCG_ERR_INVALID, "rollout needs actions and n_weeks >= 0");
  if (int rc = check_step(cfg, st)) return rc;
  if (int rc = check_horizon(cfg, st, n_weeks, flags)) return rc;
  const int64_t stride = st->n_envs * cfg->levels;
  return rollout_launches(cfg, st, n_weeks, flags, [&](int32_t done_k, int32_t K, const BgArgs& a, const RolloutWeeks& weeks) {
    const RolloutActs src{actions + done_k * stride, obs ? obs + done_k * stride : nullptr,
                          rewards ? rewards + done_k * st->n_envs : nullptr};
    return with_level(cfg->levels, [&](const BgLaunchers& k) {
      return k.rollout(cfg->variant, grid_for(st->n_envs), static_cast<hipStream_t>(stream), a, K, weeks, src);
    });
  });
}

// ---- the closed loop: scg_bg_rollout_policy, _local, _mlp and _drawn -----------------------
// What the in-transit sum needs of a config: every delay within the 64-bit live mask, and the
// ring (a full table keeps rows past T, which would need a different rule).
static int check_local_config(const scg_bg_config* cfg) {
  if (cfg->levels > SCG_BG_POLICY_MAX_LEVELS)
    return fail(SCG_ERR_INVALID, "local policy: levels=%d above %d", cfg->levels, SCG_BG_POLICY_MAX_LEVELS);
  if (cfg->full_table) return fail(SCG_ERR_INVALID, "local policy: full_table configs are not supported");
  for (int32_t w = 0; w <= cfg->max_weeks; ++w)
    if (cfg->shipment_delays[w] > kLocalMaxDelay)
      return fail(SCG_ERR_INVALID, "local policy: shipment_delays[%d]=%d above SCG_BG_LOCAL_MAX_DELAY=%d", w,
                  cfg->shipment_delays[w], kLocalMaxDelay);
  if (cfg->stochastic_delays && cfg->delay_hi - 1 > kLocalMaxDelay)
    return fail(SCG_ERR_INVALID, "local policy: stochastic delays up to delay_hi-1=%d above SCG_BG_LOCAL_MAX_DELAY=%d",
                cfg->delay_hi - 1, kLocalMaxDelay);
  return SCG_OK;
}

// The live mask of the state after week w0, and the FIXED demand of that week.
static uint64_t local_mask(const scg_bg_config* cfg, int32_t w0) {
  return cfg->stochastic_delays ? local_live_mask_stochastic(cfg->ring_slots, cfg->max_weeks, w0)
                                : local_live_mask(cfg->shipment_delays, cfg->max_weeks, w0);
}
static int32_t local_last_fixed(const scg_bg_config* cfg, int32_t w0) {
  return (cfg->demand_mode == SCG_DEMAND_FIXED && w0 >= 1) ? cfg->customer_demand[w0 - 1] : 0;
}

// The one host path of the four entry points. `who` names the policy in the messages; validate()
// checks what is particular to the policy struct; fill(src, done, done_k) sets what is particular to
// the source, for the launch that starts at week done_k of the call, `done` action words into the
// call's per-week buffers. The order of the checks is behaviour (tests/test_bg_closed_abi.py).
extern "C++" {
template <class Source, class Policy, class Validate, class Fill>
static int closed_rollout(const char* who, int32_t kind, const scg_bg_config* cfg, scg_bg_state* st, int32_t n_weeks,
                          const Policy* policy, int32_t* actions_out, int32_t* obs, int32_t* rewards, int64_t* reward_sum,
                          uint32_t flags, void* stream, Validate&& validate, Fill&& fill) {
  if (int rc = check_state(cfg, st)) return rc;
  if (!policy || !policy->params) return fail(SCG_ERR_INVALID, "%s rollout needs a policy with params", who);
  if (policy->kind != kind) return fail(SCG_ERR_INVALID, "unknown %s kind %d", who, policy->kind);
  if (int rc = validate()) return rc;
  if constexpr (Source::kLocal) {
    if (int rc = check_local_config(cfg)) return rc;
  } else if (cfg->levels > SCG_BG_POLICY_MAX_LEVELS) {
    return fail(SCG_ERR_INVALID, "%s rollout: levels=%d above %d", who, cfg->levels, SCG_BG_POLICY_MAX_LEVELS);
  }
  if (n_weeks < 0) return fail(SCG_ERR_INVALID, "%s rollout needs n_weeks >= 0", who);
  if (int rc = check_step(cfg, st)) return rc;
  if (int rc = check_horizon(cfg, st, n_weeks, flags)) return rc;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_weeks == 0) {  // no launch: the sum of no rewards
    if (reward_sum && hipMemsetAsync(reward_sum, 0, static_cast<size_t>(st->n_envs) * sizeof(int64_t), s) != hipSuccess)
      return fail(SCG_ERR_HIP, "hipMemsetAsync(reward_sum) failed");
    return SCG_OK;
  }
  const int64_t stride = st->n_envs * cfg->levels;
  return rollout_launches(cfg, st, n_weeks, flags, [&](int32_t done_k, int32_t K, const BgArgs& a, const RolloutWeeks& weeks) {
    const int64_t done = done_k * stride;
    Source src;
    src.params = policy->params;
    src.acts_out = actions_out ? actions_out + done : nullptr;
    src.obs_out = obs ? obs + done : nullptr;
    src.rew_out = rewards ? rewards + done_k * st->n_envs : nullptr;
    src.reward_sum = reward_sum;
    src.first = done_k == 0;
    if constexpr (Source::kLocal)  // st->week: the state this launch starts from (weeks.wk[0].week - 1)
      src.start = LocalStart{local_last_fixed(cfg, st->week), local_mask(cfg, st->week)};
    fill(src, done, done_k);
    return bg_launch_closed(cfg->levels, cfg->variant, grid_for(st->n_envs), s, a, K, weeks, src);
  });
}

// The two integer policies: beside the parameters, the shift and the clamp.
template <class Source, class Policy>
static int int_policy_rollout(const char* who, int32_t kind, const scg_bg_config* cfg, scg_bg_state* st, int32_t n_weeks,
                              const Policy* p, int32_t* actions_out, int32_t* obs, int32_t* rewards, int64_t* reward_sum,
                              uint32_t flags, void* stream) {
  return closed_rollout<Source>(
      who, kind, cfg, st, n_weeks, p, actions_out, obs, rewards, reward_sum, flags, stream,
      [&]() -> int {
        if (clamp_valid(p->shift, p->act_lo, p->act_hi)) return SCG_OK;
        return fail(SCG_ERR_INVALID, "%s needs shift in 0..%d and act_lo <= act_hi (got shift=%d, clamp %d..%d)", who,
                    kPolicyMaxShift, p->shift, p->act_lo, p->act_hi);
      },
      [&](Source& src, int64_t, int32_t) { src.clamp = PolicyClamp{p->shift, p->act_lo, p->act_hi}; });
}
}  // extern "C++"

int scg_bg_rollout_policy(const scg_bg_config* cfg, scg_bg_state* st, int32_t n_weeks, const scg_bg_policy* policy,
                          int32_t* actions_out, int32_t* obs, int32_t* rewards, int64_t* reward_sum, uint32_t flags,
                          void* stream) {
  return int_policy_rollout<PolicyArgs>("policy", SCG_BG_POLICY_LINEAR, cfg, st, n_weeks, policy, actions_out, obs, rewards,
                                        reward_sum, flags, stream);
}

int scg_bg_rollout_local(const scg_bg_config* cfg, scg_bg_state* st, int32_t n_weeks, const scg_bg_local_policy* policy,
                         int32_t* actions_out, int32_t* obs, int32_t* rewards, int64_t* reward_sum, uint32_t flags,
                         void* stream) {
  return int_policy_rollout<LocalArgs>("local policy", SCG_BG_POLICY_LOCAL, cfg, st, n_weeks, policy, actions_out, obs,
                                       rewards, reward_sum, flags, stream);
}

int scg_bg_rollout_mlp(const scg_bg_config* cfg, scg_bg_state* st, int32_t n_weeks, const scg_bg_mlp* policy,
                       int32_t* actions_out, int32_t* obs, int32_t* rewards, int64_t* reward_sum, uint32_t flags,
                       void* stream) {
  return closed_rollout<MlpArgs>(
      "MLP policy", SCG_BG_POLICY_MLP, cfg, st, n_weeks, policy, actions_out, obs, rewards, reward_sum, flags, stream,
      [&]() -> int {
        if (!bg_mlp_valid(policy->kind, policy->hidden, policy->act_lo, policy->act_hi))
          return fail(SCG_ERR_INVALID,
                      "MLP policy needs hidden in 1..%d and -2^24 <= act_lo <= act_hi <= 2^24 (got hidden=%d, clamp %d..%d)",
                      kBgMlpMaxHidden, policy->hidden, policy->act_lo, policy->act_hi);
        if (!policy->noise != !policy->std) return fail(SCG_ERR_INVALID, "MLP policy: noise and std go together");
        if (policy->samples_out && !policy->noise) return fail(SCG_ERR_INVALID, "MLP policy: samples_out needs noise and std");
        return SCG_OK;
      },
      [&](MlpArgs& ma, int64_t done, int32_t) {
        ma.std = policy->std;
        ma.noise = policy->noise ? policy->noise + done : nullptr;
        ma.samples_out = policy->samples_out ? policy->samples_out + done : nullptr;
        ma.features_out = policy->features_out ? policy->features_out + done * kLocalFeatures : nullptr;
        ma.hidden = policy->hidden;
        ma.lo = policy->act_lo;
        ma.hi = policy->act_hi;
      });
}

// The sampled MLP loop with the noise computed by the lanes: the launch that starts at week done_k
// of the call gets first row row0 + done_k.
int scg_bg_rollout_drawn(const scg_bg_config* cfg, scg_bg_state* st, int32_t n_weeks, const scg_bg_mlp* policy,
                         const scg_bg_noise_draw* draw, int32_t* actions_out, int32_t* obs, int32_t* rewards,
                         int64_t* reward_sum, uint32_t flags, void* stream) {
  return closed_rollout<MlpDrawnArgs>(
      "MLP policy", SCG_BG_POLICY_MLP, cfg, st, n_weeks, policy, actions_out, obs, rewards, reward_sum, flags, stream,
      [&]() -> int {
        if (!bg_mlp_valid(policy->kind, policy->hidden, policy->act_lo, policy->act_hi))
          return fail(SCG_ERR_INVALID,
                      "MLP policy needs hidden in 1..%d and -2^24 <= act_lo <= act_hi <= 2^24 (got hidden=%d, clamp %d..%d)",
                      kBgMlpMaxHidden, policy->hidden, policy->act_lo, policy->act_hi);
        if (!draw) return fail(SCG_ERR_INVALID, "noise draw: null draw");
        if (draw->reserved != 0) return fail(SCG_ERR_INVALID, "noise draw: reserved must be 0");
        if (policy->noise) return fail(SCG_ERR_INVALID, "noise draw: the policy's noise must be NULL");
        if (n_weeks > 0 && !policy->std) return fail(SCG_ERR_INVALID, "noise draw: device std is required");
        if (n_weeks > 0 && static_cast<int64_t>(draw->row0) + n_weeks > (int64_t(1) << 32))
          return fail(SCG_ERR_INVALID, "noise draw: rows %u + %d pass 2^32", draw->row0, n_weeks);
        return SCG_OK;
      },
      [&](MlpDrawnArgs& da, int64_t done, int32_t done_k) {
        da.std = policy->std;
        da.samples_out = policy->samples_out ? policy->samples_out + done : nullptr;
        da.features_out = policy->features_out ? policy->features_out + done * kLocalFeatures : nullptr;
        da.hidden = policy->hidden;
        da.lo = policy->act_lo;
        da.hi = policy->act_hi;
        da.key0 = static_cast<uint32_t>(draw->seed & 0xffffffffu);
        da.key1 = static_cast<uint32_t>(draw->seed >> 32);
        da.row0 = draw->row0 + static_cast<uint32_t>(done_k);
      });
}

int scg_bg_noise_fill(const scg_bg_config* cfg, const scg_bg_state* st, uint64_t seed, uint32_t row0, int32_t n_rows,
                      float* out, void* stream) {
  if (int rc = check_state(cfg, st)) return rc;
  if (cfg->levels > SCG_BG_POLICY_MAX_LEVELS)
    return fail(SCG_ERR_INVALID, "noise fill: levels=%d above %d", cfg->levels, SCG_BG_POLICY_MAX_LEVELS);
  if (n_rows < 0 || static_cast<int64_t>(row0) + n_rows > (int64_t(1) << 32))
    return fail(SCG_ERR_INVALID, "noise fill: rows %u + %d", row0, n_rows);
  if (n_rows == 0) return SCG_OK;
  if (!out) return fail(SCG_ERR_INVALID, "noise fill: the out buffer is required");
  return bg_launch_noise_fill(static_cast<hipStream_t>(stream), cfg->levels, st->n_envs, n_rows, static_cast<uint32_t>(seed & 0xffffffffu),
                              static_cast<uint32_t>(seed >> 32), row0, static_cast<uint32_t>(st->env_offset), out);
}

int scg_bg_local_features(const scg_bg_config* cfg, const scg_bg_state* st, int32_t* out, void* stream) {
  if (int rc = check_state(cfg, st)) return rc;
  if (!out) return fail(SCG_ERR_INVALID, "local features: null output");
  if (int rc = check_local_config(cfg)) return rc;
  if (st->week < 0) return fail(SCG_ERR_NOT_RESET, "local features before reset()");
  if (st->week > cfg->max_weeks) return fail(SCG_ERR_INVALID, "local features: week %d past the horizon %d", st->week, cfg->max_weeks);
  const BgArgs a = make_args(cfg, st);
  return bg_launch_local_features(grid_for(st->n_envs), static_cast<hipStream_t>(stream), a, cfg->levels, st->week,
                                  local_mask(cfg, st->week), local_last_fixed(cfg, st->week), out);
}

int scg_bg_poisson_demand(const scg_bg_config* cfg, const scg_bg_state* st, uint32_t episode, int32_t* out,
                          void* stream) {
  if (int rc = check_state(cfg, st)) return rc;
  if (!out) return fail(SCG_ERR_INVALID, "null output");
  if (cfg->demand_mode != SCG_DEMAND_POISSON) return fail(SCG_ERR_INVALID, "config is not in POISSON demand mode");
  BgArgs a = make_args(cfg, st);
  a.episode = episode;
  hipLaunchKernelGGL(poisson_demand_kernel, grid_for(st->n_envs), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                     a, cfg->max_weeks, out);
  return check_launch("poisson_demand_kernel");
}

int scg_uniform_ints(uint64_t seed, int64_t env_offset, int64_t n_envs, int32_t rows, int32_t width, uint32_t tag,
                     int32_t lo, int32_t hi, int32_t* out, void* stream) {
  if (!out || n_envs <= 0 || rows <= 0 || width <= 0 || hi < lo)
    return fail(SCG_ERR_INVALID, "bad uniform_ints arguments");
  // The Philox env counter is 32-bit: global env ids past 2^32 would reuse another env's draws.
  if (env_offset < 0 || env_offset + n_envs > (int64_t(1) << 32))
    return fail(SCG_ERR_INVALID, "uniform_ints env ids must lie in [0, 2^32)");
  if (static_cast<int64_t>(rows) * width > INT32_MAX)
    return fail(SCG_ERR_INVALID, "uniform_ints rows * width must fit int32");
  const uint32_t range = static_cast<uint32_t>(static_cast<int64_t>(hi) - lo + 1);  // 0 means 2^32
  if (range == 0) return fail(SCG_ERR_INVALID, "uniform_ints range must be < 2^32");
  hipLaunchKernelGGL(uniform_ints_kernel, grid_for(n_envs), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                     static_cast<uint32_t>(seed & 0xffffffffu), static_cast<uint32_t>(seed >> 32), env_offset, n_envs,
                     rows, width, tag, lo, range, out);
  return check_launch("uniform_ints_kernel");
}

}  // extern "C"
