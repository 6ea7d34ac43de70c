/*
 * scgpu — MI355X-native (gfx950) vectorised supply-chain environments: C ABI.
 *
 * This is the drop-in boundary for the hot path of caburu/gym-supplychain
 * (reference snapshot 2024-08-07, mounted at /root/reference): the per-env
 * step()/reset() dynamics of BeerGameEnv, run as fused HIP kernels over a batch of
 * N envs held in caller-owned device buffers.
 *
 * The reference is pure Python; its "interface" for this path is the gym.Env
 * surface of BeerGameEnv (gym_supplychain/envs/beergame_env.py):
 *     __init__(env_init_info)  beergame_env.py:11-60   -> scg_bg_config + scg_bg_prepare
 *     reset()                  beergame_env.py:140-156 -> scg_bg_reset
 *     step(action)             beergame_env.py:66-138  -> scg_bg_step / scg_bg_rollout
 *     _observation()           beergame_env.py:180-181 -> fused into the step epilogue
 * The Python package gym_supplychain_amd binds these entry points with ctypes
 *  and re-exposes the reference's class names and gym API.
 *
 * Conventions
 *   - Every function returns an int status (scg_status). Nothing throws across the ABI.
 *     On failure scg_last_error() describes the problem (thread-local).
 *   - The library never allocates device memory and never synchronises: all buffers
 *     are owned by the caller, every launch is asynchronous on the caller's stream
 *     (`stream` is a hipStream_t passed as void*; NULL = the null stream).
 *   - Integer state is int32; the reference's int64 values are reproduced exactly while
 *     every value stays within int32 range (DESIGN.md "Integer range").
 *   - Layouts are env-major: a [N][L] int32 array holds env n's L levels contiguously.
 */
#ifndef SCGPU_H
#define SCGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 5 (round 4): scg_sc_state.inbox_tk is uint8 [inbox_size][N] (byte-packed entries);
 *   shipment delays up to SCG_BG_MAX_DELAY = 4096; full_table of any row count.
 * 6 (round 5): the BeerGame step server (scg_bg_server_box, scg_bg_server, scg_bg_server_step,
 *   scg_bg_server_stop) and the testing hook scg_sc_nodes_max_blocks.
 * 7 (round 6): the step server serves up to SCG_BG_SERVER_SLOTS envs from one wave
 *   (scg_bg_server_slot, attach / detach / post / wait), mixing-hash check word; the
 *   SupplyChain step server (scg_sc_server_box, scg_sc_server, scg_sc_server_*).
 * 8: scg_bg_state ends with step_consts / step_consts_tag: the device block of the slab
 *   step kernel's launch constants (SCG_BG_STEP_CONSTS_BYTES).
 * 9: scg_sc_rollout (K SupplyChain steps per call, SCG_SC_ROLLOUT_MAX, SCG_SC_LAST_OBS) and
 *   the testing hook scg_sc_rollout_chunk; also scg_bg_rollout_policy (scg_bg_policy: the
 *   closed-loop BeerGame rollout with a per-env linear policy), an added entry point; also
 *   scg_sc_observe and scg_sc_rollout_policy (scg_sc_policy: the closed-loop SupplyChain
 *   rollout with a linear policy, per env or shared), added entry points; also
 *   scg_sc_rollout_mlp and scg_sc_mlp_fused (scg_sc_mlp: the same closed loop with a
 *   one-hidden-layer ReLU policy), added entry points; also scg_sc_rollout_sampled
 *   (scg_sc_sampling: either closed loop with the caller's noise added to the action before
 *   its clamp, for policy-gradient training), an added entry point; also scg_bg_rollout_local
 *   and scg_bg_local_features (scg_bg_local_policy: the closed-loop BeerGame rollout with a
 *   local-information policy on inventory position and orders), added entry points; also
 *   scg_bg_rollout_mlp (scg_bg_mlp: the same closed loop with a shared one-hidden-layer ReLU
 *   policy in float32 over the local features, deterministic or sampled from the caller's
 *   noise), an added entry point; also scg_sc_rollout_drawn, scg_sc_noise_fill and the testing
 *   hook scg_noise_from_words (scg_sc_noise_draw: the sampled SupplyChain closed loop with
 *   its noise drawn on the device from a seed and a row counter), added entry points; also
 *   scg_bg_rollout_drawn and scg_bg_noise_fill (scg_bg_noise_draw: the sampled BeerGame MLP
 *   loop with the same noise drawn on the device), added entry points. */
#define SCG_ABI_VERSION 9

#if defined(__GNUC__)
#define SCG_API __attribute__((visibility("default")))
#else
#define SCG_API
#endif

#define SCG_BG_MAX_LEVELS 16   /* template instantiations of the step kernel        */
#define SCG_BG_MAX_WEEKS 4096  /* episode horizon (len(customer_demand), :37)        */
#define SCG_BG_MAX_DELAY 4096  /* shipment delay bound: ring slots R = max delay + 1 */
#define SCG_POISSON_MAX 256    /* CDF threshold table entries                        */
#define SCG_BG_ROLLOUT_MAX 128 /* weeks per rollout launch (host loops beyond)       */

typedef enum scg_status {
  SCG_OK = 0,
  SCG_ERR_INVALID = 1,      /* bad argument or config              -> ValueError    */
  SCG_ERR_PAST_HORIZON = 2, /* step after the terminal week        -> IndexError    */
                            /* (the reference raises IndexError on customer_demand[T], :79) */
  SCG_ERR_NOT_RESET = 3,    /* step before reset                   -> RuntimeError  */
  SCG_ERR_HIP = 4           /* HIP launch/runtime error            -> RuntimeError  */
} scg_status;

typedef enum scg_demand_mode {
  SCG_DEMAND_FIXED = 0,   /* one list shared by all envs: customer_demand (beergame_env.py:33) */
  SCG_DEMAND_TABLE = 1,   /* per-env device table int32 [T][N] (caller-drawn demand)            */
  SCG_DEMAND_POISSON = 2, /* per-(env, episode, week) Poisson draw on device, Philox4x32-10     */
  SCG_DEMAND_UNIFORM = 3  /* per-(env, episode, week) randint(demand_lo, demand_hi), Philox     */
} scg_demand_mode;

/* Step flags */
#define SCG_BG_AUTORESET 1u /* at the terminal week reset in the same launch (VecEnv semantics) */
#define SCG_SC_SERIAL 2u    /* node-parallel SupplyChain kernel: step every env with its serial
                               walk (the path of envs whose receive order it cannot prove; tests) */
#define SCG_SC_LAST_OBS 8u  /* scg_sc_rollout: obs is [N][n_obs], only the last step's is stored */

/* Philox streams (counter word 3) */
#define SCG_STREAM_DEMAND 0u
#define SCG_STREAM_ACTION 1u
#define SCG_STREAM_BG2_DEMAND 4u
#define SCG_STREAM_BG2_DELAY 5u

/*
 * Env configuration, the resolved form of BeerGameEnv's env_init_info
 * (beergame_env.py:16-58). Host memory, owned by the caller.
 */
typedef struct scg_bg_config {
  int32_t levels;                 /* L, :26                                            */
  int32_t max_weeks;              /* T = len(customer_demand), :37                     */
  int32_t inv_cost;               /* :28                                               */
  int32_t backlog_cost;           /* :30                                               */
  int32_t initial_shipment_value; /* :41                                               */
  int32_t initial_orders_value;   /* :43                                               */
  int32_t initial_inventory[SCG_BG_MAX_LEVELS]; /* :35                                 */
  int32_t demand_mode;            /* scg_demand_mode                                   */
  int32_t poisson_len;            /* entries in poisson_thresholds (POISSON mode)      */
  const int32_t* shipment_delays; /* HOST [T+1]: [2] + user list, exactly :39          */
  const int32_t* customer_demand; /* HOST [T]: FIXED mode demand, :33                  */
  const int32_t* demand_table;    /* DEVICE [T][N]: TABLE mode demand                   */
  const uint32_t* poisson_thresholds; /* DEVICE [poisson_len] (scg_poisson_table)       */
  int32_t* plan;                  /* HOST [T+1] workspace, filled by scg_bg_prepare     */
  int32_t ring_slots;             /* out of scg_bg_prepare: R = max delay + 1           */
  /* BeerGameEnv2 (beergame2_env.py:5-211) when variant == 2 ----------------------------- */
  int32_t variant;                /* 1: BeerGameEnv, 2: BeerGameEnv2                    */
  int32_t max_stock;              /* v2: observation offset and capacity (:24, :112)    */
  int32_t exceeded_capacity_penalty; /* v2: per unit beyond max_stock (:35, :179-180)  */
  int32_t demand_lo, demand_hi;   /* SCG_DEMAND_UNIFORM: randint(lo, hi) per week (:77) */
  int32_t stochastic_delays;      /* v2: per-episode randint(delay_lo, delay_hi) (:91)  */
  int32_t delay_lo, delay_hi;
  /* In (BeerGameEnv only): 1 = keep the reference's whole absolute-week shipment table
   * instead of the ring — ring_slots becomes its row count max(T+1, max_w(w+d_w+1)) + 1
   * (beergame_env.py:46-50), slot s holds week s, and shipments that land after the
   * horizon are stored as the reference stores them. Rows are not cleared between
   * episodes: a row not yet scheduled in the current episode holds a stale value (the
   * reference's is 0; scg_bg_prepare's plan says which rows are scheduled by each week).
   * Any row count (T + max delay + 2 at most); the state slab, and so the slab step kernel,
   * takes ring_slots <= 127, a longer table separate buffers and the general step kernel. */
  int32_t full_table;
} scg_bg_config;

/*
 * Batch state: caller-owned device buffers plus host-side counters the library
 * advances. Optional buffers may be NULL (then that output is not produced).
 */
typedef struct scg_bg_state {
  int64_t n_envs;           /* N envs in this shard                                   */
  int64_t env_offset;       /* global id of env 0 of this shard (multi-GPU sharding)   */
  uint64_t seed;            /* Philox key                                             */
  uint32_t episode;         /* episode counter (Philox); advanced by reset/auto-reset  */
  int32_t week;             /* 0 after reset, T at the terminal week; -1 = not reset   */
  int32_t* inventory;       /* [N][L]  self.inventory      :72,:101                    */
  int32_t* backlog;         /* [N][L]  self.backlog        :103                        */
  int32_t* orders_placed;   /* [N][L]  self.orders_placed  :121                        */
  int32_t* shipments;       /* [R][N][L] ring over absolute weeks (self.shipments :50)  */
  int32_t* inventory_costs; /* [N][L]  self.inventory_costs :131   (optional)           */
  int32_t* backlog_costs;   /* [N][L]  self.backlog_costs   :132   (optional)           */
  int32_t* orders_history;  /* [T+1][N][L] self.all_orders_placed :123 (optional)       */
  int64_t* episode_return;  /* [N] running sum of rewards (optional)                   */
  int64_t* final_return;    /* [N] episode_return at the terminal week (optional)      */
  int32_t* penalty_costs;   /* [N][L]  v2 self.penalty_costs :184 (optional)           */
  /* Sticky DEVICE int32 error word (optional): bit 0 is set by any kernel whose int64
   * result (state, pipeline row, ledger, observation or reward; the reference computes in
   * int64, beergame_env.py:33,35,130-132) does not fit the int32 it is stored in. The
   * stored values are then invalid; the flag stays set (across auto-resets too) until
   * scg_bg_reset, whose kernel clears it and error_host in stream order, or the caller. */
  int32_t* error_flags;
  /* Optional HOST-mapped int32 (pinned, device-accessible): every terminal-week launch copies
   * error_flags there as the launch starts, so a host can poll earlier episodes' overflow
   * without synchronising (read it after a later episode's terminal step has completed). */
  int32_t* error_host;
  /* Optional state slab (scg_bg_slab_layout): when non-NULL, every buffer above must be
   * the slab view the layout names, and scg_bg_step launches the slab step kernel (given
   * step_consts below too), which addresses every row from this one base. */
  int32_t* slab;
  /* Optional DEVICE block of SCG_BG_STEP_CONSTS_BYTES bytes, 64-byte aligned, that the slab
   * step kernel reads its launch constants from (costs, guard, reset values, env_offset,
   * error_host, the demand table pointers and the first Poisson thresholds: everything that
   * is fixed once the env is built) in one round of scalar loads. The caller only allocates
   * it; the library fills it in stream order, by a small kernel ahead of the step, whenever
   * step_consts_tag differs from the fingerprint of cfg / st the step is called with (so
   * editing cfg between steps is safe; the contents of poisson_thresholds are fingerprinted
   * by pointer and length only). NULL: scg_bg_step runs the general step kernel, slab or not. */
  void* step_consts;
  /* Host: fingerprint of what step_consts holds (0: nothing). Zero it after writing the block
   * or the threshold table by other means. */
  uint64_t step_consts_tag;
} scg_bg_state;

#define SCG_BG_STEP_CONSTS_BYTES 512

/* Slab fields, in order: word offsets filled by scg_bg_slab_layout. */
enum scg_bg_slab_field {
  SCG_SLAB_ERROR = 0,     /* int32 error word (16-byte header)              */
  SCG_SLAB_INVENTORY,     /* [N][L]                                          */
  SCG_SLAB_BACKLOG,       /* [N][L]                                          */
  SCG_SLAB_ORDERS,        /* [N][L]                                          */
  SCG_SLAB_INV_COSTS,     /* [N][L]                                          */
  SCG_SLAB_BACKLOG_COSTS, /* [N][L]                                          */
  SCG_SLAB_TERMINAL_OBS,  /* [N][L]                                          */
  SCG_SLAB_RING,          /* [R][N][L]                                       */
  SCG_SLAB_EPISODE_RETURN,/* int64 [N] (word offset, 8-byte aligned)         */
  SCG_SLAB_FINAL_RETURN,  /* int64 [N]                                       */
  SCG_SLAB_HISTORY,       /* [T+1][N][L] when requested, else == total       */
  SCG_SLAB_TOTAL,         /* words in the slab                               */
  SCG_SLAB_FIELDS
};

/*
 * STREAM copy of `bytes` (a multiple of 16, 16-byte aligned DEVICE buffers): the
 * achievable-HBM-bandwidth probe bench.py reports beside the 8 TB/s spec
 * (roofline.measured_peak). blocks == 0: one 16-byte vector per lane, the grid covering the
 * buffer (the fastest shape measured); blocks > 0: a grid-stride loop over that many
 * workgroups of 256 lanes. Not part of the env path.
 */
SCG_API int scg_stream_copy(const void* src, void* dst, int64_t bytes, int32_t blocks, void* stream);

/* ABI version (SCG_ABI_VERSION of the built library). */
SCG_API int scg_abi_version(void);

/* sizeof(scg_bg_config) and sizeof(scg_bg_state) as compiled, to check FFI bindings. */
SCG_API int scg_bg_struct_sizes(size_t* config_size, size_t* state_size);

/* Last error message of the calling thread ("" if none). */
SCG_API const char* scg_last_error(void);

/*
 * Poisson(lam) inverse-CDF table: out[k] = min(floor(CDF(k) * 2^32), 2^32-1) for
 * k = 0..len-1, ending at the first saturated entry. Returns len (>0) or -SCG_ERR_INVALID.
 * Host function; the caller uploads the table for SCG_DEMAND_POISSON.
 */
SCG_API int scg_poisson_table(double lam, uint32_t* out, int32_t cap);

/*
 * Validate cfg and fill cfg->plan / cfg->ring_slots from cfg->shipment_delays
 * (replaces the shipment-table sizing of beergame_env.py:46-52). Host only.
 */
SCG_API int scg_bg_prepare(scg_bg_config* cfg);

/*
 * Word offsets of one state slab for n_envs envs of a prepared cfg (ring_slots known),
 * with the order history when with_history != 0. Host only; the caller allocates
 * offsets[SCG_SLAB_TOTAL] int32 words of DEVICE memory (16-byte aligned, zeroed), points
 * the scg_bg_state buffers at base + offsets[field] and sets st->slab = base (and, outside
 * the slab, st->step_consts to SCG_BG_STEP_CONSTS_BYTES of its own).
 */
SCG_API int scg_bg_slab_layout(const scg_bg_config* cfg, int64_t n_envs, int32_t with_history,
                               int64_t offsets[SCG_SLAB_FIELDS]);

/* reset() for all N envs (beergame_env.py:140-156). obs: DEVICE int32 [N][L] or NULL. */
SCG_API int scg_bg_reset(const scg_bg_config* cfg, scg_bg_state* st, int32_t* obs, void* stream);

/*
 * step(action) for all N envs (beergame_env.py:66-138), one fused kernel.
 *   action       DEVICE int32 [N][L]
 *   obs          DEVICE int32 [N][L]   inventory - backlog (:127,:180); with
 *                SCG_BG_AUTORESET at the terminal week: the reset observation
 *   reward       DEVICE int32 [N]      -sum(inv_cost*inv + backlog_cost*backlog) (:130)
 *   terminal_obs DEVICE int32 [N][L] or NULL: observation at the terminal week
 * Returns SCG_ERR_PAST_HORIZON when called after the terminal week without auto-reset.
 * Sets *done (host, may be NULL) to 1 when this step was the terminal week (:134).
 * With st->slab and st->step_consts set, reward == obs + N*L (one output allocation) and
 * terminal_obs NULL or the slab's SCG_SLAB_TERMINAL_OBS view, the slab kernel runs (terminal
 * obs into the slab); a step whose st->step_consts_tag is stale first launches the small kernel
 * that fills the block. Otherwise the general step kernel runs, with the same results.
 */
SCG_API int scg_bg_step(const scg_bg_config* cfg, scg_bg_state* st, const int32_t* action,
                int32_t* obs, int32_t* reward, int32_t* terminal_obs, uint32_t flags,
                int32_t* done, void* stream);

/*
 * scg_bg_step with the step kernel's own dispatch timestamps recorded into two
 * caller-created hipEvent_t (passed as void*, either may be NULL), via
 * hipExtLaunchKernel: hipEventElapsedTime(start, stop) is the kernel's duration as
 * rocprofv3 reports it. Used by bench.py for the roofline's measured kernel time.
 */
SCG_API int scg_bg_step_timed(const scg_bg_config* cfg, scg_bg_state* st, const int32_t* action,
                              int32_t* obs, int32_t* reward, int32_t* terminal_obs, uint32_t flags,
                              int32_t* done, void* start_event, void* stop_event, void* stream);

/*
 * Step server for drop-in envs stepped one week per host call (BeerGameEnv:
 * beergame_env.py:66-138 is one Python call per week). A launch plus a stream
 * synchronisation per week costs more than the reference's whole step, so instead one wave
 * stays resident per server: it polls a mailbox in host-mapped memory and runs the week body
 * of bg_step_kernel (the same code) on the state of whichever env posted a week. One server
 * serves up to SCG_BG_SERVER_SLOTS envs (a slot each: its request line, its answer word and
 * its kernel arguments), so a process that steps many drop-in envs in turn (a DummyVecEnv)
 * keeps ONE resident wave and one stream per device, not one per env. Every slot's config
 * must have the server's levels and demand mode; up to 64 envs per slot; variant 1, separate
 * state buffers (no slab), no auto-reset.
 *
 * The wave exits on scg_bg_server_stop, or by itself after idle_us without a request on any
 * slot, so it never outlives its process; scg_bg_server_post (re)launches it when it is not
 * running or may have timed out (idle for more than idle_us / 2 on the host's clock). When it
 * starts, every slot whose request is newer than its answer is served. Work the caller
 * launches on an env's state (reset, other steps) must be complete before that env's next
 * post, and must not start while one of its posts is unanswered; the mailbox must outlive
 * the wave. post/wait/step of different slots may run on different host threads.
 */
#define SCG_BG_SERVER_SLOTS 15
#define SCG_BG_SERVER_ARGS_BYTES 512
#define SCG_PENDING 5 /* scg_bg_server_wait: not answered within spin_us (not an error) */

typedef struct scg_bg_server_line { /* one 64-byte request line, read by the wave in one load */
  uint32_t req_seq;      /* request number (a new number is a new request)                      */
  int32_t cmd;           /* 0: step                                                            */
  uint32_t wpack;        /* the week's plan, as bg_step_kernel's packed word                   */
  int32_t week;          /* the week being stepped (1..max_weeks)                              */
  int32_t demand_fixed;  /* customer_demand[week - 1] for SCG_DEMAND_FIXED                     */
  int32_t n_inline;      /* L when env 0's action row travels in action[] (one env, L <= 8)    */
  uint32_t gen;          /* generation of the slot's kernel arguments (args[slot] below)       */
  uint32_t check;        /* scg mixing hash of the line's other 15 words: a read of the line
                            that mixes two requests is read again                            */
  int32_t action[8];
} scg_bg_server_line;

typedef struct scg_bg_server_box { /* host-mapped (hipHostMalloc mapped + coherent) */
  scg_bg_server_line req[SCG_BG_SERVER_SLOTS + 1]; /* slot k's request line is req[k]       */
  uint32_t done_seq[16];  /* slot k's last request served (written by the wave)             */
  uint32_t n_slots;       /* the wave polls slots 0 .. n_slots - 1                          */
  uint32_t exit_req;      /* the wave exits when this differs from its launch value         */
  uint32_t exit_seq;      /* written by the wave as it exits: the exit_req it saw last     */
  uint32_t pad[13];
  unsigned char args[SCG_BG_SERVER_SLOTS][SCG_BG_SERVER_ARGS_BYTES]; /* opaque, per slot    */
} scg_bg_server_box;

typedef struct scg_bg_server {
  scg_bg_server_box* box_host; /* the mailbox's host address                                */
  scg_bg_server_box* box_dev;  /* its device address (hipHostGetDevicePointer)              */
  void* stream;                /* the wave's stream: a non-blocking one of the caller's (a
                                  high-priority one keeps the parked wave off the hardware
                                  queues of normal-priority streams)                         */
  int32_t levels;              /* the wave's instantiation: every slot's config must match  */
  int32_t demand_mode;
  int32_t idle_us;             /* the wave exits after this long without a request          */
  int32_t check_us;            /* a waiting step checks this often whether the wave has
                                  gone (0: 2 s)                                              */
  /* host bookkeeping: zero before first use */
  int32_t lock;
  int32_t running;             /* the wave may be running                                   */
  uint32_t slots_used;         /* bit k: slot k attached                                    */
  int32_t pad;
  int64_t last_ns;             /* host monotonic time of the last request posted or served  */
  int64_t launches;            /* waves launched so far                                     */
} scg_bg_server;

typedef struct scg_bg_server_slot {
  scg_bg_server* server;       /* set by scg_bg_server_attach                               */
  const int32_t* action;       /* DEVICE-visible int32 [N][L], read each request            */
  const int32_t* action_host;  /* its host address, or NULL: with one env of L <= 8 the row
                                  is copied into the request line (no second read)         */
  int32_t* obs;                /* DEVICE-visible int32 [N][L]                               */
  int32_t* reward;             /* DEVICE-visible int32 [N]                                  */
  int32_t index;               /* out: the slot, -1 when detached                           */
  uint32_t gen;                /* out: generation of the arguments last published           */
  uint32_t seq;                /* out: the request last posted                              */
  int32_t week;                /* out: the week it steps                                    */
  int32_t done;                /* out: that week is the terminal one                        */
  int32_t relaunches;          /* out: waves this slot's waits launched again (wave gone)   */
} scg_bg_server_slot;

/* Take a free slot of `sv` for one env (slot->action/obs/reward set by the caller). */
SCG_API int scg_bg_server_attach(scg_bg_server* sv, scg_bg_server_slot* slot);
/* Give the slot back (no request of it may be unanswered). */
SCG_API int scg_bg_server_detach(scg_bg_server_slot* slot);
/* Post step(action) for the st->n_envs <= 64 envs of the slot; launches the wave if needed. */
SCG_API int scg_bg_server_post(const scg_bg_config* cfg, scg_bg_state* st, scg_bg_server_slot* slot);
/* Wait for the slot's posted step: SCG_OK (st->week advanced, *done as scg_bg_step),
 * SCG_PENDING after spin_us (< 0: no limit; the wait then fails after 60 s), or an error
 * (a HIP error of the wave's stream at once; a wave gone twice without answering). */
SCG_API int scg_bg_server_wait(scg_bg_state* st, scg_bg_server_slot* slot, int64_t spin_us, int32_t* done);
/* post + wait without limit. */
SCG_API int scg_bg_server_step(const scg_bg_config* cfg, scg_bg_state* st, scg_bg_server_slot* slot, int32_t* done);
/* Ask the wave to exit and wait for it (a no-op when it is not running). */
SCG_API int scg_bg_server_stop(scg_bg_server* sv);
/* The request line's check word (the mixing hash the wave recomputes). */
SCG_API uint32_t scg_bg_server_line_check(const scg_bg_server_line* line);

/*
 * K consecutive steps in one launch per <= SCG_BG_ROLLOUT_MAX weeks, state held in
 * registers/LDS (open-loop action plans, evaluation sweeps). Same results as K calls
 * of scg_bg_step with the same flags (SCG_BG_AUTORESET may cross episode ends), for
 * both variants: BeerGameEnv (variant 1: actions are order increments) and BeerGameEnv2
 * (variant 2: absolute orders, observations offset by max_stock, rewards including the
 * capacity penalty, per-env delays drawn in the launch when stochastic_delays is set;
 * an auto-reset inside a launch advances the episode the draws are keyed by).
 *   actions DEVICE int32 [K][N][L]; obs DEVICE int32 [K][N][L] or NULL;
 *   rewards DEVICE int32 [K][N] or NULL.
 * What a rollout does not produce, for either variant: no terminal_obs (with auto-reset
 * the obs row of a terminal week is the reset observation), and no export of the
 * overflow word to st->error_host at terminal weeks (the device word st->error_flags is
 * set as by scg_bg_step; read it after the rollout).
 * Every argument is checked before any HIP call: SCG_ERR_INVALID (null actions,
 * n_weeks < 0), SCG_ERR_NOT_RESET, and without SCG_BG_AUTORESET SCG_ERR_PAST_HORIZON
 * when st->week + n_weeks passes max_weeks; st is untouched on failure.
 */
SCG_API int scg_bg_rollout(const scg_bg_config* cfg, scg_bg_state* st, int32_t n_weeks,
                   const int32_t* actions, int32_t* obs, int32_t* rewards, uint32_t flags,
                   void* stream);

/*
 * Closed-loop rollout: K weeks per launch as scg_bg_rollout runs them, with each env's
 * action computed in registers from the observation the env last produced (what
 * scg_bg_reset or the previous week returned: inventory - backlog, for variant 2 plus
 * max_stock; after an auto-reset inside the launch, the reset observation) by a per-env
 * linear policy. For observation o[0..L) and parameters W[L][L], b[L] (int32):
 *   z_l = b_l + sum_j W[l][j] * o_j         int64, two's-complement wrap
 *   a_l = min(max(z_l >> shift, act_lo), act_hi)   arithmetic shift (floor), then the clamp
 * (csrc/scg_bg_policy.h is the one definition, host and device). With W = -g I, b = g S and
 * shift = log2 of the scale this is the smoothed order-up-to rule on net stock: for variant 1
 * the action is the increment over the incoming order, for variant 2 the absolute order
 * (clamp (0, max_order)).
 * The call equals n_weeks calls of scg_bg_step with the same flags, each with the action row
 * the formula gives for the previous observation: both variants, every demand mode, delay
 * lists and stochastic_delays; SCG_BG_AUTORESET may cross episode ends. As for
 * scg_bg_rollout there is no terminal_obs and no export to st->error_host.
 *   actions_out DEVICE int32 [K][N][L], the actions taken;  obs DEVICE int32 [K][N][L];
 *   rewards DEVICE int32 [K][N];  reward_sum DEVICE int64 [N], the sum of this call's K
 *   rewards per env (across auto-resets and launches; overwritten, not accumulated over
 *   calls). Each of the four may be NULL; with all four NULL and the ring in LDS a FIXED,
 *   POISSON or UNIFORM week touches no HBM (history rows excepted, when kept).
 * Every argument is checked before any HIP call, and st is untouched on failure:
 * SCG_ERR_INVALID (null policy or params, unknown kind, shift outside 0..30, act_lo > act_hi,
 * levels > SCG_BG_POLICY_MAX_LEVELS, n_weeks < 0), SCG_ERR_NOT_RESET, and without
 * SCG_BG_AUTORESET SCG_ERR_PAST_HORIZON.
 */
#define SCG_BG_POLICY_LINEAR 1
#define SCG_BG_POLICY_MAX_LEVELS 8
typedef struct scg_bg_policy {
  int32_t kind;            /* SCG_BG_POLICY_LINEAR */
  int32_t shift;           /* 0..30 */
  int32_t act_lo, act_hi;
  const int32_t* params;   /* DEVICE int32 [L*(L+1)][N], env fastest: word l*(L+1)+j is W[l][j] for j < L, b[l] for j == L */
} scg_bg_policy;

SCG_API int scg_bg_rollout_policy(const scg_bg_config* cfg, scg_bg_state* st, int32_t n_weeks,
                                  const scg_bg_policy* policy, int32_t* actions_out, int32_t* obs,
                                  int32_t* rewards, int64_t* reward_sum, uint32_t flags, void* stream);

/*
 * The same closed loop with a local-information policy: each level decides from four int32
 * about itself. For the state after week w of the current episode (w = 0: just reset), horizon
 * T, level l of L, in the reference's attribute names:
 *   f[l][0] net   inventory[l] - backlog[l] (+ max_stock for variant 2): scg_bg_rollout_policy's
 *                 observation
 *   f[l][1] line  the supply line: orders_placed[l] + (backlog[l+1] if l+1 < L else 0)
 *                 + sum_{v=w+1..T} shipments[v][l]
 *   f[l][2] down  the latest order from downstream: orders_placed[l-1] for l >= 1; for l = 0 the
 *                 customer demand of week w, initial_orders_value at w = 0 (also after an
 *                 auto-reset inside the call)
 *   f[l][3] own   orders_placed[l]
 * Shipments scheduled past week T are not in `line` (the kernels drop them: they are not in the
 * state). Every feature is int32 in wrapping arithmetic and touches no overflow flag.
 *   z_l = b_l + sum_{j<4} W[l][j] * f[l][j]        int64, two's-complement wrap
 *   a_l = min(max(z_l >> shift, act_lo), act_hi)   arithmetic shift (floor), then the clamp
 * (csrc/scg_bg_local.h is the one definition, host and device). W = (-1, -1, 0, 0), b = S is
 * order-up-to S on the inventory position (variant 2: b = S + max_stock).
 * The in-transit sum is taken once per launch over the ring rows the episode has scheduled (a
 * mask the host derives from the delay list and st->week), then kept in registers; nothing is
 * carried between launches or calls, so scg_bg_reset, scg_bg_step, scg_bg_rollout, this call and
 * a restored state may precede it in any order.
 * Buffers, flags, contract and error codes are scg_bg_rollout_policy's (kind must be
 * SCG_BG_POLICY_LOCAL); SCG_ERR_INVALID also for a delay above SCG_BG_LOCAL_MAX_DELAY
 * (shipment_delays[0..T] and, with stochastic_delays, delay_hi - 1) and for full_table configs.
 *
 * scg_bg_local_features writes the same four features of the state as it stands:
 *   out DEVICE int32 [N][L][4]. The same checks, except that week == max_weeks is allowed.
 */
#define SCG_BG_POLICY_LOCAL 2
#define SCG_BG_LOCAL_MAX_DELAY 64
typedef struct scg_bg_local_policy {
  int32_t kind;            /* SCG_BG_POLICY_LOCAL */
  int32_t shift;           /* 0..30 */
  int32_t act_lo, act_hi;
  const int32_t* params;   /* DEVICE int32 [5*L][N], env fastest: word l*5+j is W[l][j] for j < 4, b[l] for j == 4 */
} scg_bg_local_policy;

SCG_API int scg_bg_rollout_local(const scg_bg_config* cfg, scg_bg_state* st, int32_t n_weeks,
                                 const scg_bg_local_policy* policy, int32_t* actions_out, int32_t* obs,
                                 int32_t* rewards, int64_t* reward_sum, uint32_t flags, void* stream);
SCG_API int scg_bg_local_features(const scg_bg_config* cfg, const scg_bg_state* st, int32_t* out, void* stream);

/*
 * The same closed loop with a one-hidden-layer ReLU policy in float32 over the local features,
 * one network shared by every env. With f[l][j] the int32 features above of the state the env
 * stands in (after an auto-reset inside the call: the reset state's), x[l*4+j] = (float)f[l][j]
 * (round to nearest even, exact below 2^24), I = 4L and H = hidden:
 *   z_a = b2_a                                   a < L
 *   for i = 0 .. H-1 ascending:
 *       h = b1_i;  for j = 0 .. I-1 ascending:  h = h + W1[i][j] * x_j
 *       h = (h > 0) ? h : +0.0f
 *       for a < L:  z_a = z_a + W2[a][i] * h
 *   u_a   = z_a                                   noise == NULL: deterministic
 *   u_a   = z_a + (std_a * noise[k][n][a])        sampled; the product is rounded first
 *   act_a = !(u_a >= (float)act_lo) ? act_lo : (u_a >= (float)act_hi ? act_hi : (int32)rintf(u_a))
 * Every multiply and every add is rounded to float32 on its own, rintf rounds ties to even, a
 * NaN u gives act_lo; k is the week's index in the call (csrc/scg_bg_mlp.h is the one
 * definition, host and device).
 *   params DEVICE float32 [Q], Q = H*(I+1) + L*(H+1): word i*(I+1)+j is W1[i][j] for j < I and
 *     b1[i] for j == I; word H*(I+1) + a*(H+1) + i is W2[a][i] for i < H and b2[a] for i == H
 *     (the layout of scg_sc_mlp with O = I and A = L). There is no per-env form.
 *   std DEVICE float32 [L];  noise DEVICE float32 [K][N][L], both or neither;
 *   samples_out DEVICE float32 [K][N][L] or NULL: u; it may be `noise` itself (each element is
 *     read, then written, by one thread). Only with noise.
 *   features_out DEVICE int32 [K][N][L][4] or NULL: the features week k's action was computed
 *     from (what a trainer needs to recompute z with gradients).
 * actions_out, obs, rewards, reward_sum, flags, the launch cut, the contract and the error codes
 * are scg_bg_rollout_local's. SCG_ERR_INVALID, before any HIP call, also for: kind other than
 * SCG_BG_POLICY_MLP, hidden outside 1..SCG_BG_MLP_MAX_HIDDEN, act_lo or act_hi outside
 * [-2^24, 2^24] (so that both are exact as float32) or act_lo > act_hi, NULL params, noise
 * without std or std without noise, samples_out without noise.
 */
#define SCG_BG_POLICY_MLP 3
#define SCG_BG_MLP_MAX_HIDDEN 64
typedef struct scg_bg_mlp {
  int32_t kind;            /* SCG_BG_POLICY_MLP */
  int32_t hidden;          /* 1 .. SCG_BG_MLP_MAX_HIDDEN */
  int32_t act_lo, act_hi;  /* within [-2^24, 2^24] */
  const float* params;     /* DEVICE float32 [Q], shared */
  const float* std;        /* DEVICE float32 [L], or NULL */
  const float* noise;      /* DEVICE float32 [K][N][L], or NULL: deterministic */
  float* samples_out;      /* DEVICE float32 [K][N][L], or NULL */
  int32_t* features_out;   /* DEVICE int32 [K][N][L][4], or NULL */
} scg_bg_mlp;              /* 56 bytes, params at 16 */

SCG_API int scg_bg_rollout_mlp(const scg_bg_config* cfg, scg_bg_state* st, int32_t n_weeks, const scg_bg_mlp* policy,
                               int32_t* actions_out, int32_t* obs, int32_t* rewards, int64_t* reward_sum,
                               uint32_t flags, void* stream);

/*
 * scg_bg_rollout_mlp's sampled loop with the noise drawn on the device: noise[k][n][a] is not read
 * from memory but computed by the lane that owns the env, at the top of the week. It is the noise
 * of the SupplyChain closed loop (scg_sc_noise_draw below states the element; csrc/scg_normal.h is
 * the one definition, tests/noise_ref.py its NumPy statement): stream SCG_STREAM_SC_NOISE serves
 * both env families, a BeerGame action a is level a, and a BeerGame and a SupplyChain env given the
 * same seed draw the same numbers. The eps of week j of the call is element (row0 + j,
 * env_offset + n, a); j counts on across the launches a call is cut into and across auto-resets
 * inside the call, so a sharded batch draws what the unsharded one draws and a caller who cuts an
 * episode into several calls passes each its own row0.
 *   std, samples_out, features_out, params, hidden and the clamp are `policy`'s; policy->noise
 *   must be NULL. seed is the noise's own (not the state's); row0 the global row of the call's
 *   first week.
 * Contract, flags, the launch cut, the n_weeks == 0 path and the error codes are
 * scg_bg_rollout_mlp's. Checked before any HIP call, st left untouched: SCG_ERR_INVALID for a NULL
 * draw, for reserved != 0, for a non-NULL policy->noise, for a NULL policy->std with n_weeks > 0,
 * for row0 + n_weeks > 2^32, and for everything scg_bg_rollout_mlp refuses.
 */
typedef struct scg_bg_noise_draw {
  uint64_t seed;
  uint32_t row0;
  uint32_t reserved;   /* 0 */
} scg_bg_noise_draw;   /* 16 bytes */

SCG_API int scg_bg_rollout_drawn(const scg_bg_config* cfg, scg_bg_state* st, int32_t n_weeks, const scg_bg_mlp* policy,
                                 const scg_bg_noise_draw* draw, int32_t* actions_out, int32_t* obs, int32_t* rewards,
                                 int64_t* reward_sum, uint32_t flags, void* stream);

/* Rows row0 .. row0 + n_rows - 1 of that noise for the state's envs, into out DEVICE float32
 * [n_rows][N][L] (levels <= SCG_BG_POLICY_MAX_LEVELS). SCG_ERR_INVALID for a NULL out with
 * n_rows > 0, n_rows < 0 or row0 + n_rows > 2^32. */
SCG_API int scg_bg_noise_fill(const scg_bg_config* cfg, const scg_bg_state* st, uint64_t seed, uint32_t row0,
                              int32_t n_rows, float* out, void* stream);

/*
 * Device-side Philox draws for tests and benchmarks (no host round trip):
 *  scg_bg_poisson_demand: out DEVICE int32 [T][N], the demand scg_bg_step draws
 *    for episode `episode` in SCG_DEMAND_POISSON mode.
 *  scg_uniform_ints: out DEVICE int32 [rows][N][width], uniform in [lo, hi],
 *    word j of env n from philox(ctr=(env_offset+n, tag, j/4, SCG_STREAM_ACTION))[j%4]
 *    with j = row*width + col.
 */
SCG_API int scg_bg_poisson_demand(const scg_bg_config* cfg, const scg_bg_state* st, uint32_t episode,
                          int32_t* out, void* stream);
SCG_API int scg_uniform_ints(uint64_t seed, int64_t env_offset, int64_t n_envs, int32_t rows,
                     int32_t width, uint32_t tag, int32_t lo, int32_t hi, int32_t* out,
                     void* stream);

/* ======================================================================================
 * SupplyChainEnv (supplychain_env.py:478-813): generic multi-echelon, multi-product chain.
 *
 *   SupplyChainEnv.__init__(nodes_info, ...)  :482-628  -> scg_sc_config + scg_sc_node[] + scg_sc_prepare
 *   SupplyChainEnv.reset()                    :630-682  -> scg_sc_reset
 *   SupplyChainEnv.step(action)               :703-748  -> scg_sc_step / scg_sc_rollout
 *     SC_Node.act :208-396, SC_Action.apply :42-98, heapq pipeline :398-400,
 *     _build_observation :762-791, SC_Node.build_observation :428-463 (all fused)
 * Per-episode randomness (customer demand table, stochastic lead times; the reference
 * draws both with RandomState at reset, :644-672) is drawn on device with Philox:
 * demand word (t*R + r)*P + p on stream 2, lead-time word (t-1)*n_lt + k on stream 3.
 * ====================================================================================== */

#define SCG_SC_MAX_PRODUCTS 16
#define SCG_SC_MAX_DESTS 32
#define SCG_SC_MAX_INIT 16
#define SCG_SC_MAX_NODES 256
#define SCG_SC_MAX_LEVELS 16
#define SCG_SC_LEDGER_KEYS 8 /* info['sc_episode'] cost/unit categories (:416-417) */
#define SCG_SC_ROLLOUT_MAX 1024 /* steps per rollout launch; the host loops beyond */

/* SupplyChain kernels (scg_sc_config.kernel) and the state layouts they use. */
#define SCG_SC_KERNEL_AUTO 0
#define SCG_SC_KERNEL_LANE 1  /* one lane walks one env's whole chain; env-fastest state       */
#define SCG_SC_KERNEL_LEVEL 2 /* a lane group per env, one lane per node of a level; env-major */
#define SCG_SC_KERNEL_STAGED 3 /* one lane per env, one node's heaps in LDS at a time, shipments
                                  through a per-env global inbox; env-fastest                 */
#define SCG_SC_KERNEL_NODES 4  /* 64 envs x W waves per block, a wave per node: all nodes act at
                                  once, heaps and shipments in LDS; env-fastest               */
#define SCG_SC_LAYOUT_ENV_FASTEST 0 /* stock [NP][N], heaps [NP][H][N], sizes [NP][N]          */
#define SCG_SC_LAYOUT_ENV_MAJOR 1   /* stock [N][NP], heaps [N][NP][H], sizes [N][NP]          */
#define SCG_STREAM_SC_DEMAND 2u
#define SCG_STREAM_SC_LEADTIME 3u
/* Stream 6 serves both env families (scg_sc_noise_draw, scg_bg_noise_draw): a BeerGame and a
 * SupplyChain env given the same seed draw the same numbers. */
#define SCG_STREAM_SC_NOISE 6u /* the exploration noise a closed loop draws itself (scg_sc_noise_draw) */

/* One chain node (SC_Node :106-206 after define_destinations), in nodes_info order. */
typedef struct scg_sc_node {
  int32_t last_level;           /* retailer: serves customer demand (:379-387)             */
  int32_t n_supply;             /* SUPPLY actions: products with supply_capacity > 0       */
  int32_t n_ship;               /* SHIP actions: n_dests per product with stock_capacity>0 */
  int32_t n_dests;
  int32_t processing_capacity;  /* > 0: a factory (:298-310, :337-341)                     */
  int32_t retailer_index;       /* customer_demands column, -1 if not a retailer           */
  int32_t action_offset;        /* first action of this node in the action vector (:716)  */
  int32_t leadtime_offset;      /* first lead time of this node in a step's row (:720-722) */
  int32_t supply_capacity[SCG_SC_MAX_PRODUCTS];
  int32_t supply_cost[SCG_SC_MAX_PRODUCTS];
  int32_t stock_capacity[SCG_SC_MAX_PRODUCTS];
  int32_t stock_cost[SCG_SC_MAX_PRODUCTS];
  int32_t processing_ratio[SCG_SC_MAX_PRODUCTS];
  int32_t processing_cost[SCG_SC_MAX_PRODUCTS];
  int32_t max_ship[SCG_SC_MAX_PRODUCTS];       /* observation normaliser (:147, :206)     */
  int32_t initial_stock[SCG_SC_MAX_PRODUCTS];
  int32_t n_init[SCG_SC_MAX_PRODUCTS];         /* initial pipeline entries (:402-412)     */
  int32_t init_time[SCG_SC_MAX_PRODUCTS][SCG_SC_MAX_INIT];
  int32_t init_amount[SCG_SC_MAX_PRODUCTS][SCG_SC_MAX_INIT];
  int32_t dests[SCG_SC_MAX_DESTS];             /* node indices                            */
  int32_t ship_capacity[SCG_SC_MAX_DESTS];
  int32_t dest_costs[SCG_SC_MAX_PRODUCTS][SCG_SC_MAX_DESTS];
  /* out of scg_sc_prepare (staged kernel): this node's shipment inbox — one entry per
   * (product, source node) at in_base + p * in_deg + k, sources k in node order — and, per
   * destination d, where this node's shipment lands in the destination's inbox:
   * in_slot[d] + p * in_stride[d]. */
  int32_t in_deg, in_base;
  int32_t in_slot[SCG_SC_MAX_DESTS];
  int32_t in_stride[SCG_SC_MAX_DESTS];
} scg_sc_node;

typedef struct scg_sc_config {
  int32_t n_nodes, n_products, n_retailers;
  int32_t n_actions;            /* action_space size (:608-610)                            */
  int32_t n_obs;                /* observation_space size (:617-621)                       */
  int32_t n_leadtimes;          /* lead times per step when stochastic (:601-605)          */
  int32_t total_time_steps;     /* T                                                       */
  int32_t avg_leadtime, max_leadtime, stochastic_leadtimes;
  int32_t demand_lo, demand_hi; /* uniform demand range (demands_generator.py:33-36)       */
  int32_t unmet_demand_cost, exceeded_stock_capacity_cost;
  int32_t exceeded_process_capacity_cost, exceeded_ship_capacity_cost;
  int32_t heap_capacity;        /* H: entries per (node, product) heap (scg_sc_prepare)    */
  int32_t leadtime_poisson_len;
  int32_t obs_f64;              /* observation dtype: 0 float32, 1 float64                 */
  int32_t max_dests;            /* out of scg_sc_prepare: most destinations of any node    */
  const scg_sc_node* nodes;     /* DEVICE [n_nodes]                                        */
  const uint32_t* leadtime_poisson; /* DEVICE Poisson(avg_leadtime-1) thresholds           */
  const int32_t* demand_table;  /* DEVICE [N][T+1][R][P] caller tables instead of Philox    */
                                /* (NULL = draw; e.g. to replay RandomState episodes)       */
  const int32_t* leadtime_table;/* DEVICE [N][T][n_leadtimes] likewise (stochastic only)    */
  /* Kernel choice (in: SCG_SC_KERNEL_*, 0 = auto; out: the kernel scg_sc_step launches) and
   * what scg_sc_prepare derives for it: the state layout, lanes per env and the level
   * schedule (levels are runs of consecutive nodes; every shipment goes from a level to
   * the next one, so a level's nodes never depend on each other within a step). */
  int32_t kernel;
  int32_t layout;               /* out: SCG_SC_LAYOUT_*                                     */
  int32_t group;                /* out: lanes per env (level kernel), waves per block (nodes)*/
  int32_t n_levels;             /* out: 0 when the chain has no such schedule               */
  int32_t level_start[SCG_SC_MAX_LEVELS + 1];
  int32_t inbox_size;           /* out: shipment inbox entries per env (level/staged/nodes) */
  int32_t level_staged;         /* out: 1 = the level kernel stages each env's state in LDS */
  /* Per-product demand models (demands_generator.py:3-89). demand_models = 0: every
   * product is uniform on [demand_lo, demand_hi]. Otherwise per product p: kind
   * SCG_SC_DEMAND_*, range [lo_p, hi_p] (also the observation's normalisation, :771-777),
   * NORMAL / SINE_NORMAL: a draw is lo_p + #{k : thr[off_p + row * (hi_p - lo_p) + k] <= u}
   * (row 0 for NORMAL, the period for SINE_NORMAL); SINE_UNIFORM: rint(clip(base[off_p +
   * period] + j, lo_p, hi_p)) with j = pert_lo_p + floor(u * pert_n_p / 2^32). */
  int32_t demand_models;
  int32_t demand_kind[SCG_SC_MAX_PRODUCTS];
  int32_t demand_lo_p[SCG_SC_MAX_PRODUCTS], demand_hi_p[SCG_SC_MAX_PRODUCTS];
  int32_t demand_pert_lo[SCG_SC_MAX_PRODUCTS], demand_pert_n[SCG_SC_MAX_PRODUCTS];
  int64_t demand_off[SCG_SC_MAX_PRODUCTS];
  const uint32_t* demand_thr;   /* DEVICE thresholds of the NORMAL / SINE_NORMAL products  */
  const double* demand_base;    /* DEVICE [T+1] sinusoid bases of the SINE_UNIFORM products */
} scg_sc_config;

#define SCG_SC_DEMAND_UNIFORM 0
#define SCG_SC_DEMAND_NORMAL 1
#define SCG_SC_DEMAND_SINE_NORMAL 2
#define SCG_SC_DEMAND_SINE_UNIFORM 3

/* Batch state. NP = n_nodes * n_products; per-env arrays follow cfg->layout (shapes below
 * are the env-fastest ones; env-major puts the env index first). */
typedef struct scg_sc_state {
  int64_t n_envs;
  int64_t env_offset;
  uint64_t seed;
  uint32_t episode;
  int32_t time_step;            /* 0 after reset; -1 = not reset                           */
  double* stock;                /* [NP][N]     float64 stock (:228)                        */
  int32_t* heap_tk;             /* [NP][H][N]  time << 3 | NumPy kind of the amount        */
  double* heap_val;             /* [NP][H][N]  amount                                       */
  int32_t* heap_size;           /* [NP][N]                                                  */
  double* episode_return;       /* [N] optional                                             */
  double* final_return;         /* [N] optional: return at the terminal step                */
  int32_t* error_flags;         /* [1] DEVICE, sticky: bit 0 = a heap exceeded capacity    */
  uint8_t* inbox_tk;            /* [inbox_size][N] staged kernel: shipment (time - t)<<3|kind, 0xFF = none */
  double* inbox_val;            /* [inbox_size][N] staged kernel: shipment amount               */
  /* build_info ledgers, info['sc_episode'] (:684-695, :750-760): optional (every kernel but
     the level kernel).
     Entry ((part * SCG_SC_LEDGER_KEYS + key) * P + p), part 0 = costs, 1 = units, keys in
     the reference's order (stock, stock_pen, supply, process, process_pen, ship, ship_pen,
     unmet_dem); value in ledger, NumPy type (0 int, 1 float, 2 float32, 3 float64, 4 int64)
     in ledger_kind. The final_* pair receives the terminal step's ledger on auto-reset. */
  double* ledger;               /* [2 * 8 * P][N] */
  int32_t* ledger_kind;         /* [2 * 8 * P][N] */
  double* final_ledger;         /* [2 * 8 * P][N] optional */
  int32_t* final_ledger_kind;   /* [2 * 8 * P][N] optional */
  /* Node-parallel kernel with ledgers: each node's entry values of the step, float64
   * [n_nodes * 2 * 8 * P][N] (slot ((node * 2 + part) * 8 + key) * P + p; their NumPy types
   * stay in LDS), added to the ledger in node order after the step (:750-760). Without it a
   * ledger step of a SCG_SC_KERNEL_NODES config runs the lane kernel on the same state. */
  double* ledger_part;
} scg_sc_state;

/* sizeof(scg_sc_node), sizeof(scg_sc_config), sizeof(scg_sc_state), to check FFI bindings. */
SCG_API int scg_sc_struct_sizes(size_t* node_size, size_t* config_size, size_t* state_size);

/* Validate cfg against the host copy of the node table; fills n_actions, n_obs,
 * n_leadtimes, heap_capacity and max_dests. Host only. */
SCG_API int scg_sc_prepare(scg_sc_config* cfg, scg_sc_node* host_nodes);

/* reset() for all envs (:630-682). obs: DEVICE [N][n_obs] (float32 or float64) or NULL. */
SCG_API int scg_sc_reset(const scg_sc_config* cfg, scg_sc_state* st, void* obs, void* stream);

/* step(action) for all envs (:703-748).
 *   action DEVICE float32 [N][n_actions], in the reference's [-1, 1] convention (:697-698)
 *   obs    DEVICE [N][n_obs]; reward DEVICE float64 [N]; terminal_obs optional.
 * Returns SCG_ERR_PAST_HORIZON after the terminal step without SCG_BG_AUTORESET. */
SCG_API int scg_sc_step(const scg_sc_config* cfg, scg_sc_state* st, const float* action, void* obs,
                        double* reward, void* terminal_obs, uint32_t flags, int32_t* done, void* stream);

/* K steps in one call: the same results as n_steps calls of scg_sc_step with the same flags,
 * bit for bit — every observation, reward, episode_return and final_return, the sticky
 * error flag, the live heap entries in storage order, the heap sizes and the stocks
 * afterwards, st->time_step and st->episode (heap slots past a heap's size may differ).
 *   actions      DEVICE float32 [K][N][n_actions]
 *   obs          DEVICE [K][N][n_obs] in the config's obs dtype; with SCG_SC_LAST_OBS
 *                [N][n_obs], which receives only the last step's observation
 *   rewards      DEVICE float64 [K][N]
 *   terminal_obs optional [N][n_obs]: the observation of the last terminal step crossed
 *   *n_done      the number of terminal steps crossed
 *   flags        SCG_BG_AUTORESET | SCG_SC_SERIAL | SCG_SC_LAST_OBS
 * With SCG_BG_AUTORESET a rollout may cross any number of episode ends (the obs row of a
 * terminal step is then the reset observation, as in scg_sc_step); without it a rollout
 * with time_step + n_steps > T fails with SCG_ERR_PAST_HORIZON. Every argument is checked
 * before any HIP call, and a failed check leaves st untouched.
 * Fused: a SCG_SC_KERNEL_NODES config on a state without ledgers runs in launches of up to
 * SCG_SC_ROLLOUT_MAX steps, a block taking its 64 envs through all of a launch's steps with
 * their stocks and heaps in LDS in between (HBM sees the state at the launch's last step and
 * at auto-reset steps). Every other config (the lane, level and staged kernels, and the
 * node-parallel one with build_info ledgers) is stepped by n_steps launches of scg_sc_step
 * into the [k] slices: the same call and results, the per-step speed. */
SCG_API int scg_sc_rollout(const scg_sc_config* cfg, scg_sc_state* st, int32_t n_steps, const float* actions,
                           void* obs, double* rewards, void* terminal_obs, uint32_t flags, int32_t* n_done,
                           void* stream);

/* The observation of the state as it stands, at st->time_step and st->episode: what the
 * reset or step that left this state returned (a pure function of the stocks, the heaps, the
 * time step and the episode's draws), for every kernel's layout. obs: DEVICE [N][n_obs] in
 * the config's obs dtype. After scg_sc_rollout with SCG_SC_LAST_OBS off, or after a
 * checkpoint was restored, this is how a caller learns the current observation.
 * SCG_ERR_NOT_RESET before a reset. */
SCG_API int scg_sc_observe(const scg_sc_config* cfg, const scg_sc_state* st, void* obs, void* stream);

/*
 * Closed-loop rollout: K steps per call as scg_sc_rollout runs them, with each env's action
 * row computed on the device from the observation the env last produced (after an auto-reset
 * inside the call, the reset observation) by a linear policy. For that observation o[0..O) as
 * float32 (a float64 observation element is rounded to float32 first) and float32 parameters
 * W[A][O], b[A]:
 *   z_a = b_a;  for j = 0 .. O-1 ascending:  z_a = z_a + W[a][j] * o_j
 *   act_a = !(z_a >= act_lo) ? act_lo : (z_a > act_hi ? act_hi : z_a)
 * every multiply and add rounded to float32 on its own (no FMA), IEEE arithmetic; a NaN z
 * gives act_lo (csrc/scg_sc_policy.h is the one definition, host and device).
 * Word a*(O+1)+j of a policy is W[a][j] for j < O and b[a] for j == O. params is DEVICE
 * float32 [A*(O+1)][N], env fastest (shared == 0: a policy per env, each word of a wave's 64
 * envs one 256-byte row), or [A*(O+1)] (shared != 0: one policy for every env).
 *
 * The contract: the actions are the formula applied to the previous observation; everything
 * else is what scg_sc_rollout would produce from those actions, bit for bit — observations,
 * rewards, episode_return, final_return and terminal_obs, the error flag, the stocks, heap
 * sizes and live heap entries in storage order, st->time_step and st->episode.
 *   obs_io       DEVICE [N][n_obs], obs dtype, required: on entry the observation the envs last
 *                produced (scg_sc_reset's, the last step's, or scg_sc_observe's), on return
 *                the last step's
 *   act_work     DEVICE float32 [N][n_actions], required scratch (the library allocates
 *                nothing); on return the last step's action rows
 *   actions_out  DEVICE float32 [K][N][n_actions], obs_out DEVICE [K][N][n_obs], rewards_out
 *                DEVICE float64 [K][N]: each optional (NULL) on the fused path; the per-step
 *                path needs rewards_out (a step's reward row has to land somewhere)
 *   reward_sum   DEVICE float64 [N], required: the call's rewards added in step order
 *                (s = 0.0; s = s + r_k), across auto-resets and launches; overwritten
 *   terminal_obs, *n_done  as in scg_sc_rollout
 *   flags        SCG_BG_AUTORESET | SCG_SC_SERIAL
 * Every argument is checked before any HIP call, and a failed check leaves st untouched:
 * SCG_ERR_INVALID (null policy, params, obs_io, act_work or reward_sum; unknown kind; bounds
 * that are NaN, infinite or act_lo > act_hi; n_steps < 0; unknown flags), SCG_ERR_NOT_RESET,
 * and without SCG_BG_AUTORESET SCG_ERR_PAST_HORIZON. n_steps == 0 clears reward_sum.
 * Fused, under scg_sc_rollout's condition (a SCG_SC_KERNEL_NODES config on a state without
 * ledgers): the rollout kernel's block, LDS and launches of up to SCG_SC_ROLLOUT_MAX steps,
 * with the product running from the step's observation tile into the next step's action tile,
 * both in LDS; with no output requested a kept step's only HBM traffic is the parameter reads.
 * Every other config runs an action kernel and scg_sc_step per step: the same results, the
 * per-step speed.
 */
#define SCG_SC_POLICY_LINEAR 1
typedef struct scg_sc_policy {
  int32_t kind;          /* SCG_SC_POLICY_LINEAR */
  int32_t shared;        /* 0: params per env [A*(O+1)][N]; else one policy [A*(O+1)] */
  float act_lo, act_hi;  /* finite, act_lo <= act_hi */
  const float* params;   /* DEVICE float32 */
} scg_sc_policy;

SCG_API int scg_sc_rollout_policy(const scg_sc_config* cfg, scg_sc_state* st, int32_t n_steps,
                                  const scg_sc_policy* policy, void* obs_io, float* act_work, float* actions_out,
                                  void* obs_out, double* rewards_out, double* reward_sum, void* terminal_obs,
                                  uint32_t flags, int32_t* n_done, void* stream);

/*
 * The same closed loop with a one-hidden-layer ReLU policy of hidden width H. For the
 * observation o[0..O) as float32 (as above) and float32 parameters W1[H][O], b1[H], W2[A][H],
 * b2[A]:
 *   h_i = b1_i;  for j = 0 .. O-1 ascending:  h_i = h_i + W1[i][j] * o_j;   h_i = (h_i > 0) ? h_i : +0.0f
 *   z_a = b2_a;  for i = 0 .. H-1 ascending:  z_a = z_a + W2[a][i] * h_i
 *   act_a = !(z_a >= act_lo) ? act_lo : (z_a > act_hi ? act_hi : z_a)
 * every multiply and add rounded to float32 on its own (no FMA); a NaN or -0 pre-activation
 * gives +0, a NaN z gives act_lo (csrc/scg_sc_mlp.h is the one definition, host and device).
 * A policy is Q = H*(O+1) + A*(H+1) words: word i*(O+1)+j is W1[i][j] for j < O and b1[i] for
 * j == O; word H*(O+1) + a*(H+1) + i is W2[a][i] for i < H and b2[a] for i == H. params is
 * DEVICE float32 [Q][N], env fastest (shared == 0), or [Q] (shared != 0).
 *
 * Buffers, flags, contract and error codes are scg_sc_rollout_policy's; SCG_ERR_INVALID also
 * for hidden outside 1..SCG_SC_MLP_MAX_HIDDEN, an unknown activation and reserved != 0.
 * Fused under the linear policy's condition when also H <= 2 * (inbox_size + n_nodes): the
 * hidden units of a block's 64 envs then live in LDS the step leaves idle between its last
 * barrier and the next step's first (the shipment inbox and node cost rows), so the block
 * needs no more LDS than the linear closed loop's. Every other case (it is not an error) runs
 * an action kernel and scg_sc_step per step and needs rewards_out. scg_sc_mlp_fused tells
 * which: 1 fused, 0 per step, -SCG_ERR_INVALID for a bad config, state or hidden; host only,
 * no HIP call.
 */
#define SCG_SC_MLP_MAX_HIDDEN 64
#define SCG_SC_ACT_RELU 1
typedef struct scg_sc_mlp {
  int32_t hidden;        /* 1 .. SCG_SC_MLP_MAX_HIDDEN */
  int32_t activation;    /* SCG_SC_ACT_RELU */
  int32_t shared;        /* 0: params per env [Q][N]; else one policy [Q] */
  int32_t reserved;      /* 0 */
  float act_lo, act_hi;  /* finite, act_lo <= act_hi */
  const float* params;   /* DEVICE float32 */
} scg_sc_mlp;            /* 32 bytes, params at 24 */

SCG_API int scg_sc_rollout_mlp(const scg_sc_config* cfg, scg_sc_state* st, int32_t n_steps, const scg_sc_mlp* mlp,
                               void* obs_io, float* act_work, float* actions_out, void* obs_out,
                               double* rewards_out, double* reward_sum, void* terminal_obs, uint32_t flags,
                               int32_t* n_done, void* stream);
SCG_API int scg_sc_mlp_fused(const scg_sc_config* cfg, const scg_sc_state* st, int32_t hidden);

/*
 * Either closed loop with sampled actions. With z_a the linear policy's or the MLP's output
 * before its clamp, exactly as above, one standard deviation per action and noise the caller
 * supplies (the library draws none):
 *   u_a   = z_a + (std_a * eps[k][n][a])      the product rounded to float32, then the sum; no FMA
 *   act_a = !(u_a >= act_lo) ? act_lo : (u_a > act_hi ? act_hi : u_a)
 * k is the step's index within this call, 0 .. n_steps-1: it counts on across the launches the
 * call is cut into and across auto-resets inside it (a caller who cuts an episode into several
 * calls passes each call its own rows). A NaN u (a NaN z; 0 * inf) gives act_lo. Exactly one of
 * linear / mlp is non-NULL. Everything else is the contract of scg_sc_rollout_policy /
 * scg_sc_rollout_mlp unchanged: actions_out and act_work hold the clamped actions, everything
 * but the actions is what scg_sc_rollout gives for them bit for bit, the buffers, flags and
 * error codes keep their meaning, the fused and the per-step path are chosen as there
 * (scg_sc_mlp_fused answers for the sampled MLP too).
 *   std          DEVICE float32 [n_actions], for every env. The library cannot read it on the
 *                host and takes the values as they are: a negative, infinite or NaN std goes
 *                into the formula like any other float.
 *   noise        DEVICE float32 [K][N][n_actions], K = n_steps: only read
 *   samples_out  DEVICE float32 [K][N][n_actions] or NULL: u, the sample before the clamp (what
 *                the log-probability is taken of). It may be the noise buffer itself: every
 *                element is read and then written by one thread. Any other overlap of the two
 *                is the caller's error.
 * Checked before any HIP call, st left untouched: SCG_ERR_INVALID when both or neither of
 * linear / mlp is given, for a NULL smp, for a NULL std or noise with n_steps > 0, for
 * reserved != 0, and for everything the two deterministic entry points refuse.
 */
typedef struct scg_sc_sampling {
  const float* std;    /* DEVICE float32 [n_actions]: one std per action, for every env */
  const float* noise;  /* DEVICE float32 [K][N][n_actions] */
  float* samples_out;  /* DEVICE float32 [K][N][n_actions] or NULL: u before the clamp; may equal noise */
  int64_t reserved;    /* 0 */
} scg_sc_sampling;     /* 32 bytes */

SCG_API int scg_sc_rollout_sampled(const scg_sc_config* cfg, scg_sc_state* st, int32_t n_steps,
                                   const scg_sc_policy* linear, const scg_sc_mlp* mlp, const scg_sc_sampling* smp,
                                   void* obs_io, float* act_work, float* actions_out, void* obs_out,
                                   double* rewards_out, double* reward_sum, void* terminal_obs, uint32_t flags,
                                   int32_t* n_done, void* stream);

/*
 * The sampled closed loop with the noise drawn on the device: scg_sc_rollout_sampled with
 * eps[k][n][a] not read from memory but computed where it is used. Element (row k, env id e,
 * action a) of the noise of a 64-bit seed is the project's own float32 standard normal
 * (csrc/scg_normal.h, restated in NumPy by tests/noise_ref.py):
 *   blk      = philox4x32_10(ctr = (e, k, a >> 2, SCG_STREAM_SC_NOISE), key = (seed & 0xffffffff, seed >> 32))
 *   (w1, w2) = (blk.x, blk.y) for pair (a >> 1) & 1 == 0, (blk.z, blk.w) for pair 1
 *   m = (w1 >> 8) + 1, u = m * 2^-24;   v = w2 >> 8, theta = 2 pi v * 2^-24;   r = sqrt(-2 ln u)
 *   eps = r cos(theta) for even a, r sin(theta) for odd a
 * with r, cos and sin from float32 + - * / sqrt alone, each rounded on its own (no FMA, no
 * library function), so the host, the device and NumPy give the same bits; |eps - eps64| <= 7.9e-7
 * against the float64 Box-Muller of the same (u, theta). The eps of step j of the call is
 * element (row0 + j, env_offset + n, a): a sharded batch draws what the unsharded one draws, and
 * a caller who cuts an episode into several calls passes each its own row0.
 *   std          DEVICE float32 [n_actions], as scg_sc_sampling's
 *   samples_out  DEVICE float32 [K][N][n_actions] or NULL: u before the clamp
 *   seed         the noise's seed (its own: not the state's)
 *   row0         the global row index of the call's first step
 * Contract, flags, error codes and the choice of the fused or the per-step path are those of
 * scg_sc_rollout_sampled. Checked before any HIP call, st left untouched: SCG_ERR_INVALID for a
 * NULL draw, for a NULL std with n_steps > 0, for reserved != 0, for row0 + n_steps > 2^32, and
 * for everything scg_sc_rollout_sampled refuses.
 */
typedef struct scg_sc_noise_draw {
  const float* std;    /* DEVICE float32 [n_actions] */
  float* samples_out;  /* DEVICE float32 [K][N][n_actions] or NULL */
  uint64_t seed;
  uint32_t row0;
  uint32_t reserved;   /* 0 */
} scg_sc_noise_draw;   /* 32 bytes */

SCG_API int scg_sc_rollout_drawn(const scg_sc_config* cfg, scg_sc_state* st, int32_t n_steps,
                                 const scg_sc_policy* linear, const scg_sc_mlp* mlp, const scg_sc_noise_draw* draw,
                                 void* obs_io, float* act_work, float* actions_out, void* obs_out,
                                 double* rewards_out, double* reward_sum, void* terminal_obs, uint32_t flags,
                                 int32_t* n_done, void* stream);

/* Rows row0 .. row0 + n_rows - 1 of that noise for the state's envs, into out DEVICE float32
 * [n_rows][N][n_actions] (the learning pass regenerates what the rollout drew). SCG_ERR_INVALID
 * for a NULL out with n_rows > 0, n_rows < 0 or row0 + n_rows > 2^32. */
SCG_API int scg_sc_noise_fill(const scg_sc_config* cfg, const scg_sc_state* st, uint64_t seed, uint32_t row0,
                              int32_t n_rows, float* out, void* stream);

/* Testing hook: the device transform on the caller's Philox word pairs, words DEVICE uint32
 * [n][2] = (w1, w2) into out DEVICE float32 [n][2] = (r cos, r sin). */
SCG_API int scg_noise_from_words(const uint32_t* words, float* out, int64_t n, void* stream);

/* The per-episode tables scg_sc_step draws (for tests): demand DEVICE int32
 * [N][T+1][R][P], leadtimes DEVICE int32 [N][T][n_leadtimes] (NULL when deterministic). */
SCG_API int scg_sc_draw_tables(const scg_sc_config* cfg, const scg_sc_state* st, uint32_t episode,
                               int32_t* demand, int32_t* leadtimes, void* stream);

/*
 * Step server for the drop-in SupplyChainEnv (one env stepped per Python call,
 * supplychain_env.py:703-748): one resident block of the node-parallel kernel's shape (a wave
 * per node) polls a host-mapped mailbox and runs the node-parallel step of tile 0 for each
 * posted step, on the state and buffers the launch arguments named when it started — the
 * config's kernel must be SCG_SC_KERNEL_NODES, float64 observations, no ledgers, up to 64
 * envs. The same protocol as the BeerGame server: post the step (its time, flags and
 * episode travel in the request, and one env's action row too), wait for the answer word;
 * the block exits on scg_sc_server_stop or after idle_us without a request, and the next post
 * launches it again (with the then-current state pointers and action / obs / reward
 * buffers). Between two steps of an episode the block keeps the env's state in its LDS (it
 * still writes every step's state back to memory), so a step reads no state from memory;
 * a reset (a new episode) or `reload` makes it read the state again.
 */
typedef struct scg_sc_server_box { /* host-mapped (hipHostMalloc mapped + coherent), 192 B */
  /* the request: two 64-byte lines, which the block reads in one load */
  uint32_t req_seq;   /* request number                                                   */
  int32_t cmd;        /* 0: step                                                          */
  int32_t t;          /* the step's time (1..T)                                           */
  int32_t flags;      /* bit0 terminal (as scg_sc_step's kernel flags)                    */
  uint32_t episode;   /* the state's episode                                              */
  uint32_t opts;      /* bit0: env 0's action row travels in action[] (one env, A <= 16);
                         bit1: read the state from memory (not the block's LDS copy)      */
  int32_t pad0;
  uint32_t check;     /* scg mixing hash of the two lines' other 31 words                 */
  int32_t pad1[8];
  float action[16];   /* line 1: the inline action row                                    */
  /* the answer, on its own line */
  uint32_t done_seq;  /* the last request served (written by the block)                   */
  uint32_t exit_req;  /* the block exits when this differs from its launch value          */
  uint32_t exit_seq;  /* written by the block as it exits: the exit_req it saw last       */
  uint32_t pad2[13];
} scg_sc_server_box;

typedef struct scg_sc_server {
  scg_sc_server_box* box_host; /* the mailbox's host address                              */
  scg_sc_server_box* box_dev;  /* its device address                                      */
  void* stream;                /* a non-blocking stream of the caller's (high priority)   */
  const float* action;         /* DEVICE-visible float32 [N][A]                           */
  const float* action_host;    /* its host address, or NULL: with one env of A <= 16 the
                                  row is copied into the request (no read across PCIe)   */
  void* obs;                   /* DEVICE-visible float64 [N][O]                           */
  double* reward;              /* DEVICE-visible float64 [N]                              */
  int32_t idle_us;             /* the block exits after this long without a request       */
  int32_t check_us;            /* a waiting step checks this often for a gone block (0: 2 s) */
  int32_t reload;              /* set by the caller when something else wrote the state (it
                                  has no launch of its own on it otherwise): the next post
                                  makes the block read it from memory; cleared by the post */
  /* host bookkeeping: zero before first use */
  int32_t running;
  uint32_t seq;                /* the request last posted                                 */
  int32_t t;                   /* the step it runs                                        */
  int32_t done;                /* that step is the terminal one                           */
  int32_t relaunches;          /* blocks a wait launched again (block gone)               */
  int64_t last_ns;
  int64_t launches;
} scg_sc_server;

/* Post step(action) of the st->n_envs <= 64 envs (launches the block if needed). */
SCG_API int scg_sc_server_post(const scg_sc_config* cfg, scg_sc_state* st, scg_sc_server* sv);
/* Wait for it: SCG_OK (st->time_step advanced, *done), SCG_PENDING after spin_us (< 0: no
 * limit; the wait then fails after 60 s), or an error. */
SCG_API int scg_sc_server_wait(const scg_sc_config* cfg, scg_sc_state* st, scg_sc_server* sv, int64_t spin_us,
                               int32_t* done);
/* post + wait without limit. */
SCG_API int scg_sc_server_step(const scg_sc_config* cfg, scg_sc_state* st, scg_sc_server* sv, int32_t* done);
/* Ask the block to exit and wait for it (a no-op when it is not running). */
SCG_API int scg_sc_server_stop(scg_sc_server* sv);

/* Testing hook: cap the node-parallel kernel's persistent grid at `blocks` blocks (0, the
 * default: as many as the device holds at once), so a small batch runs several 64-env tiles
 * per block and the next-tile prefetch runs (scg_sc_nodes.hip). Returns the previous cap. */
SCG_API int scg_sc_nodes_max_blocks(int32_t blocks);

/* Testing hook: the fused scg_sc_rollout launches at most `steps` steps at a time (0, the
 * default, and anything larger: SCG_SC_ROLLOUT_MAX), so a short rollout crosses launch
 * boundaries. Returns the previous value. */
SCG_API int scg_sc_rollout_chunk(int32_t steps);

#ifdef __cplusplus
}
#endif

#endif /* SCGPU_H */
