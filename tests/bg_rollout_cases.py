"""The games of the BeerGame fused-rollout fuzz (tests/test_gpu_bg_rollout_fuzz.py on the device,
tests/test_bg_rollout_fuzz_inputs.py on the host): a seeded generator random_game(L, ring, seed)
and the table of games the tests run, written down so that a change to the generator fails a host
test instead of silently moving the device tests.

bg_rollout_kernel<L, Variant, Source, kLds> is one template compiled per level count, variant,
action source and ring placement; load_row / store_row vectorise differently for L % 4 == 0,
L % 2 == 0 and odd L; the ring moves from LDS to HBM at ring_slots * L > 64. The main grid is, for
every L in 1..8, the last ring that fits LDS (R = 64 // L) and the first that does not (R + 1),
each as a BeerGameVecEnv and a BeerGame2VecEnv game under the open loop and the four closed
loops. Two tiny games (T = 1 and T = 2: every week, or every second, is an auto-reset) run the
same loops; one game each at L = 9..16 runs the open loop only (the closed loops stop at 8 levels).

Sizes of every case: 260 envs (one full 256-lane block and a 4-lane tail; 260 * L % 4 == 0, so a
twin's step() runs the slab step kernel), K = 2 T + 3 weeks per call (two auto-resets, ending
mid-episode; past the 128-week launch cut at L = 1 and L = 2), envs 0, 63, 64, 255, 256 and 259
against the oracle.

The expected side is one CPU oracle per sampled env in lock step with auto-reset
(oracle/beergame.py, demand and delay tables from oracle/philox.py, oracle/poisson.py and
oracle/gen_golden_bg2.uniform_table), the actions from tests/bg_policy_ref.py,
tests/bg_local_ref.py and tests/bg_mlp_ref.py. It needs no GPU, is computed once per case and
shared, read only."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import bg_local_ref
import bg_mlp_ref
import bg_policy_ref

N_ENVS = 260
SAMPLE = (0, 63, 64, 255, 256, 259)
SHIFT = 4
LOOPS = ("open", "linear", "local", "mlp", "mlp-sampled")
CLOSED = LOOPS[1:]
POISSON_LAMBDA = 6.0
DEMAND_HI = 16                    # fixed lists and uniform draws lie in 0..15
MAX_STOCK, PENALTY = 20, 3        # BeerGame2VecEnv: a penalty the games' stocks reach
POLICY_LEVELS = 8                 # SCG_BG_POLICY_MAX_LEVELS
LEVEL_LIMIT_MESSAGE = "rollout_policy supports up to 8 levels"
LDS_BYTES = 64 * 1024
F32 = np.float32

# name: L-ring. R: ring_slots scg_bg_prepare must derive (delay list: longest delay + 1; stochastic:
# delay_hi). T: the horizon random_game draws. demand1: BeerGameVecEnv's demand mode. demand2 /
# delays2: BeerGame2VecEnv's. H / recipe: the MLP's hidden width and parameter recipe
# (test_gpu_bg_mlp_policy.py::_network). seed: one at which every condition of
# tests/test_bg_rollout_fuzz_inputs.py holds for every loop of both variants.
Game = namedtuple("Game", "name L ring R T seed demand1 demand2 delays2 H recipe")
MAIN = [
    Game("1-lds", 1, "lds", 64, 68, 20, "fixed", "fixed", "stochastic", 64, "gauss"),
    Game("1-hbm", 1, "hbm", 65, 69, 0, "poisson", "uniform", "list", 33, "tie"),
    Game("2-lds", 2, "lds", 32, 64, 3, "table", "fixed", "list", 16, "gauss"),
    Game("2-hbm", 2, "hbm", 33, 65, 16, "fixed", "uniform", "stochastic", 20, "tie"),
    Game("3-lds", 3, "lds", 21, 24, 1, "poisson", "fixed", "stochastic", 33, "gauss"),
    Game("3-hbm", 3, "hbm", 22, 25, 0, "table", "uniform", "list", 7, "tie"),
    Game("4-lds", 4, "lds", 16, 18, 0, "fixed", "fixed", "list", 48, "gauss"),
    Game("4-hbm", 4, "hbm", 17, 20, 10, "poisson", "uniform", "stochastic", 1, "tie"),
    Game("5-lds", 5, "lds", 12, 14, 0, "table", "fixed", "stochastic", 16, "gauss"),
    Game("5-hbm", 5, "hbm", 13, 17, 48, "fixed", "uniform", "list", 64, "tie"),
    Game("6-lds", 6, "lds", 10, 13, 3, "poisson", "fixed", "list", 1, "gauss"),
    Game("6-hbm", 6, "hbm", 11, 14, 6, "table", "uniform", "stochastic", 33, "tie"),
    Game("7-lds", 7, "lds", 9, 13, 0, "fixed", "fixed", "stochastic", 2, "gauss"),
    Game("7-hbm", 7, "hbm", 10, 14, 0, "poisson", "uniform", "list", 16, "tie"),
    Game("8-lds", 8, "lds", 8, 11, 0, "table", "fixed", "list", 64, "gauss"),
    Game("8-hbm", 8, "hbm", 9, 11, 3, "fixed", "uniform", "stochastic", 5, "tie"),
]
TINY = [
    Game("5-T1", 5, "lds", 3, 1, 15, "poisson", "uniform", "list", 16, "gauss"),
    Game("6-T2", 6, "lds", 3, 2, 2147, "table", "fixed", "list", 33, "tie"),
]
OPEN_ONLY = [
    Game("9-lds", 9, "lds", 7, 11, 0, "fixed", "fixed", "list", None, None),
    Game("10-hbm", 10, "hbm", 7, 10, 0, "poisson", "uniform", "stochastic", None, None),
    Game("11-lds", 11, "lds", 5, 7, 0, "table", "fixed", "stochastic", None, None),
    Game("12-hbm", 12, "hbm", 6, 10, 0, "fixed", "uniform", "list", None, None),
    Game("13-lds", 13, "lds", 4, 8, 0, "poisson", "fixed", "list", None, None),
    Game("14-hbm", 14, "hbm", 5, 9, 0, "table", "uniform", "stochastic", None, None),
    Game("15-lds", 15, "lds", 4, 7, 0, "fixed", "fixed", "stochastic", None, None),
    Game("16-hbm", 16, "hbm", 5, 9, 0, "poisson", "uniform", "list", None, None),
]
CLOSED_GAMES = MAIN + TINY
GAMES = CLOSED_GAMES + OPEN_ONLY
BY_NAME = {g.name: g for g in GAMES}
VARIANTS = (1, 2)


def ring_slots(L, ring):
    """The last ring whose block share (R * L * 256 lanes * 4 B) fits 64 KiB, or one slot more."""
    return LDS_BYTES // 1024 // L + (ring == "hbm")


def random_game(L, ring, seed, T=None):
    """A game of L levels whose delay list needs ring_slots(L, ring) slots, drawn from `seed` in the
    ranges of test_gpu_beergame_fuzz.py::_config: initial inventory in -5..39 (one level at 30 or
    more, and where L > 1 one below zero), initial shipment and orders values in 0..11, costs in
    0..5, weekly delays in 0..4 with a zero among them. On top: the longest delay D = R - 1 at week
    1 or 2, the horizon T in D + 3..D + 5 (T >= 63 at L = 2, so that 2 T + 3 weeks pass the
    128-week launch cut), a later week that ships into the long shipment's arrival week (MODE_ADD)
    and a last week whose shipment lands past T (MODE_DROP). A given T (the tiny games) keeps the
    plain draws only. `delays` and `demand` have one entry per week 1..T."""
    r = np.random.RandomState(7000 + 131 * seed + 17 * L + (ring == "hbm"))
    tiny = T is not None
    R = 3 if tiny else ring_slots(L, ring)
    D = R - 1
    small = min(4, D - 1) if not tiny else D
    if not tiny:
        T = max(D + 3 + int(r.randint(0, 3)), 63 + int(r.randint(0, 3)) if L == 2 else 0)
    delays = r.randint(0, small + 1, size=T)
    inventory = r.randint(-5, 40, size=L)
    inventory[int(r.randint(L))] = int(r.randint(30, 40))
    if L > 1:
        inventory[(int(np.argmax(inventory)) + 1 + int(r.randint(L - 1))) % L] = int(r.randint(-5, 0))
    game = dict(levels=L, ring_slots=R, weeks=T, initial_inventory=[int(x) for x in inventory],
                initial_shipment_value=int(r.randint(0, 12)), initial_orders_value=int(r.randint(0, 12)),
                inv_cost=int(r.randint(0, 6)), backlog_cost=int(r.randint(0, 6)),
                demand=[int(x) for x in r.randint(0, DEMAND_HI, size=T)])
    if tiny:
        delays[0] = D                                  # the ring's size; T = 1: it lands past T
        if T > 1:
            delays[1] = 0
    else:
        long_week = 1 + int(r.randint(0, 2))
        arrival = long_week + D
        d2 = 1 + int(r.randint(0, small))
        zero_week = int(r.choice([w for w in range(1, T) if w not in (long_week, arrival - d2)]))
        delays[long_week - 1] = D
        delays[arrival - d2 - 1] = d2                  # week arrival - d2 ships into week `arrival` too
        delays[zero_week - 1] = 0
        delays[T - 1] = 1 + int(r.randint(0, small))   # lands past T
        game.update(long_week=long_week, arrival=arrival)
    game["delays"] = [int(d) for d in delays]
    return game


@lru_cache(maxsize=None)
def game_of(g):
    return random_game(g.L, g.ring, g.seed, T=g.T if g in TINY else None)


def weeks_per_call(g):
    return 2 * g.T + 3


def cuts(g):
    """The split calls' two cuts: a seeded mid-episode week of the first episode (week 1 of the
    T = 1 game, which has none) and the first week after the first auto-reset."""
    return 1 + (g.seed + 3 * g.L) % max(g.T - 1, 1), g.T + 1


def loops_of(g):
    return LOOPS if g.L <= POLICY_LEVELS else LOOPS[:1]


def case_ids():
    return [(g, v, loop) for g in GAMES for v in VARIANTS for loop in loops_of(g)]


def case_id(g, variant, loop):
    return f"{g.name}-v{variant}-{loop}"


def clip_of(variant, loop):
    """The integer policies' clamps are the existing tests': BeerGameVecEnv's order increments in
    (-3, 5), BeerGame2VecEnv's default (0, max_order). The MLP's is (6, 10), two either side of
    where both recipes centre b2: six envs must reach both bounds and the interior, at one level
    too, where four inputs move z little (the existing cases' 300 envs reach (-3, 12) and (0, 30))."""
    if loop.startswith("mlp"):
        return 6, 10
    return (0, 30) if variant == 2 else (-3, 5)


# ---- demand and delays, as the kernels draw them -----------------------------------------------------------
def table_demand(g):
    """BeerGameVecEnv's per-env demand table int32 [T, N], drawn on the host."""
    return np.random.RandomState(900 + g.seed + 31 * g.L).randint(0, DEMAND_HI + 1, size=(g.T, N_ENVS)).astype(np.int32)


@lru_cache(maxsize=None)
def _demand(g, variant, episode):
    """int64 [N, T]: the customer demand of every env in `episode`."""
    from oracle.gen_golden_bg2 import STREAM_BG2_DEMAND, uniform_table
    from oracle.philox import STREAM_DEMAND, draw_words
    from oracle.poisson import poisson_invert, poisson_thresholds
    mode = g.demand1 if variant == 1 else g.demand2
    if mode == "fixed":
        return np.tile(np.asarray(game_of(g)["demand"], dtype=np.int64), (N_ENVS, 1))
    if mode == "table":
        return table_demand(g).T.astype(np.int64)
    if mode == "poisson":
        words = draw_words(g.seed, np.arange(N_ENVS), episode, g.T, STREAM_DEMAND)
        return poisson_invert(words, poisson_thresholds(POISSON_LAMBDA)).astype(np.int64)
    return uniform_table(g.seed, N_ENVS, episode, g.T, 0, DEMAND_HI, STREAM_BG2_DEMAND)


@lru_cache(maxsize=None)
def _delays2(g, episode):
    from oracle.gen_golden_bg2 import STREAM_BG2_DELAY, uniform_table
    return uniform_table(g.seed, N_ENVS, episode, g.T, 0, g.R, STREAM_BG2_DELAY)


def stochastic(g, variant):
    return variant == 2 and g.delays2 == "stochastic"


def make_oracle(g, variant, env, episode):
    """A fresh oracle of env `env` (its global id) for `episode`."""
    from oracle.beergame import BeerGame2Oracle, BeerGameOracle
    game = game_of(g)
    demand = _demand(g, variant, episode)[env]
    if variant == 1:
        return BeerGameOracle(dict(levels=g.L, initial_inventory=game["initial_inventory"], customer_demand=demand,
                                   shipment_delays=game["delays"], inv_cost=game["inv_cost"],
                                   backlog_cost=game["backlog_cost"],
                                   initial_shipment_value=game["initial_shipment_value"],
                                   initial_orders_value=game["initial_orders_value"]))
    delays = _delays2(g, episode)[env].tolist() if stochastic(g, variant) else game["delays"]
    return BeerGame2Oracle(max_stock=MAX_STOCK, weeks=g.T, levels=g.L, customer_demand=demand,
                           initial_inventory=game["initial_inventory"], inv_cost=game["inv_cost"],
                           backlog_cost=game["backlog_cost"], exceeded_capacity_penalty=PENALTY, shipment_delays=delays,
                           initial_shipment=game["initial_shipment_value"], initial_orders=game["initial_orders_value"])


# ---- the inputs of a case, whole batch ---------------------------------------------------------------------
@lru_cache(maxsize=None)
def inputs(g, variant, loop):
    """What the device call is given, for all N envs; shared, read only. open: actions int32
    [K, N, L]. linear / local: (W, b) of the existing tests' recipes. mlp: (w1, b1, w2, b2), and
    sampled std [L] (one element exactly 0 where L > 1) and noise [K, N, L]."""
    K, L = weeks_per_call(g), g.L
    if loop == "open":
        lo, hi = (-2, 6) if variant == 1 else (0, 30)
        acts = np.random.RandomState(300 + g.seed + 7 * L + variant).randint(lo, hi + 1, size=(K, N_ENVS, L))
        return dict(actions=acts.astype(np.int32))
    if loop == "linear":
        from test_gpu_bg_policy_rollout import _params
        W, b = _params(L, n=N_ENVS, seed=1100 + g.seed + variant)
        return dict(W=W, b=b)
    if loop == "local":
        from test_gpu_bg_local_policy import _params
        W, b = _params(L, n=N_ENVS, seed=2300 + g.seed + variant)
        return dict(W=W, b=b)
    from test_gpu_bg_mlp_policy import _network
    *net, std, noise = _network(dict(L=L, H=g.H, K=K, n=N_ENVS, recipe=g.recipe, seed=g.seed + variant))
    out = dict(net=tuple(net))
    if loop == "mlp-sampled":
        std = std.copy()
        if L > 1:
            std[(g.seed + variant) % L] = F32(0.0)
        out.update(std=std, noise=noise)
    return out


# ---- the expected side --------------------------------------------------------------------------------------
def _oracles_class():
    from test_gpu_bg_mlp_policy import MlpOracles

    class Run(MlpOracles):
        """MlpOracles on the sampled envs, which also keeps what the vec env keeps across an
        auto-reset (the returns, the order history's stale rows) and the largest value seen."""

        def __init__(self, g, variant):
            super().__init__(lambda i, ep: make_oracle(g, variant, SAMPLE[i], ep), len(SAMPLE),
                             max_stock=MAX_STOCK if variant == 2 else 0)
            self.g, self.variant = g, variant
            n, L = len(SAMPLE), g.L
            self.hist = np.zeros((n, L, g.T + 1), dtype=np.int64)
            self.ret, self.final_ret = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
            self.largest, self.penalty, self.ends = 0, False, 0
            self.linear_seen = dict(lo=False, hi=False, inside=False, negative=False)

        def reset(self):
            obs = super().reset()
            self.last_obs = obs
            self.hist[:, :, 0] = self.o[0].orders_value
            return obs

        def act_linear(self, W, b, lo, hi):
            z = bg_policy_ref.pre_shift(W, b, self.last_obs)
            a = bg_policy_ref.actions(W, b, self.last_obs, SHIFT, lo, hi)
            assert np.array_equal(a, np.clip(z >> SHIFT, lo, hi))
            for k, v in dict(lo=(a == lo).any(), hi=(a == hi).any(), inside=((a > lo) & (a < hi)).any(),
                             negative=(z < 0).any()).items():
                self.linear_seen[k] = self.linear_seen[k] or bool(v)
            return a

        def step(self, actions):
            stepped = self.o
            obs, rew = super().step(actions)
            for i, o in enumerate(stepped):
                self.hist[i, :, o.week] = o.orders_placed
                ledgers = [o.inventory_costs, o.backlog_costs] + ([o.penalty_costs] if self.variant == 2 else [])
                self.largest = max([self.largest] + [int(np.abs(np.asarray(x)).max()) for x in
                                                     [o.inventory, o.backlog, o.orders_placed, o.shipments] + ledgers])
                self.penalty = self.penalty or (self.variant == 2 and bool(np.any(o.penalty_costs)))
            self.ret += rew
            self.largest = max(self.largest, int(np.abs(obs).max()), int(np.abs(rew).max()), int(np.abs(self.ret).max()))
            if stepped[0].week == stepped[0].max_weeks:   # the vec env's auto-reset
                self.final_ret, self.ret = self.ret, np.zeros_like(self.ret)
                self.hist[:, :, 0] = self.o[0].orders_value
                self.ends += 1
            self.last_obs = obs
            return obs, rew

        def dead_row_is_not_zero(self):
            """Whether some ring row outside the live mask is non-zero now: a week v <= w that has
            arrived, within the last R weeks, whose slot v % R no live week maps to."""
            o, R = self.o[0], self.g.R
            live = {v % R for v in bg_local_ref.live_weeks(o.shipment_delays.tolist(), o.max_weeks, o.week)}
            return any(v % R not in live and any(np.any(x.shipments[v]) for x in self.o)
                       for v in range(max(1, o.week - R + 1), o.week + 1))

        def ledgers(self):
            names = ("inventory_costs", "backlog_costs") + (("penalty_costs",) if self.variant == 2 else ())
            return {k: np.stack([np.asarray(getattr(o, k)).astype(np.int64) for o in self.o]) for k in names}

    return Run


_REFS = {}


def reference(g, variant, loop):
    """The expected streams and final state of the sampled envs over the case's K weeks from reset,
    and what the run exercised: a dict of arrays indexed [k, i] or [i] with i the index into
    SAMPLE. Computed once per case and shared by the tests; read only."""
    key = (g, variant, loop)
    if key in _REFS:
        return _REFS[key]
    K, L, idx = weeks_per_call(g), g.L, list(SAMPLE)
    inp = inputs(g, variant, loop)
    lo, hi = clip_of(variant, loop)
    run = _oracles_class()(g, variant)
    out = dict(reset_obs=run.reset(), dead_row=False)
    feats, us, acts, obs, rew = [], [], [], [], []
    cut = cuts(g)[0]
    for k in range(K):
        if k == cut and not stochastic(g, variant) and run.ends == 0:
            out["dead_row"] = run.dead_row_is_not_zero()
        if loop == "open":
            a = inp["actions"][k, idx]
        elif loop == "linear":
            a = run.act_linear(inp["W"][idx], inp["b"][idx], lo, hi)
        elif loop == "local":
            feats.append(run.features().astype(np.int32))
            a = run.act(inp["W"][idx], inp["b"][idx], lo, hi)
        else:
            sampled = loop == "mlp-sampled"
            f, u, a = run.act_mlp(inp["net"], lo, hi, inp["std"], inp["noise"][k, idx]) if sampled else \
                run.act_mlp(inp["net"], lo, hi)
            feats.append(f)
            us.append(u)
        o, r = run.step(a)
        acts.append(np.asarray(a, dtype=np.int32)), obs.append(o), rew.append(r)
    out.update(actions=np.stack(acts), obs=np.stack(obs), rewards=np.stack(rew), reward_sum=np.stack(rew).sum(0),
               features=np.stack(feats) if feats else None, samples=np.stack(us) if loop == "mlp-sampled" else None,
               inventory=np.stack([o.inventory for o in run.o]), backlog=np.stack([o.backlog for o in run.o]),
               orders_placed=np.stack([o.orders_placed for o in run.o]), episode_return=run.ret, final_return=run.final_ret,
               all_orders_placed=run.hist, week=run.o[0].week, episode=run.ep, ends=run.ends, largest=run.largest,
               penalty=run.penalty, seen=dict(run.seen), mlp_seen=dict(run.mlp_seen), linear_seen=dict(run.linear_seen),
               final_features=run.features().astype(np.int32), **run.ledgers())
    out["largest"] = max(out["largest"], int(np.abs(out["reward_sum"]).max()),
                         int(np.abs(out["features"]).max()) if feats else 0)
    _REFS[key] = out
    return out


def missing(g, variant, loop):
    """The conditions of tests/test_bg_rollout_fuzz_inputs.py the case's reference misses (none, in
    the table): names, for the message."""
    ref, out = reference(g, variant, loop), []
    if ref["largest"] >= 2 ** 31 - 1:
        out.append("int32")
    if g.T == 1:
        ok = ref["ends"] >= 2 and ref["week"] == 0
    else:
        ok = ref["ends"] >= 2 and 0 < ref["week"] < g.T
    if not ok:
        out.append("episodes")
    if variant == 2 and not ref["penalty"]:
        out.append("penalty")
    if loop == "open":
        return out
    seen = dict(linear=ref["linear_seen"], local=ref["seen"]).get(loop, ref["mlp_seen"])
    out += [k for k in ("lo", "hi", "inside") if not seen[k]]
    if loop in ("linear", "local") and not seen["negative"]:
        out.append("negative")
    if loop != "linear":
        # one level has no level above it; with T = 1 every action is taken just after a reset: no backlog yet
        out += [k for k in ("transit",) + (("upstream",) if g.L > 1 and g.T > 1 else ()) if not seen[k]]
        if not stochastic(g, variant) and g.T > 1 and not ref["dead_row"]:
            out.append("dead_row")
    if loop.startswith("mlp"):
        out += [k for k in ("dead", "live") if not seen[k]]
        if not seen["tie" if g.recipe == "tie" else "order"]:
            out.append("tie" if g.recipe == "tie" else "order")
    if loop == "mlp-sampled":
        std = inputs(g, variant, loop)["std"]
        if not ((std > 0).any() and (g.L == 1 or (std == 0).sum() == 1)):
            out.append("std")
    return out


def prepare(g, variant):
    """scg_bg_prepare of the game (host only): (ring_slots, plan words of weeks 1..T)."""
    import ctypes

    from gym_supplychain_amd import _native as nat
    game, T = game_of(g), g.T
    delays = (ctypes.c_int32 * (T + 1))(2, *game["delays"])
    demand = (ctypes.c_int32 * T)(*game["demand"])
    plan = (ctypes.c_int32 * (T + 1))()
    c = nat.BgConfig()
    c.levels, c.max_weeks = g.L, T
    c.inv_cost, c.backlog_cost = game["inv_cost"], game["backlog_cost"]
    c.initial_shipment_value, c.initial_orders_value = game["initial_shipment_value"], game["initial_orders_value"]
    for i, v in enumerate(game["initial_inventory"]):
        c.initial_inventory[i] = v
    c.demand_mode = nat.SCG_DEMAND_FIXED
    c.customer_demand = ctypes.cast(demand, ctypes.c_void_p)
    if variant == 2:
        c.variant, c.max_stock, c.exceeded_capacity_penalty = 2, MAX_STOCK, PENALTY
        if stochastic(g, variant):
            c.stochastic_delays, c.delay_lo, c.delay_hi = 1, 0, g.R
            delays = (ctypes.c_int32 * (T + 1))(2, *([0] * T))   # as _Bg2Config fills them: [2] + [low] * T
    c.shipment_delays = ctypes.cast(delays, ctypes.c_void_p)
    c.plan = ctypes.cast(plan, ctypes.c_void_p)
    rc = nat.lib.scg_bg_prepare(ctypes.byref(c))
    assert rc == 0, nat.last_error()
    return c.ring_slots, list(plan)[1:]


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)
