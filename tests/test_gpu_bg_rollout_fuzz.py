"""Fuzz of the fused BeerGame rollouts on the device: rollout() and the four closed loops of
rollout_policy() (linear, local, MLP deterministic and sampled) on the games of
tests/bg_rollout_cases.py. bg_rollout_kernel is one template compiled per level count, variant,
action source and ring placement; the hand-picked game of the closed loops' own tests reaches
L = 1, 2, 3, 4 and 8 with delays of at most 9. These games run every L in 1..8 under every loop
and both variants with the ring at the last size that fits LDS and at the first that does not
(64/65 slots at L = 1 down to 8/9 at L = 8: the live mask's bit 63, a ring walked 64 rows), with
drawn costs, pipeline values and negative inventory, horizons of 1 and 2 weeks, and the open loop
at L = 9..16 with auto-reset inside the call.

The expected side is the oracle on envs 0, 63, 64, 255, 256 and 259 (tests/bg_rollout_cases.py
reference(): computed on the host, once per case, shared, read only; its conditions are checked
by tests/test_bg_rollout_fuzz_inputs.py), and across the whole batch a twin env stepped K times
with step() on the actions the call took (the slab step kernel, or bg2_step_kernel), the NumPy
formula of each closed loop on the twin's observation or policy_features(), and the same K weeks
as three calls. Every comparison is exact, the samples on the bits. A game the library refuses
fails its test.

Sizes: 260 envs (a full 256-lane block and a 4-lane tail), K = 2 T + 3 weeks per call (two
auto-resets, ending mid-episode; 131 to 141 weeks at L = 1 and 2, past the 128-week launch cut)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bg_local_ref
import bg_mlp_ref
import bg_policy_ref
import bg_rollout_cases as rc
from test_gpu_bg_local_policy import DEV, _assert_refused_then_steps_on, _assert_same_state

pytestmark = pytest.mark.gpu
IDX = list(rc.SAMPLE)
STREAMS = ("actions", "obs", "rewards", "features", "samples")


def _cases():
    return [pytest.param(g, v, loop, id=rc.case_id(g, v, loop)) for g, v, loop in rc.case_ids()]


def _padded(weeks):
    return weeks + [0] * max(3 - len(weeks), 0)


def _env(g, variant):
    from gym_supplychain_amd import BeerGame2VecEnv, BeerGameVecEnv
    game = rc.game_of(g)
    if variant == 2:
        # (a list of two entries would be read as a (low, high) range, as the reference reads it: the
        # tiny games' lists are padded to three entries, which no week reaches)
        return BeerGame2VecEnv(rc.N_ENVS, max_stock=rc.MAX_STOCK, weeks=g.T, levels=g.L,
                               customer_demand=_padded(game["demand"]) if g.demand2 == "fixed" else (0, rc.DEMAND_HI),
                               initial_inventory=game["initial_inventory"], inv_cost=game["inv_cost"],
                               backlog_cost=game["backlog_cost"], exceeded_capacity_penalty=rc.PENALTY,
                               shipment_delays=(0, g.R) if g.delays2 == "stochastic" else _padded(game["delays"]),
                               initial_shipment=game["initial_shipment_value"], initial_orders=game["initial_orders_value"],
                               seed=g.seed, device=DEV, track_history=True)
    info = dict(levels=g.L, initial_inventory=game["initial_inventory"], customer_demand=game["demand"],
                shipment_delays=game["delays"], inv_cost=game["inv_cost"], backlog_cost=game["backlog_cost"],
                initial_shipment_value=game["initial_shipment_value"], initial_orders_value=game["initial_orders_value"])
    demand = torch.as_tensor(rc.table_demand(g), device=DEV) if g.demand1 == "table" else g.demand1
    return BeerGameVecEnv(rc.N_ENVS, info, demand=demand, poisson_lambda=rc.POISSON_LAMBDA, seed=g.seed, device=DEV,
                          track_history=True)


def _np(t):
    return None if t is None else t.cpu().numpy().copy()


def _call(env, g, variant, loop, k0, k1):
    """Weeks k0..k1 of the case on env: every stream as a NumPy array (None where the loop has none)."""
    inp = rc.inputs(g, variant, loop)
    if loop == "open":
        acts = torch.as_tensor(inp["actions"][k0:k1], device=DEV)
        obs, rew = env.rollout(acts)
        return SimpleNamespace(actions=_np(acts), obs=_np(obs), rewards=_np(rew), features=None, samples=None,
                               reward_sum=_np(rew).astype(np.int64).sum(0))
    kw = dict(return_actions=True, return_obs=True, return_rewards=True)
    if loop in ("linear", "local"):
        pack = env.pack_policy if loop == "linear" else env.pack_local_policy
        # BeerGame2VecEnv's own default clamp is the one the case is written for
        clip = None if variant == 2 else rc.clip_of(variant, loop)
        assert env._policy_clip() == rc.clip_of(variant, loop) or variant == 1
        res = env.rollout_policy(pack(inp["W"], inp["b"]), None, k1 - k0, shift=rc.SHIFT, clip=clip, **kw)
    else:
        if loop == "mlp-sampled":
            noise = torch.as_tensor(inp["noise"][k0:k1], device=DEV).contiguous()
            kw.update(noise=noise, std=torch.as_tensor(inp["std"]), samples_out=torch.empty_like(noise))
        res = env.rollout_policy(env.pack_local_mlp(*(torch.as_tensor(x) for x in inp["net"])), None, k1 - k0,
                                 clip=rc.clip_of(variant, loop), return_features=True, **kw)
    assert res.reward_sum.dtype == torch.int64
    return SimpleNamespace(actions=_np(res.actions), obs=_np(res.obs), rewards=_np(res.rewards), features=_np(res.features),
                           samples=_np(res.samples), reward_sum=_np(res.reward_sum))


def _same(a, b, what):
    """Exact; float32 on the bits."""
    assert (a is None) == (b is None), what
    if a is None:
        return
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype == np.float32 or b.dtype == np.float32:
        a, b = rc.bits(a), rc.bits(b)
    assert np.array_equal(a, b), what


def _is_the_oracles(got, env, ref, what):
    """The call's streams and the env's state on the sampled envs against the reference."""
    for name in STREAMS:
        x = getattr(got, name)
        if name == "features" and x is None and ref[name] is not None:
            continue  # the local policy returns none: the twin's policy_features() are compared with them
        _same(None if x is None else x[:, IDX], ref[name], (what, name))
    _same(got.reward_sum[IDX], ref["reward_sum"], (what, "reward_sum"))
    assert np.array_equal(got.reward_sum, got.rewards.astype(np.int64).sum(0)), what
    for name in ("inventory", "backlog", "orders_placed", "inventory_costs", "backlog_costs", "episode_return",
                 "final_return", "all_orders_placed") + (("penalty_costs",) if env.penalty_costs is not None else ()):
        _same(getattr(env, name)[IDX].cpu().numpy().astype(np.int64), ref[name], (what, name))
    assert (env.week, env.episode) == (ref["week"], ref["episode"]), what


def _formula(g, variant, loop, k, seen):
    """The closed loop's (actions, samples or None) of week k over the whole batch, from `seen`:
    the observation the twin last returned (linear) or its policy_features() (local, MLP)."""
    inp = rc.inputs(g, variant, loop)
    lo, hi = rc.clip_of(variant, loop)
    if loop == "linear":
        return bg_policy_ref.actions(inp["W"], inp["b"], seen, rc.SHIFT, lo, hi), None
    if loop == "local":
        return bg_local_ref.actions(inp["W"], inp["b"], seen, rc.SHIFT, lo, hi), None
    u = bg_mlp_ref.z_values(*inp["net"], bg_mlp_ref.inputs(seen))
    if loop == "mlp-sampled":
        u = bg_mlp_ref.sample(u, inp["std"], inp["noise"][k])
    return bg_mlp_ref.finish(u, lo, hi), u if loop == "mlp-sampled" else None


def _a_dead_row_is_not_zero(env):
    """The ring holds a non-zero row outside the live mask: summing the whole ring instead of the
    live rows would fail the call that starts here."""
    R = env.ring_slots
    live = {v % R for v in bg_local_ref.live_weeks(env.config.shipment_delays.tolist(), env.max_weeks, env.week)}
    dead = [s for s in range(R) if s not in live]
    assert dead and bool(env._ring[dead].ne(0).any()), (live, dead)


@pytest.mark.parametrize("g, variant, loop", _cases())
def test_rollout(g, variant, loop):
    what = rc.case_id(g, variant, loop)
    ref, K = rc.reference(g, variant, loop), rc.weeks_per_call(g)
    env, twin, split = (_env(g, variant) for _ in range(3))
    # the game: the table's ring, on its side of the LDS limit
    assert env.ring_slots == g.R, what
    assert (env.ring_slots * g.L * 256 * 4 <= 64 * 1024) == (g.ring == "lds"), what
    # reset
    obs0 = _np(env.reset())
    _same(obs0[IDX], ref["reset_obs"], (what, "reset"))
    # one call of K weeks against the oracle
    got = _call(env, g, variant, loop, 0, K)
    assert (got.features is not None) == loop.startswith("mlp") and (got.samples is not None) == (loop == "mlp-sampled")
    _is_the_oracles(got, env, ref, what)
    # the whole batch against a twin stepped on the actions the call took
    _same(_np(twin.reset()), obs0, (what, "twin reset"))
    acts = torch.as_tensor(got.actions, device=DEV)
    last = obs0
    for k in range(K):
        if loop != "open":
            seen = last
            if loop != "linear":
                seen = _np(twin.policy_features())
                _same(seen[IDX], ref["features"][k], (what, "twin features", k))
                if got.features is not None:
                    _same(got.features[k], seen, (what, "features", k))
            a, u = _formula(g, variant, loop, k, seen)
            _same(got.actions[k], a, (what, "formula", k))
            if u is not None:
                _same(got.samples[k], u, (what, "samples formula", k))
        o, r, _, _ = twin.step(acts[k])
        last = _np(o)
        _same(got.obs[k], last, (what, "twin obs", k))
        _same(got.rewards[k], _np(r), (what, "twin rewards", k))
    _assert_same_state(env, twin)
    if loop not in ("open", "linear"):
        _same(_np(env.policy_features())[IDX], ref["final_features"], (what, "final features"))
    # the same K weeks as three calls: from a mid-episode week, and from the week after an auto-reset
    c1, c2 = rc.cuts(g)
    split.reset()
    parts = [_call(split, g, variant, loop, 0, c1)]
    assert (split.week, split.episode) == (c1 % g.T, c1 // g.T)
    if loop not in ("open", "linear") and not rc.stochastic(g, variant) and g.T > 1:
        _a_dead_row_is_not_zero(split)
    parts.append(_call(split, g, variant, loop, c1, c2))
    assert (split.week, split.episode) == (1 % g.T, 1 + (g.T == 1))
    parts.append(_call(split, g, variant, loop, c2, K))
    for name in STREAMS:
        x = getattr(got, name)
        _same(x, None if x is None else np.concatenate([getattr(p, name) for p in parts]), (what, "split", name))
    _same(got.reward_sum, sum(p.reward_sum for p in parts), (what, "split reward_sum"))
    _assert_same_state(split, env)
    for e in (env, twin, split):
        e.check_errors()


@pytest.mark.parametrize("g", rc.OPEN_ONLY, ids=[g.name for g in rc.OPEN_ONLY])
@pytest.mark.parametrize("variant", rc.VARIANTS)
def test_the_closed_loops_refuse_nine_levels_and_more(g, variant):
    """rollout_policy past the level limit: refused with the limit's message, and the env steps on."""
    W, b = np.zeros((g.L, g.L), dtype=np.int32), np.zeros(g.L, dtype=np.int32)

    def call(env):
        with pytest.raises(ValueError, match=rc.LEVEL_LIMIT_MESSAGE):
            env.rollout_policy(W, b, 2)
        env.rollout_policy(W, b, 2)

    _assert_refused_then_steps_on(lambda: _env(g, variant), call)
