"""BeerGameVecEnv.rollout_policy / BeerGame2VecEnv.rollout_policy (scg_bg_rollout_policy:
bg_rollout_kernel with the policy as its source, both variants, ring in LDS or in HBM):
closed-loop weeks in one call against a twin env stepped week by week with the NumPy restatement
of the policy
(tests/bg_policy_ref.py) applied to its own last observation, and against the oracle. Every
comparison is exact. N = 300 is one full 256-lane block and a 44-lane tail.

Per-env weights lie in [-64, 64], biases in [-2000, 2000], shift = 4; the clamp is narrow, and
every twin asserts on its expected action stream that both bounds are hit and that a negative
pre-shift value occurs, so no case passes vacuously."""
import functools

import numpy as np
import pytest
import torch

import bg_policy_ref
from oracle.beergame import BeerGame2Oracle, BeerGameOracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 300
SHIFT = 4
CLIP1 = (-3, 5)          # BeerGameEnv: increments over the incoming order
T = 12
LIST_DELAYS = [2, 0, 3, 1, 1, 4, 2, 0, 5, 1, 2, 3]  # delay 0, colliding arrival weeks, arrivals past week 12
INVENTORY = [12, 8, 4, 9, 1, 15, 7, 3]
STATE = ("inventory", "backlog", "orders_placed", "inventory_costs", "backlog_costs", "penalty_costs",
         "episode_return", "final_return", "all_orders_placed", "_ring")


def _params(L, n=N, seed=11):
    rs = np.random.RandomState(seed + L)
    return (rs.randint(-64, 65, size=(n, L, L)).astype(np.int32), rs.randint(-2000, 2001, size=(n, L)).astype(np.int32))


def _env1(n=N, L=4, delays=LIST_DELAYS, weeks=T, **kw):
    from gym_supplychain_amd import BeerGameVecEnv
    info = dict(levels=L, initial_inventory=INVENTORY[:L], customer_demand=[0] * weeks, shipment_delays=delays)
    kw.setdefault("track_history", True)
    return BeerGameVecEnv(n, info, demand="poisson", poisson_lambda=6.0, seed=5, device=DEV, **kw)


def _env2(n=N, **kw):
    from gym_supplychain_amd import BeerGame2VecEnv
    kw.setdefault("track_history", True)
    kw.setdefault("weeks", T)
    kw.setdefault("customer_demand", (0, 16))
    kw.setdefault("seed", 5)
    return BeerGame2VecEnv(n, device=DEV, **kw)


def _clip(env, clip):
    return env._policy_clip() if clip is None else clip


def _closed_loop(env, W, b, K, clip=None, shift=SHIFT):
    """Reset `env` and step it K weeks, each action the restatement of its own last observation.
    Returns the expected streams after checking that they exercise the clamp and the floor."""
    lo, hi = _clip(env, clip)
    o = env.reset().cpu().numpy().copy()
    acts, obs, rew, neg = [], [], [], False
    for _ in range(K):
        z = bg_policy_ref.pre_shift(W, b, o)
        neg = neg or bool((z < 0).any())
        a = np.clip(z >> shift, lo, hi).astype(np.int32)
        assert np.array_equal(a, bg_policy_ref.actions(W, b, o, shift, lo, hi))
        ob, r, _, _ = env.step(torch.as_tensor(a, device=DEV))
        o = ob.cpu().numpy().copy()
        acts.append(a)
        obs.append(o)
        rew.append(r.cpu().numpy().copy())
    acts, obs, rew = np.stack(acts), np.stack(obs), np.stack(rew)
    assert (acts == lo).any() and (acts == hi).any() and neg, "the case must hit both bounds and a negative value"
    assert ((acts > lo) & (acts < hi)).any()
    return dict(actions=acts, obs=obs, rewards=rew, reward_sum=rew.astype(np.int64).sum(0), env=env)


def _assert_same_state(a, b):
    for t in STATE:
        x, y = getattr(a, t), getattr(b, t)
        assert (x is None) == (y is None), t
        if x is not None:
            assert torch.equal(x, y), t
    assert (a.week, a.episode) == (b.week, b.episode)


def _assert_result(res, want, first=0):
    assert np.array_equal(res.actions.cpu().numpy(), want["actions"][first:])
    assert np.array_equal(res.obs.cpu().numpy(), want["obs"][first:])
    assert np.array_equal(res.rewards.cpu().numpy(), want["rewards"][first:])
    assert res.reward_sum.dtype == torch.int64
    assert np.array_equal(res.reward_sum.cpu().numpy(), want["rewards"][first:].astype(np.int64).sum(0))


def _assert_policy_equals_twin(make, L, K, pre_steps=0, clip=None):
    W, b = _params(L)
    want = _closed_loop(make(), W, b, K, clip)
    env = make()
    env.reset()
    for k in range(pre_steps):
        env.step(torch.as_tensor(want["actions"][k], device=DEV))
    res = env.rollout_policy(W, b, K - pre_steps, shift=SHIFT, clip=clip, return_actions=True, return_obs=True,
                             return_rewards=True)
    _assert_result(res, want, pre_steps)
    _assert_same_state(env, want["env"])
    env.check_errors()
    want["env"].check_errors()
    return env, want


@functools.lru_cache(maxsize=None)
def _twin1():
    """Variant 1, L = 4, 41 weeks of 12-week episodes: the expected streams, shared and left unchanged."""
    W, b = _params(4)
    return W, b, _closed_loop(_env1(), W, b, 3 * T + 5, CLIP1)


# ---- 1. twin, variant 1 ------------------------------------------------------------------------
def test_policy_equals_twin_variant1():
    W, b, want = _twin1()
    env = _env1()
    assert env.ring_slots == 6
    env.reset()
    res = env.rollout_policy(W, b, 3 * T + 5, shift=SHIFT, clip=CLIP1, return_actions=True, return_obs=True,
                             return_rewards=True)
    _assert_result(res, want)
    _assert_same_state(env, want["env"])
    assert (env.week, env.episode) == (5, 3)
    env.check_errors()


@pytest.mark.parametrize("L,weeks,K", [(1, T, 3 * T + 5), (3, T, 3 * T + 5), (8, T, 3 * T + 5), (4, 50, 135)],
                         ids=["1", "3", "8", "launch-cut"])
def test_policy_equals_twin_variant1_levels(L, weeks, K):
    """launch-cut: 135 weeks of 50-week episodes in one call, launches of 128 + 7 weeks with two
    auto-resets inside the first and the cut mid-episode."""
    delays = (LIST_DELAYS * 5)[:weeks]
    env, _ = _assert_policy_equals_twin(lambda: _env1(L=L, delays=delays, weeks=weeks), L, K, clip=CLIP1)
    assert (env.week, env.episode) == (K % weeks, K // weeks)


# ---- 2. twin, variant 2: default clip, penalty ledger, launch boundaries, auto-resets ----------
@pytest.mark.parametrize("delays", [(0, 5), LIST_DELAYS], ids=["stochastic", "list"])
def test_policy_equals_twin_variant2(delays):
    """Seven step()s, then 293 weeks in one call of 12-week episodes: launches of at most 128 weeks
    whose boundaries fall mid-episode, with auto-resets inside them."""
    env, want = _assert_policy_equals_twin(lambda: _env2(shipment_delays=delays), 4, 300, pre_steps=7)
    assert env._policy_clip() == (0, 30) and env.penalty_costs is not None
    assert (env.week, env.episode) == (0, 25)
    assert want["actions"].min() == 0 and want["actions"].max() == 30


# ---- 3. ring placement ---------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [16, 17])
def test_ring_placement_variant1(slots):
    """R * 4 * 256 * 4 bytes: 64 KiB exactly (the LDS kernel) and one slot more (the HBM kernel)."""
    delays = [2, 0, slots - 1, 1, 1, 4, 2, 0, 5, 1, 2, 3, slots - 1, 2, 0, 3, 7, 1, 2, 2]
    env, _ = _assert_policy_equals_twin(lambda: _env1(delays=delays, weeks=20), 4, 45, clip=CLIP1)
    assert env.ring_slots == slots


@pytest.mark.parametrize("slots", [16, 17])
def test_ring_placement_variant2(slots):
    env, _ = _assert_policy_equals_twin(lambda: _env2(weeks=20, shipment_delays=(0, slots)), 4, 45)
    assert env.ring_slots == slots


# ---- 4. oracle -----------------------------------------------------------------------------------
def test_policy_matches_oracle_variant1():
    """Eight envs, one oracle each, driven closed loop with the restatement and the Philox demand
    the kernels draw, into the second episode."""
    W, b = _params(4)
    env = _env1()
    reset_obs = env.reset().cpu().numpy().copy()
    res = env.rollout_policy(W, b, 2 * T, shift=SHIFT, clip=CLIP1, return_actions=True, return_obs=True,
                             return_rewards=True)
    acts, obs, rew = (x.cpu().numpy() for x in (res.actions, res.obs, res.rewards))
    demand = [env.poisson_demand(ep).cpu().numpy() for ep in range(2)]
    for n in (0, 1, 63, 64, 255, 256, 298, 299):
        for ep in range(2):
            o = BeerGameOracle(dict(levels=4, initial_inventory=INVENTORY[:4], customer_demand=demand[ep][:, n],
                                    shipment_delays=LIST_DELAYS))
            last = o.reset()
            assert np.array_equal(last, reset_obs[n])
            for w in range(T):
                k = ep * T + w
                a = bg_policy_ref.actions(W[n], b[n], last, SHIFT, *CLIP1)
                assert np.array_equal(acts[k, n], a), (n, ep, w)
                last, r, done, _ = o.step(a.astype(np.int64))
                last = np.array(last)
                if not done:  # the terminal week's obs row is the next episode's reset observation
                    assert np.array_equal(obs[k, n], last), (n, ep, w)
                assert rew[k, n] == r, (n, ep, w)
            assert done and np.array_equal(obs[k, n], reset_obs[n])
    assert (env.week, env.episode) == (0, 2)


def test_policy_matches_oracle_variant2():
    from oracle.gen_golden_bg2 import STREAM_BG2_DELAY, STREAM_BG2_DEMAND, uniform_table
    n8, seed = 8, 9
    W, b = _params(4, n=n8)
    env = _env2(n8, shipment_delays=(0, 5), seed=seed)
    reset_obs = env.reset().cpu().numpy().copy()
    res = env.rollout_policy(W, b, 2 * T, shift=SHIFT, return_actions=True, return_obs=True, return_rewards=True)
    acts, obs, rew = (x.cpu().numpy() for x in (res.actions, res.obs, res.rewards))
    sums = np.zeros(n8, dtype=np.int64)
    for ep in range(2):
        demand = uniform_table(seed, n8, ep, T, 0, 16, STREAM_BG2_DEMAND)
        delays = uniform_table(seed, n8, ep, T, 0, 5, STREAM_BG2_DELAY)
        for n in range(n8):
            o = BeerGame2Oracle(weeks=T, customer_demand=demand[n], shipment_delays=delays[n].tolist())
            last = o.reset()
            assert np.array_equal(last, reset_obs[n])
            for w in range(T):
                k = ep * T + w
                a = bg_policy_ref.actions(W[n], b[n], last, SHIFT, 0, 30)
                assert np.array_equal(acts[k, n], a), (n, ep, w)
                last, r, done, _ = o.step(a.astype(np.int64))
                last = np.array(last)
                if not done:
                    assert np.array_equal(obs[k, n], last), (n, ep, w)
                assert rew[k, n] == r, (n, ep, w)
                sums[n] += int(r)
            assert done
    assert np.array_equal(res.reward_sum.cpu().numpy(), sums)
    assert acts.min() == 0 and acts.max() == 30


# ---- 5. outputs optional ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [1, 2])
def test_outputs_are_optional(variant):
    W, b = _params(4)
    make = _env1 if variant == 1 else functools.partial(_env2, shipment_delays=(0, 5))
    clip = CLIP1 if variant == 1 else None
    full, bare = make(), make()
    full.reset()
    bare.reset()
    K = 128 + T + 3  # two launches: the second adds to the first's sums
    want = full.rollout_policy(W, b, K, shift=SHIFT, clip=clip, return_actions=True, return_obs=True,
                               return_rewards=True)
    got = bare.rollout_policy(W, b, K, shift=SHIFT, clip=clip)
    assert got.actions is None and got.obs is None and got.rewards is None
    assert torch.equal(got.reward_sum, want.rewards.to(torch.int64).sum(0))
    assert torch.equal(got.reward_sum, want.reward_sum)
    _assert_same_state(full, bare)
    # overwritten, not accumulated over calls; no weeks: zeros
    again = bare.rollout_policy(bare.pack_policy(W, b), None, 5, shift=SHIFT, clip=clip, return_rewards=True)
    assert torch.equal(again.reward_sum, again.rewards.to(torch.int64).sum(0))
    none = bare.rollout_policy(W, b, 0, shift=SHIFT, clip=clip, return_obs=True)
    assert not none.reward_sum.any() and none.obs.shape == (0, N, 4)
    assert (bare.week, bare.episode) == ((K + 5) % T, (K + 5) // T)


# ---- 6. replay -------------------------------------------------------------------------------------
def test_open_loop_replay_of_the_actions_taken():
    W, b, want = _twin1()
    closed, env = _env1(), _env1()
    closed.reset()
    env.reset()
    res = closed.rollout_policy(W, b, 3 * T + 5, shift=SHIFT, clip=CLIP1, return_actions=True, return_obs=True,
                                return_rewards=True)
    assert np.array_equal(res.actions.cpu().numpy(), want["actions"])
    obs, rew = env.rollout(res.actions)
    assert torch.equal(obs, res.obs) and torch.equal(rew, res.rewards)
    _assert_same_state(env, closed)


# ---- 7. shards -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [1, 2])
def test_shard_equals_its_slice_of_the_batch(variant):
    W, b = _params(4)
    make = _env1 if variant == 1 else functools.partial(_env2, shipment_delays=(0, 5))
    clip = CLIP1 if variant == 1 else None
    whole, part = make(), make(150, env_offset=150)
    whole.reset()
    part.reset()
    kw = dict(shift=SHIFT, clip=clip, return_actions=True, return_obs=True, return_rewards=True)
    a, p = whole.rollout_policy(W, b, 2 * T + 5, **kw), part.rollout_policy(W[150:], b[150:], 2 * T + 5, **kw)
    for f in ("actions", "obs", "rewards"):
        assert torch.equal(getattr(a, f)[:, 150:], getattr(p, f)), f
    assert torch.equal(a.reward_sum[150:], p.reward_sum)
    for t in STATE:
        x, y = getattr(whole, t), getattr(part, t)
        if x is not None:
            assert torch.equal(x[:, 150:] if t == "_ring" else x[150:], y), t


# ---- 8. checkpoint ---------------------------------------------------------------------------------
def test_resumes_from_a_checkpoint_mid_episode():
    W, b = _params(4)
    kw = dict(shift=SHIFT, return_actions=True, return_obs=True, return_rewards=True)
    a = _env2(shipment_delays=(0, 5))
    a.reset()
    a.rollout_policy(W, b, 17, **kw)
    state = a.state_dict()
    c = _env2(shipment_delays=(0, 5))
    c.load_state_dict(state)
    assert (c.week, c.episode) == (5, 1)
    ra, rc = a.rollout_policy(W, b, 20, **kw), c.rollout_policy(W, b, 20, **kw)
    for f in ("actions", "obs", "rewards", "reward_sum"):
        assert torch.equal(getattr(ra, f), getattr(rc, f)), f
    _assert_same_state(a, c)


# ---- 9. overflow -----------------------------------------------------------------------------------
def test_orders_leaving_int32_set_the_overflow_flag_as_the_twin_does():
    n, L = 8, 4
    W = np.zeros((L, L), dtype=np.int32)
    b = np.full(L, 2 ** 30, dtype=np.int32)  # every week adds 2^30 to each level's order
    stepped, rolled = _env1(n, auto_reset=False), _env1(n, auto_reset=False)
    stepped.reset()
    rolled.reset()
    res = rolled.rollout_policy(W, b, 4, return_actions=True)
    assert (res.actions == 2 ** 30).all()
    for k in range(4):
        stepped.step(res.actions[k])
    with pytest.raises(OverflowError):
        stepped.check_errors()
    with pytest.raises(OverflowError):
        rolled.check_errors()
    fine = _env1(n, auto_reset=False)
    fine.reset()
    fine.rollout_policy(W, b, 4, clip=CLIP1)
    fine.check_errors()


# ---- 10. refusals ----------------------------------------------------------------------------------
def test_refusals_leave_week_and_episode_alone():
    W, b = _params(4)
    env = _env1(auto_reset=False)
    env.reset()
    env.rollout_policy(W, b, 3, shift=SHIFT, clip=CLIP1)
    at = (env.week, env.episode)
    assert at == (3, 0)
    bad = [dict(weights=np.zeros((N, 4, 5), dtype=np.int32)), dict(weights=W[:, :3]), dict(bias=b[:, :3]),
           dict(weights=W.astype(np.float32) + 0.5), dict(weights=W.astype(np.int64) + 2 ** 31),
           dict(shift=31), dict(shift=-1), dict(clip=(5, 4))]
    for kw in bad:
        args = dict(weights=W, bias=b, n_weeks=2, shift=SHIFT, clip=CLIP1)
        args.update(kw)
        with pytest.raises(ValueError):
            env.rollout_policy(**args)
        assert (env.week, env.episode) == at, kw
    env.rollout_policy(W.astype(np.float64), b.astype(np.int64), 1, shift=SHIFT, clip=CLIP1)  # exact casts are taken
    at = (env.week, env.episode)
    with pytest.raises(IndexError):
        env.rollout_policy(W, b, T, shift=SHIFT, clip=CLIP1)
    assert (env.week, env.episode) == at == (4, 0)
    from gym_supplychain_amd import BeerGameVecEnv
    nine = BeerGameVecEnv(8, dict(levels=9, initial_inventory=[12] * 9), device=DEV)
    nine.reset()
    with pytest.raises(ValueError):
        nine.rollout_policy(np.zeros((9, 9), dtype=np.int32), np.zeros(9, dtype=np.int32), 2)
    assert (nine.week, nine.episode) == (0, 0)
