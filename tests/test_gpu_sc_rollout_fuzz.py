"""Fuzz of the fused SupplyChain rollouts on the device: rollout() and the four closed loops of
rollout_policy() (linear or MLP, deterministic or sampled) on the random chains of
tests/sc_rollout_cases.py, whose shapes take the node-parallel block where sc-2perstage-v0 never
does: fewer than 8 waves, waves that own two nodes, the stage's and the noise's tail loops,
observation rows of exactly 32 and of several chunks of 32, the hidden tile at its bound and at
64 units, three products, heaps of 2 to 12 slots, Poisson lead times with mean 1, and blocks
within 3 KiB of the CU's LDS. Two chains the node-parallel kernel refuses run the staged kernel
and the per-step action kernels.

The expected side is the oracle (tests/sc_closed_ref.py: the float32 policy formulas in NumPy and
oracle/supplychain.py with the device's draws) on envs 0, 63, 64 and 129, and across the whole
batch the existing twin checks: a twin env stepped K times, or rolling open loop the actions the
closed loop took. Every comparison is on the bits; no tolerance is involved. A chain the library
refuses fails its tests (the one expected refusal is asserted by its message).

Sizes: 130 envs (two full 64-env tiles and a 2-env tail), 6-step episodes, 15 steps per call
(two auto-resets, ending mid-episode), the grid capped at one block (it takes all three tiles)
and launches cut at 5 steps (they end mid-episode, the state handed over through HBM)."""
import numpy as np
import pytest
import torch

import sc_rollout_cases as rc
from test_gpu_sc_mlp_rollout import _closed_loop_is_open_loop as _mlp_closed_loop_is_open_loop
from test_gpu_sc_policy_rollout import _closed_loop_is_open_loop, small_launches  # noqa: F401 (autouse fixture)
from test_gpu_sc_rollout import DEV, _actions, _roll_equals_steps, _same_state, _step_all
from test_gpu_sc_sampled_rollout import _sampled_is_open_loop

pytestmark = pytest.mark.gpu
DTYPES = {"f64": torch.float64, "f32": torch.float32}
K, SAMPLE = rc.K, rc.SAMPLE


def _case_dtypes(cases):
    return [pytest.param(c, d, id=f"seed{c.seed}-{d}") for c in cases for d in rc.dtypes(c)]


def _closed_cases():
    return [pytest.param(c, cfg, d, id=f"seed{c.seed}-{rc.config_id(cfg)}-{d}") for c in rc.CASES
            for cfg in rc.closed_configs(c) for d in rc.dtypes(c, cfg)]


def _envs(case, dtype, count=2):
    """`count` identical envs of the case's chain, reset; the first one's reset observation is the oracle's."""
    from gym_supplychain_amd import SupplyChainVecEnv
    nodes, env_kw = rc.chain(case)
    envs = [SupplyChainVecEnv(rc.N_ENVS, nodes, seed=99 + case.seed, device=DEV, obs_dtype=DTYPES[dtype],
                              kernel="nodes" if case.kernel == "nodes" else "auto", **env_kw) for _ in range(count)]
    for e in envs:
        assert e.kernel == case.kernel, (case.seed, e.kernel)
        assert (e.n_actions, e.n_obs, e.heap_capacity, e._cfg.inbox_size) == (case.A, case.O, case.heap_cap, case.inbox)
        if case.kernel == "nodes":
            assert e._cfg.group == case.waves
        obs0 = e.reset()
    got = obs0.cpu().numpy()
    for n, r in rc.reference(case).items():
        assert np.array_equal(rc.bits(got[n]), rc.bits(_obs(r.obs0, dtype))), (case.seed, "reset", n)
    return envs


def _obs(x, dtype):
    """The oracle's float64 observation as the env's dtype gives it."""
    return np.asarray(x, dtype=np.float64) if dtype == "f64" else np.asarray(x, dtype=np.float64).astype(np.float32)


def _state_is_the_oracles(env, refs, what):
    """Time step, episode, stocks and live heap entries in storage order of the sampled envs."""
    stock = env.stock.cpu().numpy()
    for n, r in refs.items():
        assert (env.time_step, env.episode) == (r.time_step, r.episode), what
        assert np.array_equal(rc.bits(stock[n]), rc.bits(np.asarray(r.stocks, dtype=np.float64))), (what, "stocks", n)
        assert env.heaps(n) == r.heaps, (what, "heaps", n)


def _outputs_are_the_oracles(refs, dtype, obs, rewards, what, term_obs=None, actions=None, samples=None, reward_sum=None):
    """obs [k, N, O], rewards [k, N] (and actions, samples [k, N, A], reward_sum [N], the env's
    terminal observation [N, O]) of the sampled envs against their references' first k rows."""
    obs, rewards = obs.cpu().numpy(), rewards.cpu().numpy()
    k = obs.shape[0]
    for n, r in refs.items():
        assert np.array_equal(rc.bits(obs[:, n]), rc.bits(_obs(r.obs[:k], dtype))), (what, "obs", n)
        assert np.array_equal(rc.bits(rewards[:, n]), rc.bits(r.rewards[:k])), (what, "rewards", n)
        if term_obs is not None:  # of the last episode end inside the k steps
            last_end = max(j for j in r.term_obs if j < k)
            assert np.array_equal(rc.bits(term_obs[n].cpu().numpy()), rc.bits(_obs(r.term_obs[last_end], dtype))), \
                (what, "terminal observation", n)
        if actions is not None:
            assert np.array_equal(rc.bits(actions[:, n].cpu().numpy()), rc.bits(r.actions[:k])), (what, "actions", n)
        if samples is not None:
            assert np.array_equal(rc.bits(samples[:, n].cpu().numpy()), rc.bits(r.samples[:k])), (what, "samples", n)
        if reward_sum is not None:
            assert k == K, what
            assert np.array_equal(rc.bits(reward_sum[n].cpu().numpy()), rc.bits(np.float64(r.reward_sum))), (what, "reward_sum", n)


def _one_more_step(env, twin, what):
    """A write past the hidden tile lands in the stocks: the step after the call, on env and twin."""
    a = _actions(env, 1)[0]
    o1, r1, _, _ = env.step(a)
    o2, r2, _, _ = twin.step(a)
    assert torch.equal(o1, o2) and torch.equal(r1, r2), what
    _same_state(env, twin, what + ": the step after the call")


def test_the_expected_refusal():
    """Seed 48 with float64 observations: the block would need more than the CU's LDS."""
    from gym_supplychain_amd import SupplyChainVecEnv
    case = rc.BY_SEED[48]
    nodes, env_kw = rc.chain(case)
    with pytest.raises(ValueError, match=rc.LDS_MESSAGE):
        SupplyChainVecEnv(rc.N_ENVS, nodes, seed=99 + case.seed, device=DEV, obs_dtype=torch.float64, kernel="nodes", **env_kw)


@pytest.mark.parametrize("case, dtype", _case_dtypes(rc.CASES))
def test_open_loop_rollout(case, dtype):
    """rollout(actions) of 15 steps against the oracle on the sampled envs and against a twin
    stepped 15 times across the batch; a third env rolls the first 7 steps, so the terminal
    observation of each of the two episode ends crossed is seen."""
    what = f"seed {case.seed} {dtype}"
    rolled, stepped, head = _envs(case, dtype, 3)
    refs = rc.reference(case)
    acts = torch.as_tensor(rc.open_loop_actions(case), device=DEV)
    h_obs, h_rew, h_dones = head.rollout(acts[:7])
    assert h_dones.tolist() == [False] * 5 + [True, False] and (head.time_step, head.episode) == (1, 1)
    _outputs_are_the_oracles(refs, dtype, h_obs, h_rew, what + ", first 7 steps", term_obs=head._term_obs)
    obs, rew, dones = _roll_equals_steps(rolled, stepped, acts, what)
    assert dones.tolist() == [j in (5, 11) for j in range(K)] and (rolled.time_step, rolled.episode) == (3, 2)
    assert torch.equal(obs[:7], h_obs) and torch.equal(rew[:7], h_rew)
    _outputs_are_the_oracles(refs, dtype, obs, rew, what, term_obs=rolled._term_obs)
    _state_is_the_oracles(rolled, refs, what)


@pytest.mark.parametrize("seed", [36, 6])
def test_last_obs_only(seed):
    """The rollout that stores the last observation alone, on the two float64 blocks at the edge of
    LDS: the oracle's last row, every reward, the second terminal observation and the final state."""
    case = rc.BY_SEED[seed]
    rolled, stepped = _envs(case, "f64")
    refs = rc.reference(case)
    acts = torch.as_tensor(rc.open_loop_actions(case), device=DEV)
    last, rew, dones = rolled.rollout(acts, last_obs_only=True)
    o2, r2, d2 = _step_all(stepped, acts)
    assert torch.equal(last, o2[-1]) and torch.equal(rew, r2) and torch.equal(dones, d2)
    _same_state(rolled, stepped, seed)
    assert torch.equal(rolled._term_obs, stepped._term_obs)
    for n, r in refs.items():
        assert np.array_equal(rc.bits(last[n].cpu().numpy()), rc.bits(r.obs[-1]))
        assert np.array_equal(rc.bits(rew[:, n].cpu().numpy()), rc.bits(r.rewards))
        assert np.array_equal(rc.bits(rolled._term_obs[n].cpu().numpy()), rc.bits(np.asarray(r.term_obs[11], dtype=np.float64)))
    _state_is_the_oracles(rolled, refs, f"seed {seed} last_obs_only")
    rolled.check_errors()


@pytest.mark.parametrize("case, cfg, dtype", _closed_cases())
def test_closed_loop(case, cfg, dtype):
    """rollout_policy() of 15 steps: actions (and samples), observations, rewards, reward_sum, the
    terminal observation, stocks and heaps of the sampled envs against the reference, and across
    the batch the formula and a twin's open-loop rollout of the actions taken."""
    policy, hidden, shared, sampled = cfg
    what = f"seed {case.seed} {rc.config_id(cfg)} {dtype}"
    env, twin = _envs(case, dtype)
    params, eps, std = rc.policy_inputs(case, cfg)
    refs = rc.reference(case, cfg)
    if policy == "mlp":
        if case.kernel == "nodes":
            bound = rc.hidden_bound(case)
            assert env.mlp_fused(hidden), what
            if bound <= 64:
                assert env.mlp_fused(bound) and not env.mlp_fused(bound + 1), what
        else:
            assert not env.mlp_fused(hidden), what
        packed = env.pack_mlp(*params)
        assert packed.hidden == hidden and not packed.shared
    elif sampled:
        packed = env.pack_policy(*(torch.as_tensor(p) for p in params))
    if sampled:
        assert int((std == 0).sum()) == 1
        res = _sampled_is_open_loop(env, twin, packed, params, eps, std, what)
    elif policy == "mlp":
        res, _ = _mlp_closed_loop_is_open_loop(env, twin, packed, params, K, what)
    else:
        res = _closed_loop_is_open_loop(env, twin, params[0], params[1], K, what)
    assert res.dones.tolist() == [j in (5, 11) for j in range(K)] and (env.time_step, env.episode) == (3, 2)
    _outputs_are_the_oracles(refs, dtype, res.obs, res.rewards, what, term_obs=env._term_obs, actions=res.actions,
                             samples=res.samples if sampled else None, reward_sum=res.reward_sum)
    _state_is_the_oracles(env, refs, what)
    if policy == "mlp":
        _one_more_step(env, twin, what)
