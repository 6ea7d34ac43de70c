"""SupplyChainVecEnv.rollout_policy with a pack_mlp() policy (scg_sc_rollout_mlp).

The closed loop against its definition, as tests/test_gpu_sc_policy_rollout.py does for the
linear policy: the actions are the NumPy float32 formula of the one-hidden-layer ReLU policy
applied to the previous observation, and everything else is what a twin env's open-loop
rollout() of those actions gives — observations, rewards, terminal observation, returns, stocks,
heap sizes, live heap entries in storage order, time step and episode. Every comparison is on
the bits; no tolerance is involved.

Sizes: 130 envs (two full 64-env tiles and a 2-env tail), 9- to 12-step episodes, 25 to 30
steps per call (two auto-resets), the grid capped at one block (a block runs all three tiles)
and launches cut at 5 steps (they end mid-episode). Hidden widths: 16; 5 (fewer units than
waves); 40 (the fused kernel's hidden tile exactly full on sc-2perstage: the stocks lie right
behind it); 41 and 64 (the per-step path on a node-parallel config)."""
import numpy as np
import pytest
import torch

from sc_closed_ref import clamp, policy_z
from test_gpu_sc_policy_rollout import LO, HI, _bits, _sequential_sum, small_launches  # noqa: F401 (autouse fixture)
from test_gpu_sc_rollout import DEV, STOCH, _actions, _pair, _same_state

pytestmark = pytest.mark.gpu


def _params(env, hidden, shared=False, seed=3):
    """Random float32 layers: about half of the hidden units positive, both clamps binding now and then."""
    rng = np.random.default_rng(seed + 100 * hidden)
    shape = () if shared else (env.n_envs,)
    w1 = rng.normal(0.0, 0.35, shape + (hidden, env.n_obs)).astype(np.float32)
    b1 = rng.normal(0.0, 0.5, shape + (hidden,)).astype(np.float32)
    w2 = rng.normal(0.0, 1.4 / np.sqrt(hidden), shape + (env.n_actions, hidden)).astype(np.float32)
    b2 = rng.normal(0.0, 0.5, shape + (env.n_actions,)).astype(np.float32)
    return w1, b1, w2, b2


def _formula(obs, params, lo=LO, hi=HI):
    """The policy as scgpu.h states it, in NumPy float32 (tests/sc_closed_ref.py): obs [N, O] ->
    (hidden [N, H], actions [N, A])."""
    hid, z = policy_z(obs, params)
    return hid, clamp(z, lo, hi)


def _closed_loop_is_open_loop(env, twin, packed, params, k, what=""):
    """rollout_policy on env with every output; the twin rolls the actions it took. Returns the
    result and the formula's hidden units of every step."""
    obs0 = env.observe().clone()
    t0 = env.time_step
    res = env.rollout_policy(packed, None, k, return_actions=True, return_obs=True, return_rewards=True)
    assert res.actions.dtype == torch.float32 and tuple(res.actions.shape) == (k, env.n_envs, env.n_actions)
    assert res.obs.dtype == env.obs_dtype and res.rewards.dtype == torch.float64 and res.reward_sum.dtype == torch.float64
    prev = torch.cat([obs0[None], res.obs[:-1]]).cpu().numpy()
    hidden = []
    for j in range(k):
        hid, act = _formula(prev[j], params)
        hidden.append(hid)
        assert np.array_equal(_bits(res.actions[j]), _bits(act)), (what, "actions of step", j)
    obs, rew, dones = twin.rollout(res.actions)
    assert torch.equal(res.obs, obs) and np.array_equal(_bits(res.rewards), _bits(rew)), what
    assert torch.equal(res.dones, dones) and res.dones.device.type == "cpu", what
    assert dones.tolist() == [(t0 + j + 1) % env.spec.total_time_steps == 0 for j in range(k)]
    _same_state(env, twin, what)
    assert torch.equal(env._term_obs, twin._term_obs), what
    assert np.array_equal(_bits(res.reward_sum), _bits(_sequential_sum(rew))), what
    assert torch.equal(res.last_obs, obs[-1]) and torch.equal(env.observe(), obs[-1]), what
    assert torch.equal(env._pol_act, res.actions[-1]), what
    env.check_errors()
    return res, np.stack(hidden)


CASES = {
    "per_env_f32": dict(obs_dtype=torch.float32, total_time_steps=12),
    "per_env_f64": dict(obs_dtype=torch.float64, total_time_steps=12),
    "shared_f32": dict(obs_dtype=torch.float32, total_time_steps=11),
    "shared_f64": dict(obs_dtype=torch.float64, total_time_steps=11),
    "stochastic": dict(obs_dtype=torch.float32, total_time_steps=12, **STOCH),
    "multiproduct": dict(scenario="sc-2perstage-multiproduct-v0", obs_dtype=torch.float32, total_time_steps=9),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_closed_loop_is_the_formula_and_the_open_loop(case):
    """Two auto-resets inside the call, launches ending mid-episode, three tiles on one block."""
    env, twin = _pair(**CASES[case])
    assert env.kernel == "nodes" and env.mlp_fused(16)
    if case != "multiproduct":
        assert (env.n_actions, env.n_obs) == (14, 27)
    params = _params(env, 16, shared=case.startswith("shared"))
    packed = env.pack_mlp(*params)
    assert packed.hidden == 16 and packed.shared == case.startswith("shared")
    k = 30 if CASES[case]["total_time_steps"] > 9 else 25
    res, hid = _closed_loop_is_open_loop(env, twin, packed, params, k, case)
    assert int(res.dones.sum()) == 2 and env.episode == 2
    acts = res.actions.cpu().numpy()
    print(case, "actions at lo / hi / inside:", (acts == LO).mean(), (acts == HI).mean(), ((acts > LO) & (acts < HI)).mean(),
          "hidden units at 0:", (hid == 0).mean())
    assert (acts == LO).any() and (acts == HI).any() and ((acts > LO) & (acts < HI)).any()  # the clamp's three branches
    assert (hid == 0).any() and (hid > 0).any()                                                # the ReLU's two


@pytest.mark.parametrize("hidden", [5, 40])
def test_fused_hidden_widths(hidden):
    """H = 5: waves 5 to 7 compute no hidden unit. H = 40: the hidden tile fills the inbox values
    and cost rows exactly; a write past it would land in the stocks, which the twin checks
    (and the step after the call)."""
    env, twin = _pair(obs_dtype=torch.float32, total_time_steps=12, **STOCH)
    assert env.mlp_fused(hidden) and env.mlp_fused(40) and not env.mlp_fused(41)
    params = _params(env, hidden)
    packed = env.pack_mlp(*params)
    _closed_loop_is_open_loop(env, twin, packed, params, 30, f"H={hidden}")
    a = _actions(env, 1)[0]
    o1, r1, _, _ = env.step(a)
    o2, r2, _, _ = twin.step(a)
    assert torch.equal(o1, o2) and torch.equal(r1, r2)
    _same_state(env, twin, "the step after the call")


@pytest.mark.parametrize("hidden", [41, 64])
def test_wider_hidden_layers_run_per_step_on_a_nodes_config(hidden):
    env, twin = _pair(obs_dtype=torch.float32, total_time_steps=12, **STOCH)
    assert env.kernel == "nodes" and not env.mlp_fused(hidden)
    params = _params(env, hidden)
    res, _ = _closed_loop_is_open_loop(env, twin, env.pack_mlp(*params), params, 30, f"H={hidden}")
    assert int(res.dones.sum()) == 2
    with pytest.raises(ValueError):
        env.mlp_fused(65)


@pytest.mark.parametrize("kernel", ["lane", "staged", "level", "nodes_build_info"])
def test_unfused_closed_loop_equals_the_fused_one(kernel):
    """Every other config takes the action kernel and a step per step: the same twin test, and
    the fused path's results."""
    kw = dict(obs_dtype=torch.float32, total_time_steps=12, **STOCH)
    if kernel == "nodes_build_info":
        env, twin = _pair(kernel="nodes", build_info=True, **kw)
        assert env.kernel == "nodes" and env.build_info
    else:
        env, twin = _pair(kernel=kernel, **kw)
        assert env.kernel == kernel
    fused = _pair(**kw)[0]
    assert not env.mlp_fused(16) and fused.mlp_fused(16)
    params = _params(env, 16)
    res, _ = _closed_loop_is_open_loop(env, twin, env.pack_mlp(*params), params, 30, kernel)
    ref = fused.rollout_policy(fused.pack_mlp(*params), None, 30, return_actions=True, return_obs=True, return_rewards=True)
    for name in ("actions", "obs", "rewards", "reward_sum", "last_obs"):
        assert np.array_equal(_bits(getattr(res, name)), _bits(getattr(ref, name))), (kernel, name)
    assert torch.equal(env.stock, fused.stock) and torch.equal(env.final_return, fused.final_return)
    if kernel == "nodes_build_info":
        assert torch.equal(env._led, twin._led) and torch.equal(env._fled, twin._fled)


def test_call_boundaries():
    """30 steps in one call equal 7 + 0 + 23 in three; a call of no steps changes nothing."""
    kw = dict(obs_dtype=torch.float32, total_time_steps=12, **STOCH)
    one, parts = _pair(**kw)
    params = _params(one, 16)
    packed = one.pack_mlp(*params)
    out = dict(return_actions=True, return_obs=True, return_rewards=True)
    whole = one.rollout_policy(packed, None, 30, **out)
    a = parts.rollout_policy(packed, None, 7, **out)
    a = [getattr(a, f).clone() for f in ("actions", "obs", "rewards", "reward_sum")]
    before = (parts.stock.clone(), parts._heap_size.clone(), parts.time_step, parts.episode, parts.observe().clone())
    zero = parts.rollout_policy(packed, None, 0, **out)
    assert not zero.reward_sum.any() and zero.dones.numel() == 0 and zero.actions.shape[0] == 0
    assert torch.equal(parts.stock, before[0]) and torch.equal(parts._heap_size, before[1])
    assert (parts.time_step, parts.episode) == before[2:4] and torch.equal(parts.observe(), before[4])
    b = parts.rollout_policy(packed, None, 23, **out)
    for i, f in enumerate(("actions", "obs", "rewards")):
        assert np.array_equal(_bits(torch.cat([a[i], getattr(b, f)])), _bits(getattr(whole, f))), f
    total = a[3].clone()
    for r in b.rewards:
        total = total + r
    assert np.array_equal(_bits(total), _bits(whole.reward_sum))
    assert torch.equal(b.last_obs, whole.last_obs)
    _same_state(one, parts, "30 = 7 + 0 + 23")


def test_checkpoint_mid_episode():
    import gym_supplychain_amd as gsa
    kw = dict(obs_dtype=torch.float32, total_time_steps=10)
    env, twin = _pair(**kw)
    params = _params(env, 16)
    _closed_loop_is_open_loop(env, twin, env.pack_mlp(*params), params, 13, "before the checkpoint")
    assert (env.time_step, env.episode) == (3, 1)
    fresh = gsa.make_vec("sc-2perstage-v0", env.n_envs, seed=99, device=DEV, kernel="nodes", **kw)
    fresh.load_state_dict(env.state_dict())
    packed = fresh.pack_mlp(*params)
    got = fresh.rollout_policy(packed, None, 12, return_actions=True, return_obs=True)
    ref = env.rollout_policy(env.pack_mlp(*params), None, 12, return_actions=True, return_obs=True)
    assert torch.equal(got.actions, ref.actions) and torch.equal(got.obs, ref.obs)
    assert np.array_equal(_bits(got.reward_sum), _bits(ref.reward_sum))
    _same_state(fresh, env, "resumed from the checkpoint")


def test_past_the_horizon_without_auto_reset_changes_nothing():
    env, twin = _pair(auto_reset=False, obs_dtype=torch.float32)
    params = _params(env, 16)
    packed = env.pack_mlp(*params)
    for e in (env, twin):
        e.rollout(_actions(e, 2))
    with pytest.raises(IndexError):
        env.rollout_policy(packed, None, 6)  # 2 + 6 steps of a 7-step episode
    _same_state(env, twin, "after the refused call")
    assert torch.equal(env._heap_tk, twin._heap_tk) and torch.equal(env._heap_val, twin._heap_val)
    _closed_loop_is_open_loop(env, twin, packed, params, 5, "to the terminal step")
    assert env.time_step == 7
    with pytest.raises(IndexError):
        env.rollout_policy(packed, None, 1)


def test_outputs_are_optional():
    full, bare = _pair(obs_dtype=torch.float32, total_time_steps=12, **STOCH)
    params = _params(full, 16)
    packed = full.pack_mlp(*params)
    assert not packed.shared and tuple(packed.params.shape) == (16 * 28 + 14 * 17, 130)
    a = full.rollout_policy(packed, n_steps=30, return_actions=True, return_obs=True, return_rewards=True)
    c = bare.rollout_policy(packed, n_steps=30)
    assert c.actions is None and c.obs is None and c.rewards is None
    assert np.array_equal(_bits(a.reward_sum), _bits(c.reward_sum)) and torch.equal(a.last_obs, c.last_obs)
    assert torch.equal(c.dones, a.dones)
    _same_state(full, bare, "no outputs")
    assert torch.equal(full._term_obs, bare._term_obs)
    with pytest.raises(ValueError):
        full.rollout_policy(packed, packed, 2)  # a packed policy carries its biases
