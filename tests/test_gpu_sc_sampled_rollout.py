"""SupplyChainVecEnv.rollout_policy with sampled actions (scg_sc_rollout_sampled).

With `noise` float32 [K, N, A] and `std` float32 [A] the closed loop's action is the clamp of

    u = z + (std[a] * noise[k][n][a])        (the product rounded to float32, then the sum)

where z is what the linear or MLP formula gives before its clamp, k the step's index in the call.
The tests state that in NumPy float32 and check, on the bits: actions[j] and samples[j] against
the formula applied to the previous observation, and everything else against a twin env's
open-loop rollout() of the actions taken, as tests/test_gpu_sc_policy_rollout.py and
tests/test_gpu_sc_mlp_rollout.py do for the deterministic loop.

Sizes: 130 envs (two full 64-env tiles and a 2-env tail), 9- to 12-step episodes, 25 to 30
steps per call (two auto-resets), the grid capped at one block (a block runs all three tiles)
and launches cut at 5 steps, so a launch's noise rows start mid-call and mid-episode."""
import numpy as np
import pytest
import torch

from sc_closed_ref import policy_z
from sc_closed_ref import sample as _sample
from test_gpu_sc_mlp_rollout import _params as _mlp_params
from test_gpu_sc_policy_rollout import LO, HI, _bits, _sequential_sum, small_launches  # noqa: F401 (autouse fixture)
from test_gpu_sc_policy_rollout import _params as _linear_params
from test_gpu_sc_rollout import DEV, STOCH, _actions, _pair, _same_state

pytestmark = pytest.mark.gpu
OUT = dict(return_actions=True, return_obs=True, return_rewards=True)


def _noise(env, k, seed=17):
    """(noise [k, N, A], std [A]): standard normal float32; std in [0.05, 0.6] with one element exactly 0."""
    rng = np.random.default_rng(seed)
    eps = rng.standard_normal((k, env.n_envs, env.n_actions)).astype(np.float32)
    std = rng.uniform(0.05, 0.6, env.n_actions).astype(np.float32)
    std[env.n_actions // 2] = 0.0
    return eps, std


def _z(obs, params):
    """The policy's output before its clamp, in NumPy float32: linear (w, b) or MLP (w1, b1, w2, b2)."""
    return policy_z(obs, params)[1]


def _dev(x):
    return torch.as_tensor(x, device=DEV)


def _sampled_is_open_loop(env, twin, packed, params, eps, std, what=""):
    """rollout_policy with noise on env and every output; the twin rolls the actions it took
    (the checks of the deterministic tests' _closed_loop_is_open_loop, and the samples)."""
    k = eps.shape[0]
    obs0 = env.observe().clone()
    t0 = env.time_step
    noise = _dev(eps)
    samples = torch.full_like(noise, float("nan"))
    res = env.rollout_policy(packed, None, k, noise=noise, std=_dev(std), samples_out=samples, **OUT)
    assert res.samples is samples and torch.equal(noise, _dev(eps))  # the noise is only read
    assert res.actions.dtype == torch.float32 and tuple(res.actions.shape) == (k, env.n_envs, env.n_actions)
    assert res.obs.dtype == env.obs_dtype and res.rewards.dtype == torch.float64 and res.reward_sum.dtype == torch.float64
    prev = torch.cat([obs0[None], res.obs[:-1]]).cpu().numpy()
    got_u = samples.cpu().numpy()
    for j in range(k):
        u, act = _sample(_z(prev[j], params), std, eps[j])
        assert np.array_equal(_bits(got_u[j]), _bits(u)), (what, "samples of step", j)
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
    return res


def _three_branches(res, what):
    """A condition on the inputs: the clamp binds at both ends and leaves actions inside."""
    acts = res.actions.cpu().numpy()
    print(what, "actions at lo / hi / inside:", (acts == LO).mean(), (acts == HI).mean(), ((acts > LO) & (acts < HI)).mean())
    assert (acts == LO).any() and (acts == HI).any() and ((acts > LO) & (acts < HI)).any()


CASES = {
    "per_env_f32": dict(obs_dtype=torch.float32, total_time_steps=12),
    "per_env_f64": dict(obs_dtype=torch.float64, total_time_steps=12),
    "shared_f32": dict(obs_dtype=torch.float32, total_time_steps=11),
    "shared_f64": dict(obs_dtype=torch.float64, total_time_steps=11),
    "stochastic": dict(obs_dtype=torch.float32, total_time_steps=12, **STOCH),
    "multiproduct": dict(scenario="sc-2perstage-multiproduct-v0", obs_dtype=torch.float32, total_time_steps=9),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_sampled_linear_loop_is_its_formula_and_the_open_loop(case):
    """Two auto-resets inside the call, launches ending mid-episode, three tiles on one block."""
    env, twin = _pair(**CASES[case])
    assert env.kernel == "nodes" and not env.build_info
    params = _linear_params(env, shared=case.startswith("shared"))
    k = 30 if CASES[case]["total_time_steps"] > 9 else 25
    eps, std = _noise(env, k)
    packed = env.pack_policy(*(torch.as_tensor(p) for p in params))
    res = _sampled_is_open_loop(env, twin, packed, params, eps, std, case)
    assert int(res.dones.sum()) == 2 and env.episode == 2
    _three_branches(res, case)


@pytest.mark.parametrize("case", ["shared_16", "per_env_16", "per_env_40"])
def test_sampled_mlp_loop_is_its_formula_and_the_open_loop(case):
    """H = 16, and H = 40: the hidden tile exactly full on sc-2perstage, the stocks right behind it."""
    hidden = int(case.rsplit("_", 1)[1])
    env, twin = _pair(obs_dtype=torch.float32, total_time_steps=12, **STOCH)
    assert env.mlp_fused(hidden) and env.mlp_fused(40) and not env.mlp_fused(41)
    params = _mlp_params(env, hidden, shared=case.startswith("shared"))
    eps, std = _noise(env, 30)
    res = _sampled_is_open_loop(env, twin, env.pack_mlp(*params), params, eps, std, case)
    assert int(res.dones.sum()) == 2
    _three_branches(res, case)
    a = _actions(env, 1)[0]
    o1, r1, _, _ = env.step(a)
    o2, r2, _, _ = twin.step(a)
    assert torch.equal(o1, o2) and torch.equal(r1, r2)
    _same_state(env, twin, "the step after the call")


@pytest.mark.parametrize("case", ["lane_linear", "staged_mlp", "level_linear", "nodes_build_info_linear", "nodes_build_info_mlp",
                                  "nodes_mlp_41"])
def test_sampled_per_step_path(case):
    """Configs the fused path refuses run the sampled action kernel and a step per step: the
    same twin test, and the fused path's results."""
    kw = dict(obs_dtype=torch.float32, total_time_steps=12, **STOCH)
    kernel, policy = case.rsplit("_", 1) if not case.endswith("41") else ("nodes", "41")
    if kernel == "nodes_build_info":
        env, twin = _pair(kernel="nodes", build_info=True, **kw)
        assert env.kernel == "nodes" and env.build_info
    else:
        env, twin = _pair(kernel=kernel, **kw)
        assert env.kernel == kernel
    if policy == "linear":
        params = _linear_params(env)
        pack = lambda e: e.pack_policy(*(torch.as_tensor(p) for p in params))  # noqa: E731
    else:
        hidden = 41 if policy == "41" else 16
        params = _mlp_params(env, hidden)
        pack = lambda e: e.pack_mlp(*params)  # noqa: E731
        assert not env.mlp_fused(hidden)
    eps, std = _noise(env, 30)
    res = _sampled_is_open_loop(env, twin, pack(env), params, eps, std, case)
    assert int(res.dones.sum()) == 2
    _three_branches(res, case)
    if policy != "41":  # the fused path on the same inputs
        fused = _pair(**kw)[0]
        s2 = torch.empty_like(res.samples)
        ref = fused.rollout_policy(pack(fused), None, 30, noise=_dev(eps), std=_dev(std), samples_out=s2, **OUT)
        for name in ("actions", "obs", "rewards", "reward_sum", "last_obs", "samples"):
            assert np.array_equal(_bits(getattr(res, name)), _bits(getattr(ref, name))), (case, name)
        assert torch.equal(env.stock, fused.stock) and torch.equal(env.final_return, fused.final_return)
    if kernel == "nodes_build_info":
        assert torch.equal(env._led, twin._led) and torch.equal(env._fled, twin._fled)


@pytest.mark.parametrize("policy", ["linear", "mlp"])
def test_noise_rows_count_on_across_launches_and_calls(policy):
    """One call of 13 steps (launches of 5, 5 and 3) equals calls of 6 and 7 steps fed noise[:6]
    and noise[6:]: a row's index is the step's index in the call."""
    kw = dict(obs_dtype=torch.float32, total_time_steps=10)
    one, parts = _pair(**kw)
    if policy == "linear":
        params = _linear_params(one)
        packed = one.pack_policy(*(torch.as_tensor(p) for p in params))
    else:
        params = _mlp_params(one, 16)
        packed = one.pack_mlp(*params)
    eps, std = _noise(one, 13)
    noise, sd = _dev(eps), _dev(std)
    s_whole, s_a, s_b = torch.empty_like(noise), torch.empty_like(noise[:6]), torch.empty_like(noise[6:])
    whole = one.rollout_policy(packed, None, 13, noise=noise, std=sd, samples_out=s_whole, **OUT)
    a = parts.rollout_policy(packed, None, 6, noise=noise[:6], std=sd, samples_out=s_a, **OUT)
    a_sum = a.reward_sum.clone()
    b = parts.rollout_policy(packed, None, 7, noise=noise[6:], std=sd, samples_out=s_b, **OUT)
    for f in ("actions", "obs", "rewards"):
        assert np.array_equal(_bits(torch.cat([getattr(a, f), getattr(b, f)])), _bits(getattr(whole, f))), f
    assert np.array_equal(_bits(torch.cat([s_a, s_b])), _bits(s_whole))
    total = a_sum
    for r in b.rewards:
        total = total + r
    assert np.array_equal(_bits(total), _bits(whole.reward_sum))
    _same_state(one, parts, "13 = 6 + 7")
    assert (one.time_step, one.episode) == (3, 1)
    # and the whole call is the formula: step 7's row is noise[7], whatever launch or episode it falls in
    u, act = _sample(_z(whole.obs[6].cpu().numpy(), params), std, eps[7])
    assert np.array_equal(_bits(s_whole[7]), _bits(u)) and np.array_equal(_bits(whole.actions[7]), _bits(act))


@pytest.mark.parametrize("case", ["linear", "mlp", "lane"])
def test_samples_may_overwrite_the_noise(case):
    """samples_out=noise (a clone) gives the samples and the state of a separate buffer."""
    kw = dict(obs_dtype=torch.float32, total_time_steps=12, **STOCH)
    apart, inplace = _pair(kernel="lane" if case == "lane" else "nodes", **kw)
    if case == "mlp":
        packed = apart.pack_mlp(*_mlp_params(apart, 16))
    else:
        packed = apart.pack_policy(*(torch.as_tensor(p) for p in _linear_params(apart)))
    eps, std = _noise(apart, 30)
    noise, sd = _dev(eps), _dev(std)
    samples = torch.empty_like(noise)
    a = apart.rollout_policy(packed, None, 30, noise=noise, std=sd, samples_out=samples, **OUT)
    buf = noise.clone()
    b = inplace.rollout_policy(packed, None, 30, noise=buf, std=sd, samples_out=buf, **OUT)
    assert b.samples is buf and np.array_equal(_bits(buf), _bits(samples))
    assert not torch.equal(buf, noise)
    for f in ("actions", "obs", "rewards", "reward_sum"):
        assert np.array_equal(_bits(getattr(a, f)), _bits(getattr(b, f))), f
    _same_state(apart, inplace, "in place")


@pytest.mark.parametrize("case", ["linear", "mlp", "lane_mlp"])
def test_std_zero_is_the_deterministic_loop(case):
    """z + 0 * eps compares equal to z (a -0 z becomes +0): the actions compare equal, the state is the same bits."""
    kw = dict(obs_dtype=torch.float32, total_time_steps=12, **STOCH)
    env, twin = _pair(kernel="lane" if case.startswith("lane") else "nodes", **kw)
    if case.endswith("mlp"):
        packed = env.pack_mlp(*_mlp_params(env, 16))
    else:
        packed = env.pack_policy(*(torch.as_tensor(p) for p in _linear_params(env)))
    eps, _ = _noise(env, 30)
    zero = torch.zeros(env.n_actions, dtype=torch.float32, device=DEV)
    res = env.rollout_policy(packed, None, 30, noise=_dev(eps), std=zero, **OUT)
    assert res.samples is None
    ref = twin.rollout_policy(packed, None, 30, **OUT)
    assert bool((res.actions == ref.actions).all())
    assert torch.equal(res.obs, ref.obs) and np.array_equal(_bits(res.rewards), _bits(ref.rewards))
    assert np.array_equal(_bits(res.reward_sum), _bits(ref.reward_sum))
    _same_state(env, twin, "std = 0")
    scalar = _pair(kernel="lane" if case.startswith("lane") else "nodes", **kw)[0]
    got = scalar.rollout_policy(packed, None, 30, noise=_dev(eps), std=0.0, **OUT)  # a float std: every action's
    assert np.array_equal(_bits(got.actions), _bits(res.actions))


def test_argument_errors_leave_the_env_unchanged():
    env, twin = _pair(obs_dtype=torch.float32, total_time_steps=12, **STOCH)
    N, A = env.n_envs, env.n_actions
    packed = env.pack_mlp(*_mlp_params(env, 16))
    eps, std = _noise(env, 4)
    noise, sd = _dev(eps), _dev(std)
    ok = torch.empty_like(noise)
    nan_std, neg_std = std.copy(), std.copy()
    nan_std[1], neg_std[2] = np.nan, -0.125
    bad = [dict(noise=noise),                                            # noise without std
           dict(std=sd),                                                 # std without noise
           dict(samples_out=ok),                                         # samples_out without noise
           dict(noise=noise[:3], std=sd),                                # wrong shapes
           dict(noise=noise[:, :-1], std=sd),
           dict(noise=noise[:, :, :-1].contiguous(), std=sd),
           dict(noise=noise.flatten(), std=sd),
           dict(noise=noise.double(), std=sd),                           # wrong dtype
           dict(noise=noise.cpu(), std=sd),                              # wrong device
           dict(noise=_dev(np.zeros((4, N, 2 * A), np.float32))[:, :, ::2], std=sd),  # not contiguous
           dict(noise=noise, std=_dev(neg_std)),
           dict(noise=noise, std=_dev(nan_std)),
           dict(noise=noise, std=-1.0),
           dict(noise=noise, std=float("inf")),
           dict(noise=noise, std=sd[:-1]),                               # wrong length
           dict(noise=noise, std=sd, samples_out=ok[:3]),
           dict(noise=noise, std=sd, samples_out=ok.double()),
           dict(noise=noise, std=sd, samples_out=ok.cpu()),
           dict(noise=noise, std=sd, samples_out=torch.empty((4, N, 2 * A), dtype=torch.float32, device=DEV)[:, :, ::2])]
    for kw in bad:
        with pytest.raises(ValueError):
            env.rollout_policy(packed, None, 4, **kw)
    _same_state(env, twin, "after the refused calls")
    a = _actions(env, 1)[0]
    o1, r1, _, _ = env.step(a)
    o2, r2, _, _ = twin.step(a)
    assert torch.equal(o1, o2) and torch.equal(r1, r2)
    _same_state(env, twin, "one step after the refused calls")
    # and the arguments as documented pass
    res = env.rollout_policy(packed, None, 4, noise=noise, std=std.tolist(), samples_out=ok)
    assert res.samples is ok and res.actions is None
