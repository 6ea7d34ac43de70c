"""scg_sc_rollout_sampled checks every argument before any HIP call (no GPU needed), as
tests/test_sc_mlp_abi.py shows for scg_sc_rollout_mlp: a real sc-2perstage config prepared on
the host, fake non-null device pointers that are never dereferenced, and a failed check leaves
the state's time step and episode untouched. The Python keyword checks of rollout_policy that
need no device are covered on a CPU stand-in."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from conftest import REPO
from test_sc_rollout_abi import T, _prepared

FAKE = 0x1000
NAN, INF = float("nan"), float("inf")


@pytest.fixture(params=["nodes", "lane"])
def prepared(request):
    nat, c, st, nodes = _prepared()
    if request.param == "lane":  # the per-step path checks the same, before its first launch
        c.kernel = nat.SC_KERNEL_LANE
        assert nat.lib.scg_sc_prepare(ctypes.byref(c), nodes) == 0
        c.nodes = FAKE
    return nat, c, st


def _linear(nat, kind=1, shared=0, lo=-1.0, hi=1.0, params=FAKE):
    return nat.ScPolicy(kind, shared, lo, hi, params)


def _mlp(nat, hidden=16, activation=1, shared=0, reserved=0, lo=-1.0, hi=1.0, params=FAKE):
    return nat.ScMlp(hidden, activation, shared, reserved, lo, hi, params)


def _smp(nat, std=FAKE, noise=FAKE, samples=FAKE, reserved=0):
    return nat.ScSampling(std, noise, samples, reserved)


def _call(nat, c, st, k, linear=None, mlp=None, smp="default", flags=0, obs_io=FAKE, act_work=FAKE, reward_sum=FAKE,
          outs=(FAKE, FAKE, FAKE)):
    if isinstance(smp, str):
        smp = _smp(nat)
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    done = ctypes.c_int32(-1)
    return nat.lib.scg_sc_rollout_sampled(ctypes.byref(c), ctypes.byref(st), k, ref(linear), ref(mlp), ref(smp), obs_io,
                                          act_work, *outs, reward_sum, None, flags, ctypes.byref(done), None)


def test_version_symbol_and_struct():
    from gym_supplychain_amd import _native as nat
    assert nat.ABI_VERSION == 9 and nat.lib.scg_abi_version() == 9
    assert "scg_sc_rollout_sampled" in nat.SIGNATURES and hasattr(nat.lib, "scg_sc_rollout_sampled")
    res, args = nat.SIGNATURES["scg_sc_rollout_sampled"]
    assert res is ctypes.c_int and len(args) == 16
    assert args[3:6] == [ctypes.POINTER(nat.ScPolicy), ctypes.POINTER(nat.ScMlp), ctypes.POINTER(nat.ScSampling)]
    S = nat.ScSampling
    assert ctypes.sizeof(S) == 32
    assert (S.std.offset, S.noise.offset, S.samples_out.offset, S.reserved.offset) == (0, 8, 16, 24)
    assert ctypes.sizeof(nat.ScPolicy) == 24 and ctypes.sizeof(nat.ScMlp) == 32  # the policies' structs are untouched
    header = open(os.path.join(REPO, "include", "scgpu.h")).read()
    assert "#define SCG_ABI_VERSION 9" in header and "typedef struct scg_sc_sampling {" in header
    assert "scg_sc_rollout_sampled(" in header


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("policy", ["linear", "mlp"])
def test_rejects_bad_arguments(prepared, policy, flags):
    nat, c, st = prepared
    good = dict(linear=_linear(nat)) if policy == "linear" else dict(mlp=_mlp(nat))
    bad = [dict(linear=_linear(nat), mlp=_mlp(nat)),   # both policies
           dict(linear=None, mlp=None),                # neither
           dict(smp=None, **good),
           dict(smp=_smp(nat, std=None), **good), dict(smp=_smp(nat, noise=None), **good),
           dict(smp=_smp(nat, reserved=1), **good), dict(smp=_smp(nat, reserved=-1), **good),
           dict(smp=_smp(nat, reserved=1 << 40), **good),
           # what the deterministic entry points refuse
           dict(obs_io=None, **good), dict(act_work=None, **good), dict(reward_sum=None, **good), dict(k=-1, **good),
           dict(flags=flags | 8, **good)]
    if policy == "linear":
        bad += [dict(linear=_linear(nat, params=None)), dict(linear=_linear(nat, kind=0)), dict(linear=_linear(nat, kind=2)),
                dict(linear=_linear(nat, lo=1.0, hi=-1.0)), dict(linear=_linear(nat, lo=NAN)), dict(linear=_linear(nat, hi=INF))]
    else:
        bad += [dict(mlp=_mlp(nat, params=None)), dict(mlp=_mlp(nat, hidden=0)), dict(mlp=_mlp(nat, hidden=65)),
                dict(mlp=_mlp(nat, activation=0)), dict(mlp=_mlp(nat, reserved=1)), dict(mlp=_mlp(nat, lo=1.0, hi=-1.0)),
                dict(mlp=_mlp(nat, lo=NAN)), dict(mlp=_mlp(nat, hi=INF)), dict(mlp=_mlp(nat, lo=-INF))]
    for kw in bad:
        kw.setdefault("flags", flags)
        assert _call(nat, c, st, kw.pop("k", 2), **kw) == nat.SCG_ERR_INVALID, kw
        assert (st.time_step, st.episode) == (0, 3)
    # good arguments pass every check: the call gets as far as the horizon's
    st.time_step = T
    for smp in (_smp(nat), _smp(nat, samples=None), _smp(nat, noise=FAKE, samples=FAKE)):
        assert _call(nat, c, st, 1, smp=smp, flags=flags, **good) == nat.SCG_ERR_PAST_HORIZON
    # no steps: std and noise may be null (the call would clear reward_sum, a HIP call; refused earlier here)
    assert _call(nat, c, st, 0, smp=_smp(nat, std=None, noise=None), flags=flags, **good) == nat.SCG_ERR_PAST_HORIZON
    assert (st.time_step, st.episode) == (T, 3)
    st.time_step = 0
    st.stock = None  # the state check runs first
    assert _call(nat, c, st, 2, flags=flags, **good) == nat.SCG_ERR_INVALID and "state buffers" in nat.last_error()


def test_optional_outputs_and_the_paths(prepared):
    """As the deterministic entry points: no output needed on the fused path, rewards_out on the per-step path
    (another kernel, or an MLP too wide for the idle LDS)."""
    nat, c, st = prepared
    st.time_step = T
    want = nat.SCG_ERR_PAST_HORIZON if c.kernel == nat.SC_KERNEL_NODES else nat.SCG_ERR_INVALID
    for good in (dict(linear=_linear(nat)), dict(mlp=_mlp(nat))):
        assert _call(nat, c, st, 1, outs=(None, None, None), **good) == want
        assert _call(nat, c, st, 1, outs=(None, None, FAKE), **good) == nat.SCG_ERR_PAST_HORIZON
    wide = _mlp(nat, hidden=2 * (c.inbox_size + c.n_nodes) + 1)
    assert _call(nat, c, st, 1, mlp=wide, outs=(None, None, None)) == nat.SCG_ERR_INVALID
    assert "rewards_out" in nat.last_error()
    assert _call(nat, c, st, 1, mlp=wide, outs=(None, None, FAKE)) == nat.SCG_ERR_PAST_HORIZON
    assert (st.time_step, st.episode) == (T, 3)


@pytest.mark.parametrize("flags", [0, 1])
def test_not_reset_and_past_horizon(prepared, flags):
    nat, c, st = prepared
    st.time_step = -1
    assert _call(nat, c, st, 2, linear=_linear(nat), flags=flags) == nat.SCG_ERR_NOT_RESET
    assert (st.time_step, st.episode) == (-1, 3)
    for t0, k in ((0, T + 1), (3, T - 2), (T - 1, 2)):
        st.time_step = t0
        assert _call(nat, c, st, k, mlp=_mlp(nat)) == nat.SCG_ERR_PAST_HORIZON, (t0, k)
        assert (st.time_step, st.episode) == (t0, 3)


def _cpu_env(n=5, a=3):
    """_sampling needs of an env only its sizes and device: a stand-in on the CPU."""
    from gym_supplychain_amd.envs.supplychain_env import SupplyChainVecEnv
    env = types.SimpleNamespace(n_envs=n, n_actions=a, device=torch.device("cpu"))
    env._sampling = types.MethodType(SupplyChainVecEnv._sampling, env)
    return env


def test_python_keyword_checks():
    from gym_supplychain_amd.envs.supplychain_env import ScPolicyRollout
    assert "samples" in ScPolicyRollout.__slots__ and ScPolicyRollout(None, None, None).samples is None
    env = _cpu_env()
    K, N, A = 4, 5, 3
    noise = torch.randn((K, N, A))
    out = torch.empty((K, N, A))
    n, sd, s = env._sampling(K, noise, [0.5, 0.0, 0.25], out)
    assert n is noise and s is out and sd.dtype == torch.float32 and sd.tolist() == [0.5, 0.0, 0.25]
    assert env._sampling(K, noise, 0.5, None)[1].tolist() == [0.5] * A and env._sampling(K, noise, 0.5, noise)[2] is noise
    assert env._sampling(K, noise, np.array([1, 2, 3], dtype=np.float64), None)[1].tolist() == [1.0, 2.0, 3.0]
    bad = [(noise, None, None), (None, 0.5, None), (None, None, out),
           (noise[:3], 0.5, None), (noise.double(), 0.5, None), (noise.numpy(), 0.5, None),
           (torch.randn((K, N, 2 * A))[:, :, ::2], 0.5, None), (noise.flatten(), 0.5, None),
           (noise, -0.5, None), (noise, NAN, None), (noise, INF, None), (noise, [0.5, -0.0 - 1e-9, 0.5], None),
           (noise, [0.5, 0.5], None), (noise, [[0.5, 0.5, 0.5]], None), (noise, "wide", None),
           (noise, 0.5, out[:3]), (noise, 0.5, out.double()), (noise, 0.5, torch.empty((K, N, 2 * A))[:, :, ::2])]
    for args in bad:
        with pytest.raises(ValueError):
            env._sampling(K, *args)
