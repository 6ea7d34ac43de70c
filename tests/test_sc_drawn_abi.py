"""scg_sc_rollout_drawn and scg_sc_noise_fill check every argument before any HIP call (no GPU
needed), as tests/test_sc_sampled_abi.py shows for scg_sc_rollout_sampled: a real sc-2perstage
config prepared on the host, fake non-null device pointers that are never dereferenced, and a
failed check leaves the state's time step and episode untouched. The Python keyword checks of
rollout_policy(noise_seed=) and draw_noise that need no device are covered on a CPU stand-in."""
import ctypes
import os
import types

import pytest
import torch

from conftest import REPO
from test_sc_rollout_abi import T
from test_sc_sampled_abi import FAKE, INF, NAN, _linear, _mlp, prepared  # noqa: F401  (prepared: a fixture)


def _drw(nat, std=FAKE, samples=FAKE, seed=7, row0=0, reserved=0):
    return nat.ScNoiseDraw(std, samples, seed, row0, reserved)


def _call(nat, c, st, k, linear=None, mlp=None, drw="default", flags=0, obs_io=FAKE, act_work=FAKE, reward_sum=FAKE,
          outs=(FAKE, FAKE, FAKE)):
    if isinstance(drw, str):
        drw = _drw(nat)
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    done = ctypes.c_int32(-1)
    return nat.lib.scg_sc_rollout_drawn(ctypes.byref(c), ctypes.byref(st), k, ref(linear), ref(mlp), ref(drw), obs_io,
                                        act_work, *outs, reward_sum, None, flags, ctypes.byref(done), None)


def test_version_symbols_and_struct():
    from gym_supplychain_amd import _native as nat
    assert nat.ABI_VERSION == 9 and nat.lib.scg_abi_version() == 9
    for name in ("scg_sc_rollout_drawn", "scg_sc_noise_fill", "scg_noise_from_words"):
        assert name in nat.SIGNATURES and hasattr(nat.lib, name)
    res, args = nat.SIGNATURES["scg_sc_rollout_drawn"]
    assert res is ctypes.c_int and len(args) == 16
    assert args[3:6] == [ctypes.POINTER(nat.ScPolicy), ctypes.POINTER(nat.ScMlp), ctypes.POINTER(nat.ScNoiseDraw)]
    assert args[6:] == nat.SIGNATURES["scg_sc_rollout_sampled"][1][6:]  # the same argument tail
    D = nat.ScNoiseDraw
    assert ctypes.sizeof(D) == 32
    assert (D.std.offset, D.samples_out.offset, D.seed.offset, D.row0.offset, D.reserved.offset) == (0, 8, 16, 24, 28)
    assert ctypes.sizeof(nat.ScSampling) == 32 and ctypes.sizeof(nat.ScPolicy) == 24 and ctypes.sizeof(nat.ScMlp) == 32
    assert nat.SCG_STREAM_SC_NOISE == 6
    header = open(os.path.join(REPO, "include", "scgpu.h")).read()
    assert "#define SCG_ABI_VERSION 9" in header and "typedef struct scg_sc_noise_draw {" in header
    assert "#define SCG_STREAM_SC_NOISE 6u" in header
    for name in ("scg_sc_rollout_drawn(", "scg_sc_noise_fill(", "scg_noise_from_words("):
        assert name in header


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("policy", ["linear", "mlp"])
def test_rejects_bad_arguments(prepared, policy, flags):  # noqa: F811
    nat, c, st = prepared
    good = dict(linear=_linear(nat)) if policy == "linear" else dict(mlp=_mlp(nat))
    bad = [dict(linear=_linear(nat), mlp=_mlp(nat)),   # both policies
           dict(linear=None, mlp=None),                # neither
           dict(drw=None, **good),
           dict(drw=_drw(nat, std=None), **good),
           dict(drw=_drw(nat, reserved=1), **good), dict(drw=_drw(nat, reserved=1 << 31), **good),
           dict(drw=_drw(nat, row0=2 ** 32 - 1), **good),           # 2 steps from the last row
           dict(k=T, drw=_drw(nat, row0=2 ** 32 - T + 1), **good),
           # what the sampled entry point refuses
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
    for drw in (_drw(nat), _drw(nat, samples=None), _drw(nat, seed=2 ** 64 - 1), _drw(nat, seed=0),
                _drw(nat, row0=2 ** 32 - 1)):  # one step on the last row: row0 + 1 == 2^32
        assert _call(nat, c, st, 1, drw=drw, flags=flags, **good) == nat.SCG_ERR_PAST_HORIZON
    # no steps: std may be null (the call would clear reward_sum, a HIP call; refused earlier here)
    assert _call(nat, c, st, 0, drw=_drw(nat, std=None, row0=2 ** 32 - 1), flags=flags, **good) == nat.SCG_ERR_PAST_HORIZON
    assert (st.time_step, st.episode) == (T, 3)
    st.time_step = 0
    st.stock = None  # the state check runs first
    assert _call(nat, c, st, 2, flags=flags, **good) == nat.SCG_ERR_INVALID and "state buffers" in nat.last_error()


def test_optional_outputs_and_the_paths(prepared):  # noqa: F811
    """As the sampled entry point: no output needed on the fused path, rewards_out on the per-step path."""
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
def test_not_reset_and_past_horizon(prepared, flags):  # noqa: F811
    nat, c, st = prepared
    st.time_step = -1
    assert _call(nat, c, st, 2, linear=_linear(nat), flags=flags) == nat.SCG_ERR_NOT_RESET
    assert (st.time_step, st.episode) == (-1, 3)
    for t0, k in ((0, T + 1), (3, T - 2), (T - 1, 2)):
        st.time_step = t0
        assert _call(nat, c, st, k, mlp=_mlp(nat)) == nat.SCG_ERR_PAST_HORIZON, (t0, k)
        assert (st.time_step, st.episode) == (t0, 3)


def test_noise_fill_and_words_hook_reject_bad_arguments(prepared):  # noqa: F811
    nat, c, st = prepared
    fill = lambda seed, row0, k, out: nat.lib.scg_sc_noise_fill(ctypes.byref(c), ctypes.byref(st), seed, row0, k, out, None)  # noqa: E731
    assert fill(7, 0, -1, FAKE) == nat.SCG_ERR_INVALID
    assert fill(7, 0, 2, None) == nat.SCG_ERR_INVALID
    assert fill(7, 2 ** 32 - 1, 2, FAKE) == nat.SCG_ERR_INVALID
    assert fill(7, 2 ** 32 - 1, 0, None) == 0 and fill(2 ** 64 - 1, 0, 0, None) == 0  # no rows: nothing to do
    assert nat.lib.scg_noise_from_words(None, FAKE, 4, None) == nat.SCG_ERR_INVALID
    assert nat.lib.scg_noise_from_words(FAKE, None, 4, None) == nat.SCG_ERR_INVALID
    assert nat.lib.scg_noise_from_words(FAKE, FAKE, -1, None) == nat.SCG_ERR_INVALID
    assert nat.lib.scg_noise_from_words(None, None, 0, None) == 0
    st.stock = None
    assert fill(7, 0, 2, FAKE) == nat.SCG_ERR_INVALID and "state buffers" in nat.last_error()
    assert (st.time_step, st.episode) == (0, 3)


def _cpu_env(n=5, a=3):
    """The keyword checks need of an env only its sizes and device: a stand-in on the CPU."""
    from gym_supplychain_amd.envs.supplychain_env import SupplyChainVecEnv
    env = types.SimpleNamespace(n_envs=n, n_actions=a, device=torch.device("cpu"))
    env._sampling = types.MethodType(SupplyChainVecEnv._sampling, env)
    env._noise_rows = SupplyChainVecEnv._noise_rows
    env.draw_noise = types.MethodType(SupplyChainVecEnv.draw_noise, env)
    return env


def test_python_keyword_checks():
    import inspect

    from gym_supplychain_amd.envs.supplychain_env import SupplyChainVecEnv
    sig = inspect.signature(SupplyChainVecEnv.rollout_policy).parameters
    assert sig["noise_seed"].default is None and sig["noise_row"].default == 0
    assert list(inspect.signature(SupplyChainVecEnv.draw_noise).parameters) == ["self", "noise_seed", "n_steps", "noise_row", "out"]
    env = _cpu_env()
    K, N, A = 4, 5, 3
    out = torch.empty((K, N, A))
    n, sd, s = env._sampling(K, None, [0.5, 0.0, 0.25], out, drawn=True)
    assert n is None and s is out and sd.tolist() == [0.5, 0.0, 0.25]
    assert env._sampling(K, None, 0.5, None, drawn=True)[1].tolist() == [0.5] * A
    for args in ((None, None, None), (None, None, out), (None, -0.5, None), (None, NAN, None), (None, [0.5, 0.5], None),
                 (None, 0.5, out[:3]), (None, 0.5, out.double())):
        with pytest.raises(ValueError):
            env._sampling(K, *args, drawn=True)
    assert env._noise_rows(0, 0, K) == (0, 0) and env._noise_rows(2 ** 64 - 1, 2 ** 32 - K, K) == (2 ** 64 - 1, 2 ** 32 - K)
    for seed, row in ((-1, 0), (2 ** 64, 0), (1.5, 0), (True, 0), ("7", 0), (7, -1), (7, 2 ** 32 - K + 1), (7, 0.0), (7, None)):
        with pytest.raises(ValueError):
            env._noise_rows(seed, row, K)
    # draw_noise refuses before it reaches the library
    for kw in (dict(noise_seed=-1, n_steps=K), dict(noise_seed=7, n_steps=-1), dict(noise_seed=7, n_steps=1.0),
               dict(noise_seed=7, n_steps=K, noise_row=2 ** 32 - 1), dict(noise_seed=7, n_steps=K, out=out[:3]),
               dict(noise_seed=7, n_steps=K, out=out.double()), dict(noise_seed=7, n_steps=K, out=out.numpy())):
        with pytest.raises(ValueError):
            env.draw_noise(**kw)
