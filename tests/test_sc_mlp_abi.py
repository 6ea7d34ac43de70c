"""scg_sc_rollout_mlp and scg_sc_mlp_fused check every argument before any HIP call (no GPU
needed): a real sc-2perstage config prepared on the host (tests/test_sc_rollout_abi.py), fake
non-null device pointers that are never dereferenced, and a failed check leaves the state's
time step and episode untouched. pack_mlp's word order and its shape and value errors are
checked on CPU tensors."""
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


def _mlp(nat, hidden=16, activation=1, shared=0, reserved=0, lo=-1.0, hi=1.0, params=FAKE):
    return nat.ScMlp(hidden, activation, shared, reserved, lo, hi, params)


def _call(nat, c, st, k, mlp="default", flags=0, obs_io=FAKE, act_work=FAKE, reward_sum=FAKE, outs=(FAKE, FAKE, FAKE)):
    if isinstance(mlp, str):
        mlp = _mlp(nat)
    ref = ctypes.byref(mlp) if mlp is not None else None
    done = ctypes.c_int32(-1)
    return nat.lib.scg_sc_rollout_mlp(ctypes.byref(c), ctypes.byref(st), k, ref, obs_io, act_work, *outs, reward_sum, None,
                                      flags, ctypes.byref(done), None)


def test_version_symbols_and_struct():
    from gym_supplychain_amd import _native as nat
    assert nat.ABI_VERSION == 9 and nat.lib.scg_abi_version() == 9
    assert "scg_sc_rollout_mlp" in nat.SIGNATURES and "scg_sc_mlp_fused" in nat.SIGNATURES
    assert nat.SC_ACT_RELU == 1 and nat.SC_MLP_MAX_HIDDEN == 64
    M = nat.ScMlp
    assert ctypes.sizeof(M) == 32 and M.params.offset == 24
    assert (M.hidden.offset, M.activation.offset, M.shared.offset, M.reserved.offset, M.act_lo.offset,
            M.act_hi.offset) == (0, 4, 8, 12, 16, 20)
    assert ctypes.sizeof(nat.ScPolicy) == 24  # the linear policy's struct is untouched
    header = open(os.path.join(REPO, "include", "scgpu.h")).read()
    assert "#define SCG_SC_MLP_MAX_HIDDEN 64" in header and "#define SCG_SC_ACT_RELU 1" in header
    assert "#define SCG_ABI_VERSION 9" in header


@pytest.mark.parametrize("flags", [0, 1])
def test_rejects_bad_arguments(prepared, flags):
    nat, c, st = prepared
    bad = [dict(mlp=None), dict(mlp=_mlp(nat, params=None)), dict(mlp=_mlp(nat, hidden=0)), dict(mlp=_mlp(nat, hidden=-1)),
           dict(mlp=_mlp(nat, hidden=65)), dict(mlp=_mlp(nat, activation=0)), dict(mlp=_mlp(nat, activation=2)),
           dict(mlp=_mlp(nat, reserved=1)), dict(mlp=_mlp(nat, lo=1.0, hi=-1.0)), dict(mlp=_mlp(nat, lo=NAN)),
           dict(mlp=_mlp(nat, hi=NAN)), dict(mlp=_mlp(nat, lo=-INF)), dict(mlp=_mlp(nat, hi=INF)),
           dict(obs_io=None), dict(act_work=None), dict(reward_sum=None), dict(k=-1), dict(flags=flags | 8)]
    for kw in bad:
        kw.setdefault("flags", flags)
        assert _call(nat, c, st, kw.pop("k", 2), **kw) == nat.SCG_ERR_INVALID, kw
        assert (st.time_step, st.episode) == (0, 3)
    # a shared mlp, the widest one and equal bounds pass the check: the call gets as far as the horizon's
    st.time_step = T
    for ok in (_mlp(nat, shared=1, lo=0.5, hi=0.5), _mlp(nat, hidden=64), _mlp(nat, hidden=1)):
        assert _call(nat, c, st, 1, mlp=ok, flags=flags) == nat.SCG_ERR_PAST_HORIZON
    st.time_step = 0
    st.stock = None  # the state check runs first
    assert _call(nat, c, st, 2, flags=flags) == nat.SCG_ERR_INVALID and "state buffers" in nat.last_error()


def test_optional_outputs(prepared):
    """No output is needed on the fused path; the per-step path (another kernel, or hidden units
    that do not fit) needs rewards_out."""
    nat, c, st = prepared
    st.time_step = T  # past every argument check, refused at the horizon's
    want = nat.SCG_ERR_PAST_HORIZON if c.kernel == nat.SC_KERNEL_NODES else nat.SCG_ERR_INVALID
    assert _call(nat, c, st, 1, outs=(None, None, None)) == want
    assert _call(nat, c, st, 1, outs=(None, None, FAKE)) == nat.SCG_ERR_PAST_HORIZON
    wide = _mlp(nat, hidden=2 * (c.inbox_size + c.n_nodes) + 1)
    assert _call(nat, c, st, 1, mlp=wide, outs=(None, None, None)) == nat.SCG_ERR_INVALID
    assert "rewards_out" in nat.last_error()
    assert _call(nat, c, st, 1, mlp=wide, outs=(None, None, FAKE)) == nat.SCG_ERR_PAST_HORIZON
    assert (st.time_step, st.episode) == (T, 3)


@pytest.mark.parametrize("flags", [0, 1])
def test_not_reset_and_past_horizon(prepared, flags):
    nat, c, st = prepared
    st.time_step = -1
    assert _call(nat, c, st, 2, flags=flags) == nat.SCG_ERR_NOT_RESET
    assert (st.time_step, st.episode) == (-1, 3)
    st.time_step = T  # as after a terminal step without auto-reset
    assert _call(nat, c, st, 1, flags=flags) == nat.SCG_ERR_PAST_HORIZON
    assert (st.time_step, st.episode) == (T, 3)


def test_past_the_horizon_without_auto_reset_leaves_the_state(prepared):
    nat, c, st = prepared
    for t0, k in ((0, T + 1), (3, T - 2), (T - 1, 2)):
        st.time_step = t0
        assert _call(nat, c, st, k) == nat.SCG_ERR_PAST_HORIZON, (t0, k)
        assert "terminal step" in nat.last_error()
        assert (st.time_step, st.episode) == (t0, 3)


def test_mlp_fused_query():
    nat, c, st, nodes = _prepared()
    fused = lambda h: nat.lib.scg_sc_mlp_fused(ctypes.byref(c), ctypes.byref(st), h)  # noqa: E731
    most = 2 * (c.inbox_size + c.n_nodes)
    assert c.inbox_size >= 0 and most == 40  # sc-2perstage: 10 KB of inbox values and cost rows per block
    assert [fused(h) for h in (1, 16, most, most + 1, 64)] == [1, 1, 1, 0, 0]
    for h in (0, -1, 65):
        assert fused(h) == -nat.SCG_ERR_INVALID
    ledgers = ("ledger", "ledger_kind", "final_ledger", "final_ledger_kind", "ledger_part")
    for f in ledgers:  # build_info ledgers: the per-step path
        setattr(st, f, FAKE)
    assert fused(16) == 0, nat.last_error()
    for f in ledgers:
        setattr(st, f, None)
    st.stock = None
    assert fused(16) == -nat.SCG_ERR_INVALID
    st.stock = FAKE
    c.kernel = nat.SC_KERNEL_LANE
    assert nat.lib.scg_sc_prepare(ctypes.byref(c), nodes) == 0
    c.nodes = FAKE
    assert fused(16) == 0 and fused(1) == 0


def test_the_linear_entry_point_still_refuses_other_kinds(prepared):
    nat, c, st = prepared
    done = ctypes.c_int32(-1)
    for kind in (2, 0):
        pol = nat.ScPolicy(kind, 0, -1.0, 1.0, FAKE)
        rc = nat.lib.scg_sc_rollout_policy(ctypes.byref(c), ctypes.byref(st), 2, ctypes.byref(pol), FAKE, FAKE, FAKE, FAKE,
                                           FAKE, FAKE, None, 0, ctypes.byref(done), None)
        assert rc == nat.SCG_ERR_INVALID and (st.time_step, st.episode) == (0, 3)


def _cpu_env(n=5, a=3, o=4):
    """pack_mlp needs of an env only its sizes and device: a stand-in on the CPU."""
    from gym_supplychain_amd.envs.supplychain_env import SupplyChainVecEnv
    env = types.SimpleNamespace(n_envs=n, n_actions=a, n_obs=o, device=torch.device("cpu"))
    env._exact_f32 = types.MethodType(SupplyChainVecEnv._exact_f32, env)
    env.pack_mlp = types.MethodType(SupplyChainVecEnv.pack_mlp, env)
    return env


def test_pack_mlp_word_order_and_errors():
    env = _cpu_env()
    N, A, O, H = 5, 3, 4, 2
    rng = np.random.default_rng(0)
    w1, b1 = rng.normal(size=(N, H, O)).astype(np.float32), rng.normal(size=(N, H)).astype(np.float32)
    w2, b2 = rng.normal(size=(N, A, H)).astype(np.float32), rng.normal(size=(N, A)).astype(np.float32)
    p = env.pack_mlp(w1, b1, w2, b2)
    Q = H * (O + 1) + A * (H + 1)
    assert (p.hidden, p.shared, p.n_envs, p.n_actions, p.n_obs) == (H, False, N, A, O)
    assert tuple(p.params.shape) == (Q, N) and p.params.dtype == torch.float32 and p.params.is_contiguous()
    got = p.params.numpy()
    for i in range(H):
        for j in range(O):
            assert np.array_equal(got[i * (O + 1) + j], w1[:, i, j])
        assert np.array_equal(got[i * (O + 1) + O], b1[:, i])
    for a in range(A):
        for i in range(H):
            assert np.array_equal(got[H * (O + 1) + a * (H + 1) + i], w2[:, a, i])
        assert np.array_equal(got[H * (O + 1) + a * (H + 1) + H], b2[:, a])
    one = env.pack_mlp(w1[0], b1[0], w2[0], b2[0])
    assert one.shared and tuple(one.params.shape) == (Q,) and np.array_equal(one.params.numpy(), got[:, 0])
    spread = env.pack_mlp(w1, b1[1], w2, b2[2])  # [H] and [A] biases are broadcast over the envs
    assert np.array_equal(spread.params.numpy()[O], np.full(N, b1[1, 0])) and spread.params.shape == (Q, N)
    assert env.pack_mlp(w1.astype(np.float64), torch.as_tensor(b1), w2, b2.tolist()).params.equal(p.params)
    assert env.pack_mlp(np.zeros((64, O), np.float32), np.zeros(64), np.zeros((A, 64)), np.zeros(A)).hidden == 64
    bad = [(w1[0], b1, w2, b2),                   # shared w1 with per-env rest
           (w1, b1, w2[0], b2),                   # per-env w1 with a shared w2
           (w1[0], b1[0], w2[0], b2),             # a per-env bias on a shared policy
           (w1, b1, w2[:, :, :1], b2),            # another H in the second layer
           (w1, b1[:, :1], w2, b2),               # another H in the bias
           (w1[:, :, :-1], b1, w2, b2),           # not n_obs inputs
           (w1, b1, w2[:, :-1], b2),              # not n_actions outputs
           (w1[:-1], b1[:-1], w2[:-1], b2[:-1]),  # not n_envs policies
           (np.zeros((0, O)), np.zeros(0), np.zeros((A, 0)), np.zeros(A)),     # H = 0
           (np.zeros((65, O)), np.zeros(65), np.zeros((A, 65)), np.zeros(A)),  # H = 65
           (w1.astype(np.float64) + 1e-12, b1, w2, b2),  # not float32 values
           (w1, b1, w2, b2.astype(np.float64) + 1e-12),
           (w1[0, 0], b1[0], w2[0], b2[0])]
    for args in bad:
        with pytest.raises(ValueError):
            env.pack_mlp(*args)
