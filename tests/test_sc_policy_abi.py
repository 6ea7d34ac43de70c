"""scg_sc_rollout_policy and scg_sc_observe check every argument before any HIP call (no GPU
needed): a real sc-2perstage config prepared on the host (tests/test_sc_rollout_abi.py), fake
non-null device pointers that are never dereferenced, and a failed check leaves the state's
time step and episode untouched."""
import ctypes
import os

import pytest

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


def _policy(nat, kind=1, shared=0, lo=-1.0, hi=1.0, params=FAKE):
    return nat.ScPolicy(kind, shared, lo, hi, params)


def _call(nat, c, st, k, pol="default", flags=0, obs_io=FAKE, act_work=FAKE, reward_sum=FAKE,
          outs=(FAKE, FAKE, FAKE)):
    if isinstance(pol, str):
        pol = _policy(nat)
    ref = ctypes.byref(pol) if pol is not None else None
    done = ctypes.c_int32(-1)
    return nat.lib.scg_sc_rollout_policy(ctypes.byref(c), ctypes.byref(st), k, ref, obs_io, act_work, *outs, reward_sum,
                                         None, flags, ctypes.byref(done), None)


def test_version_symbols_and_struct():
    from gym_supplychain_amd import _native as nat
    assert nat.ABI_VERSION == 9 and nat.lib.scg_abi_version() == 9
    assert "scg_sc_rollout_policy" in nat.SIGNATURES and "scg_sc_observe" in nat.SIGNATURES
    assert nat.SC_POLICY_LINEAR == 1
    P = nat.ScPolicy
    assert ctypes.sizeof(P) == 24
    assert (P.kind.offset, P.shared.offset, P.act_lo.offset, P.act_hi.offset, P.params.offset) == (0, 4, 8, 12, 16)
    header = open(os.path.join(REPO, "include", "scgpu.h")).read()
    assert "#define SCG_SC_POLICY_LINEAR 1" in header and "#define SCG_ABI_VERSION 9" in header


@pytest.mark.parametrize("flags", [0, 1])
def test_rejects_bad_arguments(prepared, flags):
    nat, c, st = prepared
    bad = [dict(pol=None), dict(pol=_policy(nat, params=None)), dict(pol=_policy(nat, kind=0)),
           dict(pol=_policy(nat, kind=2)), dict(pol=_policy(nat, lo=1.0, hi=-1.0)), dict(pol=_policy(nat, lo=NAN)),
           dict(pol=_policy(nat, hi=NAN)), dict(pol=_policy(nat, lo=-INF)), dict(pol=_policy(nat, hi=INF)),
           dict(obs_io=None), dict(act_work=None), dict(reward_sum=None), dict(k=-1), dict(flags=flags | 8)]
    for kw in bad:
        kw.setdefault("flags", flags)
        assert _call(nat, c, st, kw.pop("k", 2), **kw) == nat.SCG_ERR_INVALID, kw
        assert (st.time_step, st.episode) == (0, 3)
    # a shared policy and equal bounds pass the policy check: the call gets as far as the horizon's
    st.time_step = T
    assert _call(nat, c, st, 1, pol=_policy(nat, shared=1, lo=0.5, hi=0.5), flags=flags) == nat.SCG_ERR_PAST_HORIZON
    st.time_step = 0
    st.stock = None  # the state check runs first
    assert _call(nat, c, st, 2, flags=flags) == nat.SCG_ERR_INVALID and "state buffers" in nat.last_error()


def test_optional_outputs(prepared):
    """No output is needed on the fused path; the per-step path needs rewards_out."""
    nat, c, st = prepared
    st.time_step = T  # past every argument check, refused at the horizon's
    want = nat.SCG_ERR_PAST_HORIZON if c.kernel == nat.SC_KERNEL_NODES else nat.SCG_ERR_INVALID
    assert _call(nat, c, st, 1, outs=(None, None, None)) == want
    assert _call(nat, c, st, 1, outs=(None, None, FAKE)) == nat.SCG_ERR_PAST_HORIZON
    assert (st.time_step, st.episode) == (T, 3)


@pytest.mark.parametrize("flags", [0, 1])
def test_not_reset_and_past_horizon(prepared, flags):
    nat, c, st = prepared
    st.time_step = -1
    assert _call(nat, c, st, 2, flags=flags) == nat.SCG_ERR_NOT_RESET
    assert nat.lib.scg_sc_observe(ctypes.byref(c), ctypes.byref(st), FAKE, None) == nat.SCG_ERR_NOT_RESET
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


def test_observe_rejects_a_null_buffer(prepared):
    nat, c, st = prepared
    assert nat.lib.scg_sc_observe(ctypes.byref(c), ctypes.byref(st), None, None) == nat.SCG_ERR_INVALID
    st.heap_size = None
    assert nat.lib.scg_sc_observe(ctypes.byref(c), ctypes.byref(st), FAKE, None) == nat.SCG_ERR_INVALID
