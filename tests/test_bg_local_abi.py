"""scg_bg_rollout_local and scg_bg_local_features check every argument before any HIP call (no
GPU needed): BeerGameEnv (variant 1) and BeerGameEnv2 (variant 2, with a delay list and with
stochastic delays) configs prepared on the host, fake non-null device pointers that are never
dereferenced, and a failed check leaves the state's week and episode untouched."""
import ctypes

import pytest

from test_abi import HEADER
from test_bg2_rollout_abi import DELAYS, T, _prepared
from test_bg_policy_abi import FAKE, _prepared_v1


@pytest.fixture(params=["v1", "v2-list", "v2-stochastic"])
def prepared(request):
    if request.param == "v1":
        return _prepared_v1()
    return _prepared(DELAYS[request.param[3:]])


def _policy(nat, kind=2, shift=4, lo=-7, hi=9, params=FAKE):
    return nat.BgLocalPolicy(kind, shift, lo, hi, params)


def _call(nat, c, st, k, pol="default", flags=0, outs=(FAKE, FAKE, FAKE, FAKE)):
    if isinstance(pol, str):
        pol = _policy(nat)
    ref = ctypes.byref(pol) if pol is not None else None
    return nat.lib.scg_bg_rollout_local(ctypes.byref(c), ctypes.byref(st), k, ref, *outs, flags, None)


def _features(nat, c, st, out=FAKE):
    return nat.lib.scg_bg_local_features(ctypes.byref(c), ctypes.byref(st), out, None)


def test_version_symbols_and_struct():
    from gym_supplychain_amd import _native as nat
    assert nat.ABI_VERSION == 9 and nat.lib.scg_abi_version() == 9
    assert "scg_bg_rollout_local" in nat.SIGNATURES and "scg_bg_local_features" in nat.SIGNATURES
    assert (nat.BG_POLICY_LOCAL, nat.BG_LOCAL_MAX_DELAY, nat.BG_LOCAL_FEATURES) == (2, 64, 4)
    # scg_bg_local_policy: four int32, then the pointer
    assert ctypes.sizeof(nat.BgLocalPolicy) == 24
    assert [getattr(nat.BgLocalPolicy, f).offset for f in ("kind", "shift", "act_lo", "act_hi", "params")] == \
        [0, 4, 8, 12, 16]
    header = open(HEADER).read()
    assert "#define SCG_BG_POLICY_LOCAL 2" in header and "#define SCG_BG_LOCAL_MAX_DELAY 64" in header


@pytest.mark.parametrize("flags", [0, 1])
def test_rejects_bad_arguments(prepared, flags):
    nat, c, st, _ = prepared
    bad = [dict(pol=None), dict(pol=_policy(nat, params=None)), dict(pol=_policy(nat, kind=0)),
           dict(pol=_policy(nat, kind=1)), dict(pol=_policy(nat, kind=3)), dict(pol=_policy(nat, shift=-1)),
           dict(pol=_policy(nat, shift=31)), dict(pol=_policy(nat, lo=5, hi=4)), dict(k=-1)]
    for kw in bad:
        assert _call(nat, c, st, kw.pop("k", 2), flags=flags, **kw) == nat.SCG_ERR_INVALID, kw
        assert (st.week, st.episode) == (0, 3)
    # the same with no output requested
    assert _call(nat, c, st, 2, pol=_policy(nat, shift=31), flags=flags, outs=(None,) * 4) == nat.SCG_ERR_INVALID
    assert (st.week, st.episode) == (0, 3)
    assert _features(nat, c, st, out=None) == nat.SCG_ERR_INVALID


@pytest.mark.parametrize("flags", [0, 1])
def test_not_reset(prepared, flags):
    nat, c, st, _ = prepared
    st.week = -1
    assert _call(nat, c, st, 2, flags=flags) == nat.SCG_ERR_NOT_RESET
    assert _features(nat, c, st) == nat.SCG_ERR_NOT_RESET
    assert (st.week, st.episode) == (-1, 3)


def test_past_the_horizon_without_auto_reset_leaves_the_state(prepared):
    nat, c, st, _ = prepared
    for w0, k in ((0, T + 1), (3, T - 2), (T - 1, 2)):
        st.week = w0
        assert _call(nat, c, st, k) == nat.SCG_ERR_PAST_HORIZON, (w0, k)
        assert "terminal week" in nat.last_error()
        assert (st.week, st.episode) == (w0, 3)


def test_levels_nine_refused_eight_accepted_by_the_checks():
    """Levels 9: SCG_ERR_INVALID for the level count. Levels 8 passes that check: the same call
    gets as far as the horizon check, the last one before the first launch."""
    nat, c9, st9, _keep9 = _prepared_v1(levels=9)
    assert _call(nat, c9, st9, 2) == nat.SCG_ERR_INVALID
    assert "levels=9" in nat.last_error()
    assert _features(nat, c9, st9) == nat.SCG_ERR_INVALID and "levels=9" in nat.last_error()
    assert (st9.week, st9.episode) == (0, 3)
    nat, c8, st8, _keep8 = _prepared_v1(levels=8)
    assert _call(nat, c8, st8, T + 1) == nat.SCG_ERR_PAST_HORIZON
    assert (st8.week, st8.episode) == (0, 3)


@pytest.mark.parametrize("week", [0, 5, T])
def test_a_delay_of_65_is_refused_64_is_not(week):
    """Any entry of shipment_delays[0..T] counts, d_0 included; 64 passes that check and the same
    call gets as far as the horizon check."""
    nat, c, st, keep = _prepared_v1()
    old = keep["delays"][week]
    for d, want in ((65, nat.SCG_ERR_INVALID), (64, nat.SCG_ERR_PAST_HORIZON)):
        keep["delays"][week] = d
        assert nat.lib.scg_bg_prepare(ctypes.byref(c)) == 0
        assert _call(nat, c, st, T + 1) == want, (week, d)
        if d == 65:
            assert "SCG_BG_LOCAL_MAX_DELAY" in nat.last_error() and f"shipment_delays[{week}]=65" in nat.last_error()
            assert _call(nat, c, st, 2, flags=1) == nat.SCG_ERR_INVALID
            assert _features(nat, c, st) == nat.SCG_ERR_INVALID and "SCG_BG_LOCAL_MAX_DELAY" in nat.last_error()
        assert (st.week, st.episode) == (0, 3)
    keep["delays"][week] = old


def test_delay_hi_66_is_refused_65_is_not():
    nat, c, st, _keep = _prepared(DELAYS["stochastic"])
    for hi, want in ((66, nat.SCG_ERR_INVALID), (65, nat.SCG_ERR_PAST_HORIZON)):
        c.delay_hi = hi
        assert nat.lib.scg_bg_prepare(ctypes.byref(c)) == 0 and c.ring_slots == hi
        assert _call(nat, c, st, T + 1) == want, hi
        if hi == 66:
            assert "delay_hi" in nat.last_error() and "SCG_BG_LOCAL_MAX_DELAY" in nat.last_error()
            assert _features(nat, c, st) == nat.SCG_ERR_INVALID and "delay_hi" in nat.last_error()
        assert (st.week, st.episode) == (0, 3)


def test_full_table_is_refused():
    nat, c, st, _keep = _prepared_v1()
    c.full_table = 1
    assert nat.lib.scg_bg_prepare(ctypes.byref(c)) == 0
    for flags in (0, 1):
        assert _call(nat, c, st, 2, flags=flags) == nat.SCG_ERR_INVALID
        assert "full_table" in nat.last_error()
    assert _features(nat, c, st) == nat.SCG_ERR_INVALID and "full_table" in nat.last_error()
    assert (st.week, st.episode) == (0, 3)


def test_the_linear_entry_point_still_refuses_kind_2():
    from test_bg_policy_abi import _call as linear_call, _policy as linear_policy
    nat, c, st, _keep = _prepared_v1()
    assert linear_call(nat, c, st, 2, pol=linear_policy(nat, kind=2)) == nat.SCG_ERR_INVALID
