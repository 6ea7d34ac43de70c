"""scg_bg_rollout accepts BeerGameEnv2 configs (variant 2) and checks every argument before
any HIP call (no GPU needed): a variant-2 config prepared on the host, with a delay list and
with stochastic delays, fake non-null device pointers that are never dereferenced, and a
failed check leaves the state's week and episode untouched."""
import ctypes

import numpy as np
import pytest

T = 12
DELAYS = {"list": [2, 0, 3, 1, 1, 4, 2, 0, 5, 1, 2, 3], "stochastic": (0, 5)}


def _prepared(delays):
    from gym_supplychain_amd import _native as nat
    from gym_supplychain_amd.envs.beergame_env import _Bg2Config
    stochastic = isinstance(delays, tuple)
    cfg = _Bg2Config(100, 30, T, 4, (0, 16) if stochastic else [4] * T, [12, 12, 12, 12], 1, 2, 100, delays, 4, 4)
    keep = {"delays": (ctypes.c_int32 * (T + 1))(*cfg.shipment_delays.tolist()),
            "demand": (ctypes.c_int32 * T)(*cfg.customer_demand[:T].tolist()),
            "plan": (ctypes.c_int32 * (T + 1))()}
    c = nat.BgConfig()
    c.levels, c.max_weeks = cfg.levels, T
    c.inv_cost, c.backlog_cost = cfg.inv_cost, cfg.backlog_cost
    c.initial_shipment_value, c.initial_orders_value = cfg.initial_shipment_value, cfg.initial_orders_value
    for i, v in enumerate(cfg.initial_inventory.tolist()):
        c.initial_inventory[i] = v
    c.variant, c.max_stock, c.exceeded_capacity_penalty = 2, cfg.max_stock, cfg.penalty
    if stochastic:
        c.demand_mode = nat.SCG_DEMAND_UNIFORM
        c.demand_lo, c.demand_hi = cfg.demand_range
        c.stochastic_delays, c.delay_lo, c.delay_hi = 1, cfg.delay_range[0], cfg.delay_range[1]
    else:
        c.demand_mode = nat.SCG_DEMAND_FIXED
        c.customer_demand = ctypes.cast(keep["demand"], ctypes.c_void_p)
    c.shipment_delays = ctypes.cast(keep["delays"], ctypes.c_void_p)
    c.plan = ctypes.cast(keep["plan"], ctypes.c_void_p)
    assert nat.lib.scg_bg_prepare(ctypes.byref(c)) == 0, nat.last_error()
    assert c.variant == 2 and c.ring_slots == (5 if stochastic else int(np.max(cfg.shipment_delays)) + 1)
    fake = 0x1000
    st = nat.BgState()
    st.n_envs, st.env_offset, st.seed, st.episode, st.week = 300, 0, 1, 3, 0
    for f in ("inventory", "backlog", "orders_placed", "shipments", "inventory_costs", "backlog_costs",
              "penalty_costs", "episode_return", "final_return", "error_flags"):
        setattr(st, f, fake)
    return nat, c, st, keep


@pytest.fixture(params=sorted(DELAYS))
def prepared(request):
    return _prepared(DELAYS[request.param])


def _rollout(nat, c, st, k, actions=0x1000, flags=0):
    rc = nat.lib.scg_bg_rollout(ctypes.byref(c), ctypes.byref(st), k, actions, 0x1000, 0x1000, flags, None)
    msg = nat.last_error()
    assert "not implemented" not in msg, msg
    return rc


def test_version_and_symbols_unchanged():
    from gym_supplychain_amd import _native as nat
    assert nat.ABI_VERSION == 9 and nat.lib.scg_abi_version() == 9
    assert "scg_bg_rollout" in nat.SIGNATURES and not any("rollout2" in s or "bg2" in s for s in nat.SIGNATURES)


def test_rejects_bad_arguments(prepared):
    nat, c, st, _ = prepared
    assert _rollout(nat, c, st, 2, actions=None) == nat.SCG_ERR_INVALID
    assert _rollout(nat, c, st, -1) == nat.SCG_ERR_INVALID
    assert _rollout(nat, c, st, -1, flags=nat.SCG_BG_AUTORESET) == nat.SCG_ERR_INVALID
    assert (st.week, st.episode) == (0, 3)


@pytest.mark.parametrize("flags", [0, 1])
def test_not_reset(prepared, flags):
    nat, c, st, _ = prepared
    st.week = -1
    assert _rollout(nat, c, st, 2, flags=flags) == nat.SCG_ERR_NOT_RESET
    assert (st.week, st.episode) == (-1, 3)


def test_past_the_horizon_without_auto_reset_leaves_the_state(prepared):
    nat, c, st, _ = prepared
    for w0, k in ((0, T + 1), (3, T - 2), (T - 1, 2)):
        st.week = w0
        assert _rollout(nat, c, st, k) == nat.SCG_ERR_PAST_HORIZON, (w0, k)
        assert "terminal week" in nat.last_error()
        assert (st.week, st.episode) == (w0, 3)
