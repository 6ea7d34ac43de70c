"""scg_sc_rollout checks every argument before any HIP call (no GPU needed): a real
sc-2perstage config prepared on the host, fake non-null device pointers that are never
dereferenced, and a failed check leaves the state's time step and episode untouched."""
import ctypes
import os

import pytest

from conftest import REPO

T = 7


def _prepared():
    from gym_supplychain_amd import _native as nat
    from gym_supplychain_amd.envs import SupplyChainSpec
    from gym_supplychain_amd.envs.scenarios import two_per_stage_nodes
    nodes_info, kwargs = two_per_stage_nodes(total_time_steps=T)
    spec = SupplyChainSpec(nodes_info, **kwargs)
    nodes = spec.node_table()
    c = nat.ScConfig()
    c.n_nodes, c.n_products, c.n_retailers = len(spec.nodes), spec.P, spec.n_retailers
    c.total_time_steps, c.avg_leadtime, c.max_leadtime = spec.total_time_steps, spec.avg_leadtime, spec.max_leadtime
    c.demand_lo, c.demand_hi = spec.demand_models[0].lo, spec.demand_models[0].hi
    for k, v in spec.penalties.items():
        setattr(c, k, v)
    c.kernel = nat.SC_KERNEL_NODES
    assert nat.lib.scg_sc_prepare(ctypes.byref(c), nodes) == 0, nat.last_error()
    fake = 0x1000
    c.nodes = fake  # the device node table: never read before the checks fail
    st = nat.ScState()
    st.n_envs, st.env_offset, st.seed, st.episode, st.time_step = 130, 0, 1, 3, 0
    for f in ("stock", "heap_tk", "heap_val", "heap_size", "error_flags", "episode_return", "final_return"):
        setattr(st, f, fake)
    return nat, c, st, nodes


@pytest.fixture()
def prepared():
    return _prepared()


def _rollout(nat, c, st, k, actions=0x1000, obs=0x1000, rewards=0x1000, flags=0):
    done = ctypes.c_int32(-1)
    rc = nat.lib.scg_sc_rollout(ctypes.byref(c), ctypes.byref(st), k, actions, obs, rewards, None, flags,
                                ctypes.byref(done), None)
    return rc, done.value


def test_symbol_constants_and_version():
    from gym_supplychain_amd import _native as nat
    assert nat.ABI_VERSION == 9 and nat.lib.scg_abi_version() == 9
    assert nat.SC_ROLLOUT_MAX == 1024 and nat.SCG_SC_LAST_OBS == 8
    assert "scg_sc_rollout" in nat.SIGNATURES
    header = open(os.path.join(REPO, "include", "scgpu.h")).read()
    assert "#define SCG_SC_ROLLOUT_MAX 1024" in header and "#define SCG_SC_LAST_OBS 8u" in header


def test_rejects_bad_arguments(prepared):
    nat, c, st, _ = prepared
    assert _rollout(nat, c, st, 0)[0] == nat.SCG_ERR_INVALID
    assert _rollout(nat, c, st, -3)[0] == nat.SCG_ERR_INVALID
    assert _rollout(nat, c, st, 2, actions=None)[0] == nat.SCG_ERR_INVALID
    assert _rollout(nat, c, st, 2, rewards=None)[0] == nat.SCG_ERR_INVALID
    assert _rollout(nat, c, st, 2, obs=None)[0] == nat.SCG_ERR_INVALID
    assert _rollout(nat, c, st, 2, obs=None, flags=nat.SCG_SC_LAST_OBS)[0] == nat.SCG_ERR_INVALID
    assert (st.time_step, st.episode) == (0, 3)
    st.stock = None  # sc_check runs first
    rc, _ = _rollout(nat, c, st, 2)
    assert rc == nat.SCG_ERR_INVALID and "state buffers" in nat.last_error()


@pytest.mark.parametrize("flags", [0, 1])
def test_not_reset_and_past_horizon(prepared, flags):
    nat, c, st, _ = prepared
    st.time_step = -1
    assert _rollout(nat, c, st, 2, flags=flags)[0] == nat.SCG_ERR_NOT_RESET
    st.time_step = T  # as after a terminal step without auto-reset
    assert _rollout(nat, c, st, 1, flags=flags)[0] == nat.SCG_ERR_PAST_HORIZON
    assert (st.time_step, st.episode) == (T, 3)


@pytest.mark.parametrize("kernel", ["nodes", "lane"])
def test_rollout_past_the_horizon_without_auto_reset_leaves_the_state(prepared, kernel):
    nat, c, st, nodes = prepared
    if kernel == "lane":  # the loop path checks the same, before its first step
        c.kernel = nat.SC_KERNEL_LANE
        assert nat.lib.scg_sc_prepare(ctypes.byref(c), nodes) == 0
    for t0, k in ((0, T + 1), (3, T - 2), (T - 1, 2)):
        st.time_step = t0
        rc, _ = _rollout(nat, c, st, k)
        assert rc == nat.SCG_ERR_PAST_HORIZON and "terminal step" in nat.last_error(), (t0, k)
        assert (st.time_step, st.episode) == (t0, 3)
