"""GPU parity: the HIP BeerGame kernels (through the C ABI) against the reference's golden
vectors and, at full BASELINE sizes, against the oracle. Integer state must be bit-exact.
"""
import numpy as np
import pytest
import torch

from golden_io import beergame_cases, load_beergame
from oracle.beergame import run_batch_episode
from oracle.philox import STREAM_ACTION, STREAM_DEMAND, draw_words
from oracle.poisson import poisson_invert, poisson_thresholds

pytestmark = pytest.mark.gpu
CASES = beergame_cases()
DEV = "cuda"


def _vec(g, **kw):
    from gym_supplychain_amd import BeerGameVecEnv
    T, N, L = g["actions"].shape
    if g["is_poisson"]:
        env = BeerGameVecEnv(N, g["info"], demand="poisson", poisson_lambda=float(g["lam"]), seed=int(g["seed"]),
                             horizon=T, device=DEV, **kw)
        for _ in range(int(g["episode"])):  # each reset after the first starts the next episode
            env.reset()
    else:
        env = BeerGameVecEnv(N, dict(g["info"], customer_demand=g["demand"][0].tolist()), demand="fixed",
                             device=DEV, **kw)
    return env


def _i32(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("name", CASES)
def test_step_matches_reference(name):
    g = load_beergame(name)
    T, N, L = g["actions"].shape
    env = _vec(g, auto_reset=False, track_history=True)
    obs = env.reset()
    assert np.array_equal(obs.cpu().numpy(), g["ref_reset_obs"])
    acts = _i32(g["actions"])
    for w in range(T):
        obs, rew, done, info = env.step(acts[w])
        assert np.array_equal(obs.cpu().numpy(), g["ref_obs"][w]), (name, w)
        assert np.array_equal(rew.cpu().numpy(), g["ref_reward"][w]), (name, w)
        assert np.array_equal(env.inventory.cpu().numpy(), g["ref_inventory"][w])
        assert np.array_equal(env.backlog.cpu().numpy(), g["ref_backlog"][w])
        assert np.array_equal(env.orders_placed.cpu().numpy(), g["ref_orders_placed"][w])
        assert bool(done.all()) == bool(g["ref_done"][w].all()) and bool(done.any()) == bool(g["ref_done"][w].any())
    assert np.array_equal(env.inventory_costs.cpu().numpy(), g["ref_inventory_costs"])
    assert np.array_equal(env.backlog_costs.cpu().numpy(), g["ref_backlog_costs"])
    assert np.array_equal(env.all_orders_placed.cpu().numpy(), g["ref_all_orders_placed"])
    assert np.array_equal(env.episode_return.cpu().numpy(), g["ref_reward"].astype(np.int64).sum(0))
    assert np.array_equal(env.final_return.cpu().numpy(), g["ref_reward"].astype(np.int64).sum(0))
    with pytest.raises(IndexError):  # the reference raises on customer_demand[T] (:79)
        env.step(acts[0])


@pytest.mark.parametrize("name", [c for c in CASES if c != "levels3_fixed"])
def test_device_poisson_draws_match_oracle(name):
    g = load_beergame(name)
    env = _vec(g)
    got = env.poisson_demand(int(g["episode"])).cpu().numpy().T
    assert np.array_equal(got, g["demand"])


@pytest.mark.parametrize("name", CASES)
def test_table_demand_and_rollout_match_reference(name):
    from gym_supplychain_amd import BeerGameVecEnv
    g = load_beergame(name)
    T, N, L = g["actions"].shape
    env = BeerGameVecEnv(N, g["info"], demand=_i32(g["demand"].T), device=DEV, auto_reset=False,
                         track_history=True)
    env.reset()
    obs, rew = env.rollout(_i32(g["actions"]))
    assert np.array_equal(obs.cpu().numpy(), g["ref_obs"])
    assert np.array_equal(rew.cpu().numpy(), g["ref_reward"])
    assert np.array_equal(env.inventory.cpu().numpy(), g["ref_inventory"][-1])
    assert np.array_equal(env.backlog.cpu().numpy(), g["ref_backlog"][-1])
    assert np.array_equal(env.orders_placed.cpu().numpy(), g["ref_orders_placed"][-1])
    assert np.array_equal(env.inventory_costs.cpu().numpy(), g["ref_inventory_costs"])
    assert np.array_equal(env.backlog_costs.cpu().numpy(), g["ref_backlog_costs"])
    assert np.array_equal(env.all_orders_placed.cpu().numpy(), g["ref_all_orders_placed"])
    with pytest.raises(IndexError):
        env.rollout(_i32(g["actions"][:1]))


@pytest.mark.parametrize("name", CASES)
def test_single_env_facade(name):
    """The drop-in BeerGameEnv: results, state attributes (incoming_orders and the whole
    absolute-week shipments table included, beergame_env.py:46-52,79-81) every week."""
    import contextlib
    import io
    from gym_supplychain_amd import BeerGameEnv
    g = load_beergame(name)
    T, N, L = g["actions"].shape
    for n in range(2):
        env = BeerGameEnv(dict(g["info"], customer_demand=g["demand"][n].tolist()))
        with pytest.raises(AttributeError):
            env.step(np.zeros(L, dtype=np.int64))
        o = env.reset()
        assert o.dtype == np.int64 and np.array_equal(o, g["ref_reset_obs"][n])
        assert np.array_equal(env.incoming_orders, np.full(L, int(g["initial_orders_value"])))
        for w in range(T):
            obs, r, done, info = env.step(g["actions"][w, n].tolist())
            assert obs.dtype == np.int64 and isinstance(r, np.int64) and isinstance(done, bool) and info == {}
            assert np.array_equal(obs, g["ref_obs"][w, n]) and r == g["ref_reward"][w, n]
            assert done == bool(g["ref_done"][w, n])
            assert np.array_equal(env.incoming_orders, g["ref_incoming_orders"][w, n]), (name, n, w)
            sh = env.shipments
            assert sh.dtype == np.int64 and np.array_equal(sh, g["ref_shipments"][w, n]), (name, n, w)
        assert np.array_equal(env.inventory_costs, g["ref_inventory_costs"][n])
        assert np.array_equal(env.all_orders_placed, g["ref_all_orders_placed"][n])
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            env.render()
        text = buf.getvalue()
        for key in ("Week:", "Inventory:", "Incoming order:", "Orders placed:", "Next shipments:", "Current delay:",
                    "Inventory costs:", "Backlog costs:"):
            assert key in text
        with pytest.raises(IndexError):
            env.step(g["actions"][0, n])


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("slab", [True, False])
def test_vec_full_table_matches_reference(name, slab):
    """BeerGameVecEnv(full_table=True): the reference's absolute-week shipments table of
    every env, every week, through the slab and the general step kernels, across an
    auto-reset (stale rows of the previous episode read 0 until scheduled again)."""
    g = load_beergame(name)
    T, N, L = g["actions"].shape
    ns = g["ref_shipments"].shape[1]
    env = _vec(g, full_table=True, state_slab=slab, auto_reset=True)
    assert env.full_table and env.ring_slots == g["ref_shipments"].shape[2]
    env.reset()
    acts = _i32(g["actions"])
    for w in range(T):
        obs, rew, done, info = env.step(acts[w])
        ref_obs = g["ref_obs"][w] if w < T - 1 else g["ref_reset_obs"]
        assert np.array_equal(obs.cpu().numpy(), ref_obs) and np.array_equal(rew.cpu().numpy(), g["ref_reward"][w])
        if w < T - 1:
            assert np.array_equal(env.shipment_table()[:ns].cpu().numpy(), g["ref_shipments"][w]), (name, w)
    # after the fused auto-reset: only the initial pipeline rows are scheduled
    table = env.shipment_table()[:ns].cpu().numpy()
    assert np.array_equal(table, np.broadcast_to(_initial_table(g), table.shape))


def _initial_table(g):
    T, _, L = g["actions"].shape
    R = g["ref_shipments"].shape[2]
    t = np.zeros((R, L), dtype=np.int64)
    t[1:3] = int(g["initial_shipment_value"])   # shipment_delays[0] = 2 (:39, :52)
    return t


def _oracle_episode(info, N, T, L, seed, lam, episode, actions, env_offset=0):
    thr = poisson_thresholds(lam)
    words = draw_words(seed, np.arange(env_offset, env_offset + N), episode, T, STREAM_DEMAND)
    demand = poisson_invert(words, thr)
    return run_batch_episode(info, demand, actions)


def _uniform_actions_np(seed, N, T, L, tag, lo, hi, env_offset=0):
    words = draw_words(seed, np.arange(env_offset, env_offset + N), tag, T * L, STREAM_ACTION)
    v = lo + ((words.astype(np.uint64) * np.uint64(hi - lo + 1)) >> np.uint64(32)).astype(np.int64)
    return v.reshape(N, T, L).transpose(1, 0, 2)


def _uniform_actions_dev(seed, N, T, L, tag, lo, hi, env_offset=0):
    import ctypes
    from gym_supplychain_amd import _native as nat
    out = torch.empty((T, N, L), dtype=torch.int32, device=DEV)
    nat.check(nat.lib.scg_uniform_ints(seed, env_offset, N, T, L, tag, lo, hi, out.data_ptr(),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def test_full_size_episode_matches_oracle():
    """BASELINE config 2 at full size: 65,536 envs, Poisson(8) demand, default chain."""
    from gym_supplychain_amd import BeerGameVecEnv
    N, T, L, seed, lam = 65536, 35, 4, 0x5EED0000, 8.0
    acts = _uniform_actions_dev(seed, N, T, L, 0, 0, 8)
    acts_np = _uniform_actions_np(seed, N, T, L, 0, 0, 8)
    assert np.array_equal(acts.cpu().numpy(), acts_np)
    env = BeerGameVecEnv(N, {}, demand="poisson", poisson_lambda=lam, seed=seed, device=DEV, auto_reset=False,
                         track_history=True)
    env.reset()
    want = _oracle_episode({}, N, T, L, seed, lam, 0, acts_np)
    obs_all = np.zeros((T, N, L), dtype=np.int64)
    rew_all = np.zeros((T, N), dtype=np.int64)
    for w in range(T):
        obs, rew, done, _ = env.step(acts[w])
        obs_all[w] = obs.cpu().numpy()
        rew_all[w] = rew.cpu().numpy()
    assert np.array_equal(obs_all, want["obs"])
    assert np.array_equal(rew_all, want["reward"])
    assert np.array_equal(env.inventory_costs.cpu().numpy(), want["inventory_costs"])
    assert np.array_equal(env.backlog_costs.cpu().numpy(), want["backlog_costs"])
    assert np.array_equal(env.all_orders_placed.cpu().numpy(), want["all_orders_placed"])
    # size-independent property: the return is the sum of the per-step rewards
    assert np.array_equal(env.final_return.cpu().numpy(), want["reward"].sum(0))


def test_autoreset_across_episodes_matches_oracle():
    from gym_supplychain_amd import BeerGameVecEnv
    N, T, L, seed, lam = 4096, 35, 4, 17, 8.0
    info = dict(shipment_delays=[1, 3, 0, 2] * 9)
    env = BeerGameVecEnv(N, info, demand="poisson", poisson_lambda=lam, seed=seed, device=DEV, auto_reset=True)
    obs0 = env.reset().clone()
    for ep in range(3):
        acts_np = _uniform_actions_np(seed, N, T, L, ep, -2, 9)
        acts = _i32(acts_np)
        want = _oracle_episode(info, N, T, L, seed, lam, ep, acts_np)
        for w in range(T):
            obs, rew, done, info_d = env.step(acts[w])
            assert np.array_equal(rew.cpu().numpy(), want["reward"][w]), (ep, w)
            if w < T - 1:
                assert not bool(done.any()) and info_d == {}
                assert np.array_equal(obs.cpu().numpy(), want["obs"][w])
            else:
                assert bool(done.all())
                assert np.array_equal(info_d["terminal_observation"].cpu().numpy(), want["obs"][w])
                assert np.array_equal(info_d["episode_return"].cpu().numpy(), want["reward"].sum(0))
                assert np.array_equal(obs.cpu().numpy(), obs0.cpu().numpy())  # reset observation
        assert env.week == 0 and env.episode == ep + 1


def _assert_rollout_equals_steps(N, info, seed=5):
    """A twin pair from reset over three 12-week episodes and five weeks: one env steps, the other
    rolls out in one call; every obs and reward and the state afterwards are equal."""
    from gym_supplychain_amd import BeerGameVecEnv
    T, L = len(info["customer_demand"]), info["levels"]
    K = 3 * T + 5
    acts = _uniform_actions_dev(seed, N, K, L, 7, -3, 7)
    a = BeerGameVecEnv(N, info, demand="poisson", poisson_lambda=6.0, seed=seed, device=DEV)
    b = BeerGameVecEnv(N, info, demand="poisson", poisson_lambda=6.0, seed=seed, device=DEV)
    a.reset()
    b.reset()
    obs_r, rew_r = b.rollout(acts)
    for k in range(K):
        obs, rew, _, _ = a.step(acts[k])
        assert torch.equal(obs, obs_r[k]) and torch.equal(rew, rew_r[k]), k
    for t in ("inventory", "backlog", "orders_placed", "inventory_costs", "backlog_costs", "episode_return",
              "final_return"):
        assert torch.equal(getattr(a, t), getattr(b, t)), t
    assert (a.week, a.episode) == (b.week, b.episode)
    return a, b


def test_rollout_equals_steps_across_episode_end():
    T = 12
    _assert_rollout_equals_steps(3000, dict(levels=5, initial_inventory=[12, 8, 4, 9, 1], customer_demand=[0] * T,
                                            shipment_delays=[2, 0, 3, 1, 1, 4, 2, 0, 5, 1, 2, 3]))


@pytest.mark.parametrize("max_delay", [3, 5], ids=["lds", "hbm"])
def test_rollout_equals_steps_at_16_levels(max_delay):
    """L = 16, the most a rollout takes: 4 ring slots x 16 levels x 256 lanes is the LDS ring at
    exactly 64 KiB, 6 slots the HBM ring. 300 envs: a full block and a 44-lane tail; 41 weeks:
    auto-resets inside the launch and a last group of one week."""
    T, L = 12, 16
    delays = [2, 0, 3, 1, 1, max_delay, 2, 0, max_delay, 1, 2, 3]
    stepped, env = _assert_rollout_equals_steps(300, dict(levels=L, initial_inventory=list(range(3, 3 + L)),
                                                          customer_demand=[0] * T, shipment_delays=delays))
    assert torch.equal(stepped._ring, env._ring)
    assert env.ring_slots == max_delay + 1 and (env.week, env.episode) == (5, 3)
    stepped.check_errors()
    env.check_errors()


def test_sharding_is_invariant():
    """Rank shards (env_offset) reproduce one big batch bit for bit (DESIGN.md multi-GPU)."""
    from gym_supplychain_amd import BeerGameVecEnv
    N, T, L, seed = 2000, 35, 4, 3
    acts = _uniform_actions_dev(seed, N, T, L, 0, 0, 8)
    whole = BeerGameVecEnv(N, {}, demand="poisson", seed=seed, device=DEV)
    parts = [BeerGameVecEnv(N // 2, {}, demand="poisson", seed=seed, env_offset=o, device=DEV) for o in (0, N // 2)]
    whole.reset()
    for p in parts:
        p.reset()
    for w in range(T):
        o, r, _, _ = whole.step(acts[w])
        o1, r1, _, _ = parts[0].step(acts[w, : N // 2])
        o2, r2, _, _ = parts[1].step(acts[w, N // 2:])
        assert torch.equal(o, torch.cat([o1, o2])) and torch.equal(r, torch.cat([r1, r2]))


def test_errors():
    from gym_supplychain_amd import BeerGameVecEnv
    from gym_supplychain_amd import _native as nat
    env = BeerGameVecEnv(8, {}, device=DEV)
    with pytest.raises(RuntimeError):
        env.step(torch.zeros((8, 4), dtype=torch.int32, device=DEV))
    env.reset()
    with pytest.raises(ValueError):
        env.step(torch.zeros((8, 5), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        BeerGameVecEnv(8, {}, demand="poisson", poisson_lambda=-1.0, device=DEV)
    with pytest.raises(ValueError):
        BeerGameVecEnv(8, {"shipment_delays": [nat.BG_MAX_DELAY + 1] * 35}, device=DEV)


def test_timed_step_matches_and_stamps_kernel():
    from gym_supplychain_amd import BeerGameVecEnv
    from gym_supplychain_amd import _native as nat
    N, T, L = 4096, 35, 4
    acts = _uniform_actions_dev(1, N, T, L, 0, 0, 8)
    a = BeerGameVecEnv(N, {}, demand="poisson", seed=1, device=DEV)
    b = BeerGameVecEnv(N, {}, demand="poisson", seed=1, device=DEV)
    a.reset()
    b.reset()
    evs = [(nat.hip_event(), nat.hip_event()) for _ in range(T)]
    for w in range(T):
        oa, ra, _, _ = a.step(acts[w])
        ob, rb, _, _ = b.step(acts[w], evs[w])
        assert torch.equal(oa, ob) and torch.equal(ra, rb)
    torch.cuda.synchronize()
    ms = [nat.hip_event_elapsed_ms(s, e) for s, e in evs]
    assert all(0.0 < m < 50.0 for m in ms), ms
    for s, e in evs:
        nat.hip_event_destroy(s)
        nat.hip_event_destroy(e)


# ---- BeerGameEnv2 ----------------------------------------------------------------------
from golden_io import beergame2_cases, load_beergame2  # noqa: E402


@pytest.mark.parametrize("name", beergame2_cases())
def test_beergame2_matches_reference(name):
    from gym_supplychain_amd import BeerGame2VecEnv
    g = load_beergame2(name)
    T, N, L = g["actions"].shape
    kw = dict(g["kwargs"])
    for k in ("customer_demand", "shipment_delays"):
        if isinstance(kw.get(k), list) and len(kw[k]) == 2:
            kw[k] = tuple(kw[k])
    env = BeerGame2VecEnv(N, seed=int(g["seed"]), device=DEV, auto_reset=False, track_history=True, **kw)
    for _ in range(int(g["episode"])):
        env.reset()
    obs = env.reset()
    assert np.array_equal(obs.cpu().numpy(), g["ref_reset_obs"])
    acts = _i32(g["actions"])
    for w in range(T):
        obs, rew, done, _ = env.step(acts[w])
        assert np.array_equal(obs.cpu().numpy(), g["ref_obs"][w]), (name, w)
        assert np.array_equal(rew.cpu().numpy(), g["ref_reward"][w]), (name, w)
        assert np.array_equal(env.inventory.cpu().numpy(), g["ref_inventory"][w])
        assert np.array_equal(env.backlog.cpu().numpy(), g["ref_backlog"][w])
        assert np.array_equal(env.orders_placed.cpu().numpy(), g["ref_orders_placed"][w])
    for k in ("inventory_costs", "backlog_costs", "penalty_costs"):
        assert np.array_equal(getattr(env, k).cpu().numpy().astype(np.float64), g["ref_" + k])
    with pytest.raises(IndexError):
        env.step(acts[0])


def test_beergame2_facade_and_autoreset():
    from gym_supplychain_amd import BeerGame2VecEnv, BeerGameEnv2
    g = load_beergame2("defaults")
    T, N, L = g["actions"].shape
    e = BeerGameEnv2()
    o = e.reset()
    assert o.dtype == np.int64 and np.array_equal(o, g["ref_reset_obs"][0])
    for w in range(T):
        obs, r, done, info = e.step(g["actions"][w, 0])
        assert np.array_equal(obs, g["ref_obs"][w, 0]) and r == g["ref_reward"][w, 0] and type(r) is int
        assert done == (w == T - 1) and info == {}
    assert e.penalty_costs.dtype == np.float64 and np.array_equal(e.penalty_costs, g["ref_penalty_costs"][0])
    # auto-reset with stochastic draws: the second episode draws fresh tables
    v = BeerGame2VecEnv(256, customer_demand=(0, 16), shipment_delays=(0, 5), seed=3, device=DEV)
    v.reset()
    a = torch.full((256, 4), 5, dtype=torch.int32, device=DEV)
    rets = []
    for ep in range(2):
        for w in range(35):
            _, _, done, info = v.step(a)
        assert bool(done.all())
        rets.append(info["episode_return"].clone())
    assert not torch.equal(rets[0], rets[1])


@pytest.mark.parametrize("N,lam", [(1000, 8.0), (257, 60.0), (77, 100.0)])
def test_ragged_batch_threshold_paths_match_oracle(N, lam):
    """Tail lanes of a partial block and every Poisson-threshold path of the step kernel:
    table of <= 64 entries (one per lane), 65..128 (two per lane) and > 128 (scalar walk)."""
    from gym_supplychain_amd import BeerGameVecEnv
    T, L, seed = 35, 4, 0xC0FFEE
    acts_np = _uniform_actions_np(seed, N, T, L, 0, 0, 12)
    acts = _i32(acts_np)
    env = BeerGameVecEnv(N, {}, demand="poisson", poisson_lambda=lam, seed=seed, device=DEV, auto_reset=False,
                         track_history=True)
    env.reset()
    want = _oracle_episode({}, N, T, L, seed, lam, 0, acts_np)
    for w in range(T):
        obs, rew, _, _ = env.step(acts[w])
        assert np.array_equal(obs.cpu().numpy(), want["obs"][w]), w
        assert np.array_equal(rew.cpu().numpy(), want["reward"][w]), w
    assert np.array_equal(env.inventory_costs.cpu().numpy(), want["inventory_costs"])
    assert np.array_equal(env.all_orders_placed.cpu().numpy(), want["all_orders_placed"])


# ---- state slab and int32 overflow --------------------------------------
def test_slab_and_general_kernels_agree():
    """The slab step kernel and the general kernel on separate buffers, same inputs, over
    auto-reset episodes with every optional output on; the slab kernel is the one a default
    VecEnv launches."""
    from gym_supplychain_amd import BeerGameVecEnv
    N, T, L, seed = 4096, 35, 4, 99
    info = dict(shipment_delays=[1, 3, 0, 2, 2] * 7)
    acts = _uniform_actions_dev(seed, N, 2 * T + 3, L, 1, -2, 9)
    kw = dict(demand="poisson", seed=seed, device=DEV, track_history=True)
    a = BeerGameVecEnv(N, info, **kw)
    b = BeerGameVecEnv(N, info, state_slab=False, **kw)
    _step_pair(a, b, acts)


def _step_pair(a, b, acts):
    """Steps the slab env a and the separate-buffers env b through acts, comparing every output
    and every state tensor after each step. Returns a's (obs, reward, all done) per step as host
    values; a terminal step's obs is its terminal observation."""
    assert a._slab is not None and b._slab is None
    a.reset()
    b.reset()
    seen = []
    for k in range(acts.shape[0]):
        oa, ra, da, ia = a.step(acts[k])
        ob, rb, db, ib = b.step(acts[k])
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
        if ia:
            assert torch.equal(ia["terminal_observation"], ib["terminal_observation"])
            assert torch.equal(ia["episode_return"], ib["episode_return"])
        for t in ("inventory", "backlog", "orders_placed", "inventory_costs", "backlog_costs", "episode_return",
                  "all_orders_placed"):
            assert torch.equal(getattr(a, t), getattr(b, t)), (k, t)
        assert torch.equal(a._ring, b._ring), k
        seen.append(((ia["terminal_observation"] if ia else oa).cpu().numpy(), ra.cpu().numpy(), bool(da.all())))
    a.check_errors()
    b.check_errors()
    return seen


@pytest.mark.parametrize("demand", ["fixed", "poisson", "table"])
@pytest.mark.parametrize("N,L", [(260, 4), (12, 3), (6, 2), (8, 1)])
def test_slab_and_general_kernels_agree_at_small_shapes(N, L, demand):
    """The same pair at the shapes where a row path changes: a full block plus a 4-lane tail
    (260, 4), scalar rows (12, 3), int2 rows (6, 2), a single level (8, 1); every N * L is a
    multiple of 4, so the first env does run the slab kernel. Six weeks whose delays ship
    direct (0), twice into one arrival week (weeks 1 and 2 into week 4: store, then accumulate)
    and past the horizon (weeks 5 and 6: drop), with ledgers, returns and history on, over
    2 T + 3 steps (two auto-resets). The first episode is also held against the NumPy oracle."""
    from gym_supplychain_amd import BeerGameVecEnv
    T, seed, lam = 6, 31, 8.0
    info = dict(levels=L, initial_inventory=[12, 9, 7, 5][:L], shipment_delays=[3, 2, 0, 1, 4, 1])
    acts_np = _uniform_actions_np(seed, N, 2 * T + 3, L, 1, -2, 9)
    kw = dict(seed=seed, device=DEV, track_history=True)
    if demand == "fixed":
        info["customer_demand"] = [4, 0, 9, 2, 7, 5]
        dem_np = np.tile(np.asarray(info["customer_demand"], dtype=np.int64), (N, 1))
        kw["demand"] = "fixed"
    elif demand == "poisson":
        words = draw_words(seed, np.arange(N), 0, T, STREAM_DEMAND)
        dem_np = poisson_invert(words, poisson_thresholds(lam))
        kw.update(demand="poisson", poisson_lambda=lam, horizon=T)
    else:
        dem_np = (np.arange(N)[:, None] * 7 + np.arange(T)[None, :] * 3) % 11
        kw["demand"] = _i32(dem_np.T)
    a = BeerGameVecEnv(N, info, **kw)
    b = BeerGameVecEnv(N, info, state_slab=False, **kw)
    seen = _step_pair(a, b, _i32(acts_np))
    want = run_batch_episode(info, dem_np, acts_np[:T])
    for w in range(T):
        obs, rew, done = seen[w]
        assert np.array_equal(obs, want["obs"][w]) and np.array_equal(rew, want["reward"][w]), w
        assert done == (w == T - 1)
    assert a.week == 3 and a.episode == 2


@pytest.mark.parametrize("N,L", [(77, 3), (1001, 5)])
def test_general_kernel_for_unaligned_batches_matches_oracle(N, L):
    """N * L not a multiple of 4: separate buffers, general kernel, still the oracle's results."""
    from gym_supplychain_amd import BeerGameVecEnv
    T, seed, lam = 35, 12, 8.0
    info = dict(levels=L, initial_inventory=[12] * L)
    acts_np = _uniform_actions_np(seed, N, T, L, 0, 0, 10)
    env = BeerGameVecEnv(N, info, demand="poisson", poisson_lambda=lam, seed=seed, device=DEV, auto_reset=False)
    assert env._slab is None
    env.reset()
    want = _oracle_episode(info, N, T, L, seed, lam, 0, acts_np)
    acts = _i32(acts_np)
    for w in range(T):
        obs, rew, _, _ = env.step(acts[w])
        assert np.array_equal(obs.cpu().numpy(), want["obs"][w]) and np.array_equal(rew.cpu().numpy(), want["reward"][w])


@pytest.mark.parametrize("slab", [True, False])
def test_int32_overflow_is_flagged(slab):
    """The reference is int64 (beergame_env.py:33,35,121,130-132): orders that double every
    level past 2^31, or a cost product beyond int32, set the sticky flag."""
    from gym_supplychain_amd import BeerGameEnv, BeerGameVecEnv
    N, L = 256, 4
    env = BeerGameVecEnv(N, {}, device=DEV, state_slab=slab, auto_reset=False)
    env.reset()
    big = torch.full((N, L), 2 ** 30, dtype=torch.int32, device=DEV)
    env.step(big)
    env.check_errors()                          # orders 2^30 + 4 still fit
    env.step(big)                               # incoming 2^30 + 4 plus action 2^30 -> > 2^31
    with pytest.raises(OverflowError):
        env.check_errors()
    # the cost product alone: inventory 12 * inv_cost 2^28 > 2^31
    env = BeerGameVecEnv(N, {"inv_cost": 2 ** 28}, device=DEV, state_slab=slab, auto_reset=False)
    env.reset()
    env.step(torch.zeros((N, L), dtype=torch.int32, device=DEV))
    with pytest.raises(OverflowError):
        env.check_errors()
    # a normal episode leaves it clear
    env = BeerGameVecEnv(N, {}, demand="poisson", device=DEV, state_slab=slab)
    env.reset()
    for w in range(70):
        env.step(_uniform_actions_dev(1, N, 1, L, w, 0, 8)[0])
    env.check_errors()
    # the drop-in env raises at the step that overflows
    e = BeerGameEnv({})
    e.reset()
    e.step([2 ** 30] * 4)
    with pytest.raises(OverflowError):
        e.step([2 ** 30] * 4)
    # ... and reset() scopes the flag to the episode: the next episode is exact again
    e.reset()
    for w in range(35):
        e.step([1, 2, 3, 4])


@pytest.mark.parametrize("slab", [True, False])
def test_overflow_flag_is_cleared_by_reset(slab):
    """An overflowing action makes that episode invalid, not the env: reset() clears the
    device word and its host-mapped copy in stream order."""
    from gym_supplychain_amd import BeerGameVecEnv
    N, L, T = 256, 4, 35
    env = BeerGameVecEnv(N, {}, demand="poisson", device=DEV, state_slab=slab)   # auto-reset
    env.reset()
    big = torch.full((N, L), 2 ** 30, dtype=torch.int32, device=DEV)
    acts = _uniform_actions_dev(5, N, T, L, 0, 0, 8)
    env.step(big)
    env.step(big)
    with pytest.raises(OverflowError):
        env.check_errors()
    env.reset()                                  # episode 1 starts clean
    for ep in range(3):                          # three whole episodes, terminal polls included
        for w in range(T):
            env.step(acts[w])
    env.check_errors()
    torch.cuda.synchronize()
    assert env._err_word.value == 0


def test_action_cache_sees_metadata_changes():
    """A validated action tensor whose strides change in place (same data pointer) is
    validated again instead of being read as a contiguous [N, L] buffer."""
    from gym_supplychain_amd import BeerGameVecEnv
    N, L = 4, 4
    env = BeerGameVecEnv(N, {}, device=DEV, auto_reset=False)
    env.reset()
    a = torch.arange(N * L, dtype=torch.int32, device=DEV).view(N, L)
    env.step(a)                                  # the action lands in orders_placed (:121)
    ref = env.orders_placed.clone()
    env.reset()
    a.t_()                                       # same pointer, transposed strides
    env.step(a)
    got = env.orders_placed.clone()
    env.reset()
    env.step(a.contiguous())
    want = env.orders_placed.clone()
    assert torch.equal(got, want) and not torch.equal(got, ref)
    # resize_ to fewer rows keeps the pointer and the stride (L, 1): the shape check refuses it
    b = torch.arange(N * L, dtype=torch.int32, device=DEV).view(N, L)
    env.reset()
    env.step(b)
    b.resize_((N - 1, L))
    env.reset()
    with pytest.raises(ValueError):
        env.step(b)


def test_overflow_reported_at_next_terminal_step_and_by_other_kernels():
    from gym_supplychain_amd import BeerGame2VecEnv, BeerGameVecEnv
    N, L, T = 512, 4, 35
    env = BeerGameVecEnv(N, {}, device=DEV)     # auto-reset
    env.reset()
    big = torch.full((N, L), 2 ** 30, dtype=torch.int32, device=DEV)
    zero = torch.zeros((N, L), dtype=torch.int32, device=DEV)
    for w in range(T):                          # overflow in episode 0; its terminal launch exports the flag
        env.step(big if w < 3 else zero)
    torch.cuda.synchronize()                    # (a host running ahead of the GPU would see it later)
    with pytest.raises(OverflowError):
        for w in range(T):                      # raised by episode 1's terminal step
            env.step(zero)
    # rollout kernel
    env = BeerGameVecEnv(N, {}, device=DEV, auto_reset=False)
    env.reset()
    env.rollout(big.unsqueeze(0).expand(4, N, L).contiguous())
    with pytest.raises(OverflowError):
        env.check_errors()
    # BeerGameEnv2 kernel: penalty 2^30 per unit beyond max_stock
    v2 = BeerGame2VecEnv(N, exceeded_capacity_penalty=2 ** 30, max_stock=1, device=DEV, auto_reset=False)
    v2.reset()
    v2.step(zero)
    with pytest.raises(OverflowError):
        v2.check_errors()


def test_episode_return_gather_snapshot_on_device():
    """EpisodeReturnGather with one process: the per-env returns of a finished episode are
    snapshotted on the launch stream (a device-to-device hipMemcpyAsync) and survive the next
    episode overwriting the env's own buffer."""
    from gym_supplychain_amd import BeerGameVecEnv
    from gym_supplychain_amd.distributed import EpisodeReturnGather
    N, T = 4096, 35
    env = BeerGameVecEnv(N, {}, demand="poisson", poisson_lambda=8.0, seed=3, device=DEV, auto_reset=True,
                         track_returns=True)
    gather = EpisodeReturnGather(N, DEV)
    env.reset()
    acts = torch.randint(0, 9, (T, N, 4), dtype=torch.int32, device=DEV)
    finals = []
    for ep in range(2):
        for w in range(T):
            _, _, _, info = env.step(acts[w])
            if info:
                gather.on_episode_end(info["episode_return"])
                finals.append(info["episode_return"].clone())
                if ep == 0:
                    snap = gather.result()
                    first = snap.clone()
    torch.cuda.synchronize()
    assert torch.equal(first, finals[0].to(torch.int64))
    assert torch.equal(gather.result(), finals[1].to(torch.int64)) and gather.gathers == 2
