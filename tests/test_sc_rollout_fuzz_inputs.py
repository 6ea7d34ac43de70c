"""The inputs of the fused-rollout fuzz (tests/test_gpu_sc_rollout_fuzz.py), checked on the host.

scg_sc_prepare must derive exactly the shape tests/sc_rollout_cases.py writes down for every
chain, and the kernel it expects: a later change to tests/sc_fuzz.py or to the admission rules
fails here and cannot silently move the device tests off the code paths they are there for. And
the closed loop's reference (tests/sc_closed_ref.py) alone, run with the parameters and noise the
device tests use, must cross two episode ends, stop mid-episode and take every branch of the
formulas: conditions on the inputs, not re-derived from the device's output."""
import numpy as np
import pytest

import sc_rollout_cases as rc
from sc_closed_ref import HI, LO

IDS = [f"seed{c.seed}" for c in rc.CASES]


def test_the_table_reaches_what_it_is_there_for():
    """The properties the chains were picked for, stated on the table itself."""
    by = rc.BY_SEED
    assert len(rc.NODES_CASES) == 12 and len(rc.STAGED_CASES) == 2
    assert min(c.waves for c in rc.NODES_CASES) == 5 and {c.waves for c in rc.NODES_CASES} == {5, 6, 7, 8}
    assert [c.seed for c in rc.NODES_CASES if c.nodes > c.waves] == [6, 10, 38, 57]      # a wave owns two nodes
    assert [c.seed for c in rc.NODES_CASES if c.A > 4 * c.waves] == [36]                 # the stage's tail loop
    assert by[47].A == 4 * by[47].waves - 1
    assert [c.seed for c in rc.NODES_CASES if c.A > 2 * c.waves] == [36, 47, 48, 30, 6, 10, 38, 57]  # the noise tail
    assert by[6].O == 32 and by[2].O > 32 and -(-by[33].O // 32) == 5                    # chunks of 32 observations
    assert rc.hidden_bound(by[13]) == 20 and rc.hidden_bound(by[38]) == 70
    assert {c.P for c in rc.NODES_CASES} == {1, 2, 3}
    assert min(c.heap_cap for c in rc.NODES_CASES) == 2 and max(c.heap_cap for c in rc.NODES_CASES) == 12
    assert any(c.stochastic and c.avg_lt == 1 for c in rc.NODES_CASES)
    assert by[57].bucket == 4 and by[57].nodes > by[57].waves
    assert [c.seed for c in rc.NODES_CASES if not c.f64] == [48]
    assert all(rc.dtypes(c, cfg) for c in rc.CASES for cfg in [None] + rc.closed_configs(c))
    assert [c.seed for c in rc.CASES if "f32" in rc.dtypes(c)] == [13, 36, 48, 6]
    assert all(rc.dtypes(c, cfg) == ["f64"] + ["f32"] * (c.seed in (13, 36, 6) and cfg == rc.closed_configs(c)[-1])
               for c in rc.NODES_CASES if c.f64 for cfg in rc.closed_configs(c))
    assert all(rc.dtypes(rc.BY_SEED[48], cfg) == ["f32"] for cfg in [None] + rc.closed_configs(rc.BY_SEED[48]))
    assert rc.T == 6 and rc.K == 15 and rc.N_ENVS == 130 and rc.SAMPLE == (0, 63, 64, 129)


@pytest.mark.parametrize("case", rc.CASES, ids=IDS)
def test_prepare_reports_the_tables_shape(case):
    from gym_supplychain_amd import _native as nat
    nodes, env_kw = rc.chain(case)
    assert env_kw["total_time_steps"] == rc.T and env_kw["num_products"] == case.P
    assert (env_kw["stochastic_leadtimes"], env_kw["avg_leadtime"], env_kw["max_leadtime"]) == \
        (case.stochastic, case.avg_lt, case.max_lt)
    for f64 in (True, False):
        admitted = case.kernel == "nodes" and (case.f64 or not f64)
        r, c, err = rc.prepare(case, "nodes", f64)
        if not admitted:
            assert r == nat.SCG_ERR_INVALID and rc.LDS_MESSAGE in err, (case.seed, f64, err)
        else:
            assert r == 0, (case.seed, f64, err)
            assert c.kernel == nat.SC_KERNEL_NODES
            assert (c.n_nodes, c.group, c.n_products, c.n_actions, c.n_obs, c.heap_capacity, c.inbox_size) == \
                (case.nodes, case.waves, case.P, case.A, case.O, case.heap_cap, case.inbox), (case.seed, f64)
            assert c.group == min(case.nodes, 8)
        r, c, err = rc.prepare(case, "auto", f64)
        assert r == 0, err
        assert (c.n_nodes, c.n_products, c.n_actions, c.n_obs, c.heap_capacity) == \
            (case.nodes, case.P, case.A, case.O, case.heap_cap)
        d = c.max_dests
        assert (2 if d <= 2 else 4 if d <= 4 else 8) == case.bucket
        if case.kernel == "staged":
            assert c.kernel == nat.SC_KERNEL_STAGED and c.inbox_size == case.inbox


def _configs():
    return [pytest.param(c, cfg, id=f"seed{c.seed}-{rc.config_id(cfg)}") for c in rc.CASES for cfg in rc.closed_configs(c)]


@pytest.mark.parametrize("case, cfg", _configs())
def test_the_closed_loops_inputs_take_every_branch(case, cfg):
    policy, hidden, shared, sampled = cfg
    if policy == "mlp" and case.kernel == "nodes":
        assert hidden <= 64 and (hidden <= rc.hidden_bound(case))
    refs = rc.reference(case, cfg)
    assert sorted(refs) == sorted(rc.SAMPLE)
    for n, r in refs.items():
        assert r.actions.shape == (rc.K, case.A) and r.actions.dtype == np.float32
        assert r.obs.shape == (rc.K, case.O) and r.obs.dtype == np.float64
        assert int(r.dones.sum()) >= 2 and sorted(r.term_obs) == list(np.flatnonzero(r.dones))  # two episode ends ...
        assert not r.dones[-1] and 0 < r.time_step < rc.T and r.episode == 2                   # ... and ends mid-episode
        assert np.isfinite(r.rewards).all() and np.isfinite(r.obs).all() and np.isfinite(r.actions).all()
    acts = np.stack([r.actions for r in refs.values()])
    assert (acts == LO).any() and (acts == HI).any() and ((acts > LO) & (acts < HI)).any()     # the clamp's three branches
    if policy == "mlp":
        hid = np.stack([r.hidden for r in refs.values()])
        assert hid.shape[-1] == hidden and (hid == 0).any() and (hid > 0).any()                # the ReLU's two
    if sampled:
        _, eps, std = rc.policy_inputs(case, cfg)
        assert (std == 0).sum() >= 1 and (std > 0).any() and eps.shape == (rc.K, rc.N_ENVS, case.A)
        u = np.stack([r.samples for r in refs.values()])
        assert u.shape == acts.shape and np.isfinite(u).all()
    else:
        assert all(r.samples is None for r in refs.values())


@pytest.mark.parametrize("case", rc.CASES, ids=IDS)
def test_the_open_loops_reference(case):
    """The open loop's actions lie a little outside the Box on both sides, and its reference crosses
    the same two episode ends."""
    acts = rc.open_loop_actions(case)
    assert acts.shape == (rc.K, rc.N_ENVS, case.A) and acts.dtype == np.float32
    assert (acts < -1).any() and (acts > 1).any() and acts.min() >= -1.1 and acts.max() <= np.float32(1.1)
    for n, r in rc.reference(case).items():
        assert np.array_equal(rc.bits(r.actions), rc.bits(acts[:, n]))
        assert sorted(r.term_obs) == [5, 11] and r.time_step == 3 and r.episode == 2
