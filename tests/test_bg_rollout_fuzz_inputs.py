"""The inputs of the BeerGame fused-rollout fuzz (tests/test_gpu_bg_rollout_fuzz.py), checked on the
host.

scg_bg_prepare must give every game of tests/bg_rollout_cases.py the ring it writes down, on the
side of the 64 KiB LDS limit it is there for, with a plan that takes all four modes: a later change
to the generator fails here and cannot silently move the device tests off the code paths they are
there for. And the reference alone (one CPU oracle per sampled env, the NumPy restatements of the
three policies) must cross two episode ends, stop mid-episode, fit int32 and take every branch of
the formulas: conditions on the inputs, none re-derived from the device's output. No case is
skipped or excepted; two conditions cannot hold by construction and are not asked: the
upstream-backlog term where no action is taken with a backlog (one level; T = 1, where every
action follows a reset), and a zero among the standard deviations of one level."""
import numpy as np
import pytest

import bg_local_ref
import bg_rollout_cases as rc

MODE_DIRECT, MODE_STORE, MODE_ADD, MODE_DROP = range(4)   # csrc/scg_bg_plan.h


def _ids(games):
    return [g.name for g in games]


def test_the_table_is_the_grid():
    """The grid statements, on the table itself."""
    main = rc.MAIN
    assert [(g.L, g.ring) for g in main] == [(L, ring) for L in range(1, 9) for ring in ("lds", "hbm")]
    assert [g.R for g in main] == [64, 65, 32, 33, 21, 22, 16, 17, 12, 13, 10, 11, 9, 10, 8, 9]
    assert all(g.R == rc.ring_slots(g.L, g.ring) for g in main + rc.OPEN_ONLY)
    assert all(g.T >= g.R - 1 + 3 for g in main + rc.OPEN_ONLY)
    by = rc.BY_NAME
    assert by["1-hbm"].R - 1 == 64 == bg_local_ref.MAX_DELAY and by["1-hbm"].delays2 == "list"
    assert all(rc.weeks_per_call(g) > 128 for g in main if g.L <= 2)                 # across the launch cut
    assert [g.demand1 for g in main[:3]] == ["fixed", "poisson", "table"]
    assert all(g.demand1 == main[i % 3].demand1 for i, g in enumerate(main))           # rotates over the games
    assert all(g.demand2 == ("fixed", "uniform")[i % 2] for i, g in enumerate(main))
    assert all((g.delays2 == "stochastic") == ((g.ring == "lds") == (g.L % 2 == 1)) for g in main)
    assert sum(g.delays2 == "stochastic" for g in main) == 8
    assert all(g.recipe == ("gauss", "tie")[i % 2] for i, g in enumerate(rc.CLOSED_GAMES))
    widths = {g.H for g in rc.CLOSED_GAMES}
    assert widths >= {1, 16, 33, 64} and len(widths - {1, 16, 33, 64}) >= 2 and max(widths) <= 64
    assert [(g.L, g.T, g.ring) for g in rc.TINY] == [(5, 1, "lds"), (6, 2, "lds")]
    assert [g.L for g in rc.OPEN_ONLY] == list(range(9, 17)) and {g.ring for g in rc.OPEN_ONLY} == {"lds", "hbm"}
    for games in (rc.TINY, rc.OPEN_ONLY):
        assert {g.demand1 for g in games} >= {"poisson", "table"} and {g.demand2 for g in rc.OPEN_ONLY} == {"fixed", "uniform"}
    assert {g.delays2 for g in rc.OPEN_ONLY} == {"list", "stochastic"}
    assert len(rc.case_ids()) == 5 * 2 * 18 + 16
    assert rc.N_ENVS == 260 and rc.SAMPLE == (0, 63, 64, 255, 256, 259)
    assert all(rc.N_ENVS * g.L % 4 == 0 for g in rc.GAMES)                            # the twin's slab step kernel


@pytest.mark.parametrize("g", rc.GAMES, ids=_ids(rc.GAMES))
def test_the_generator_draws_the_tables_game(g):
    game = rc.game_of(g)
    assert (game["levels"], game["ring_slots"], game["weeks"]) == (g.L, g.R, g.T)
    assert game == rc.random_game(g.L, g.ring, g.seed, T=g.T if g in rc.TINY else None)
    inv, delays = game["initial_inventory"], game["delays"]
    assert len(inv) == g.L and -5 <= min(inv) and 30 <= max(inv) <= 39 and (g.L == 1 or min(inv) < 0)
    assert 0 <= game["initial_shipment_value"] <= 11 and 0 <= game["initial_orders_value"] <= 11
    assert 0 <= game["inv_cost"] <= 5 and 0 <= game["backlog_cost"] <= 5
    assert len(delays) == len(game["demand"]) == g.T and max(delays) == g.R - 1
    assert 0 <= min(game["demand"]) and max(game["demand"]) < rc.DEMAND_HI
    if g not in rc.TINY:
        assert 0 in delays and sorted(delays)[-2] <= 4 and delays.index(g.R - 1) + 1 == game["long_week"] <= 2
        assert game["arrival"] == game["long_week"] + g.R - 1 <= g.T - 1                 # lands inside the episode
        assert sum(w + d == game["arrival"] for w, d in enumerate(delays, 1) if d) >= 2  # a second week ships into it
        assert delays[-1] >= 1                                                           # lands past T
    c1, c2 = rc.cuts(g)
    assert 1 <= c1 < c2 == g.T + 1 < rc.weeks_per_call(g) and (c1 < g.T or g.T == 1)


@pytest.mark.parametrize("g", rc.GAMES, ids=_ids(rc.GAMES))
def test_prepare_gives_the_tables_ring_and_every_mode(g):
    """ring_slots of both variants, its side of the LDS limit, and (delay lists) DIRECT, STORE,
    ADD and DROP among the plan words; the tiny games' two weeks have what two weeks can."""
    for variant in rc.VARIANTS:
        slots, plan = rc.prepare(g, variant)
        assert slots == g.R, (g.name, variant)
        assert (slots * g.L * 256 * 4 <= rc.LDS_BYTES) == (g.ring == "lds")
        if rc.stochastic(g, variant):
            continue
        game = rc.game_of(g)
        assert [p >> 8 for p in plan] == game["delays"]
        modes = {p & 3 for p in plan}
        if g in rc.TINY:
            assert modes == ({MODE_DROP} if g.T == 1 else {MODE_DROP, MODE_DIRECT})
        else:
            assert modes == {MODE_DIRECT, MODE_STORE, MODE_ADD, MODE_DROP}
            assert plan[game["long_week"] - 1] & 3 == MODE_STORE and plan[-1] & 3 == MODE_DROP
            assert any(p & 3 == MODE_ADD and w + (p >> 8) == game["arrival"] for w, p in enumerate(plan, 1))
            assert plan[game["arrival"] - 1] & 4                                         # PLAN_ARRIVE
    if g.ring == "hbm" or g in rc.TINY:
        return
    assert (g.R + 1) * g.L * 256 * 4 > rc.LDS_BYTES                                     # the last ring that fits


def _cases():
    return [pytest.param(g, v, loop, id=rc.case_id(g, v, loop)) for g, v, loop in rc.case_ids()]


@pytest.mark.parametrize("g, variant, loop", _cases())
def test_the_reference_takes_every_branch(g, variant, loop):
    ref = rc.reference(g, variant, loop)
    K, n, L = rc.weeks_per_call(g), len(rc.SAMPLE), g.L
    assert ref["actions"].shape == ref["obs"].shape == (K, n, L) and ref["rewards"].shape == (K, n)
    assert ref["largest"] < 2 ** 31 - 1                                  # shipments, ledgers and reward_sum included
    assert ref["ends"] >= 2 and (ref["week"], ref["episode"]) == (K % g.T, K // g.T)
    assert 0 < ref["week"] < g.T or g.T == 1
    assert rc.missing(g, variant, loop) == [], rc.case_id(g, variant, loop)
    inp = rc.inputs(g, variant, loop)
    lo, hi = rc.clip_of(variant, loop)
    a = ref["actions"]
    if loop == "open":
        assert np.array_equal(a, inp["actions"][:, list(rc.SAMPLE)])
        return
    assert (a == lo).any() and (a == hi).any() and ((a > lo) & (a < hi)).any() and a.min() >= lo and a.max() <= hi
    if loop in ("local", "mlp", "mlp-sampled"):
        assert ref["features"].shape == (K, n, L, 4) and ref["features"].dtype == np.int32
    if loop in ("linear", "local"):
        assert inp["W"].shape == (rc.N_ENVS, L, L if loop == "linear" else 4) and np.abs(inp["W"]).max() <= 64
        assert np.abs(inp["b"]).max() <= 2000
    else:
        w1, b1, w2, b2 = inp["net"]
        assert w1.shape == (g.H, 4 * L) and w2.shape == (L, g.H) and all(x.dtype == np.float32 for x in inp["net"])
    if loop == "mlp-sampled":
        std, noise, u = inp["std"], inp["noise"], ref["samples"]
        assert noise.shape == (K, rc.N_ENVS, L) and u.shape == (K, n, L) and np.isfinite(u).all()
        assert (std > 0).any() and int((std == 0).sum()) == (1 if L > 1 else 0)
    else:
        assert ref["samples"] is None
