"""BeerGameVecEnv / BeerGame2VecEnv .rollout_policy(noise_seed=, noise_row=) and .draw_noise
(scg_bg_rollout_drawn: bg_rollout_kernel with MlpDrawnArgs as its source, both variants, ring in
LDS or in HBM; scg_bg_noise_fill).

Three kinds of evidence, every comparison exact and the samples bit for bit:
  - draw_noise() against the NumPy statement of the noise (tests/noise_ref.py rows);
  - the seeded loop against the tensor loop fed draw_noise()'s rows, on twin envs, for every
    sampled case of tests/test_gpu_bg_mlp_policy.py and three more at L = 2, 3 and 5;
  - the seeded loop against the per-env CPU oracles and the NumPy float32 MLP fed noise_ref.rows
    (no device-produced noise enters the expected side).
N = 300 is one full 256-lane block and a 44-lane tail; T = 12."""
import functools

import numpy as np
import pytest
import torch

import noise_ref
from test_gpu_bg_local_policy import DEV, INVENTORY, LIST_DELAYS, T, _assert_same_state, _env2
from test_gpu_bg_mlp_policy import (CASES, HBM_DELAYS, N, STOCHASTIC, _assert_refused_then_steps_on, _case, _clip, _make_env,
                                    _make_oracles, _network, _small)

pytestmark = pytest.mark.gpu

NEW_CASES = {
    "v2-L2-H16-gauss-drawn-list": _case(2, 2, 16, "gauss", True, seed=11),
    "v1-L3-H16-gauss-drawn-list": _case(1, 3, 16, "gauss", True, clip=(-3, 12), seed=12),
    "v2-L5-H16-gauss-drawn-stochastic": _case(2, 5, 16, "gauss", True, STOCHASTIC, seed=13),
}
SAMPLED = {**{k: c for k, c in CASES.items() if c["sampled"]}, **NEW_CASES}
# (noise_seed, noise_row) per case; the 140-week case has row != 0 so that the second launch's first row counts
DRAW = {name: (0x9E3779B97F4A7C15 ^ (i * 0x1000193), (0, 5, 2 ** 32 - 200, 1000)[i % 4]) for i, name in enumerate(SAMPLED)}
DRAW["v1-L4-H16-gauss-sampled-140"] = (2 ** 64 - 1, 2 ** 32 - 140)   # the call ends on the last row
FIELDS = ("samples", "actions", "obs", "rewards", "features", "reward_sum")


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _mlp(env, c):
    w1, b1, w2, b2, std, _ = _network(c)
    return env.pack_local_mlp(*(torch.as_tensor(x) for x in (w1, b1, w2, b2))), torch.as_tensor(std)


def _run(env, c, K, samples=True, full=True, **kw):
    packed, std = _mlp(env, c)
    if samples:
        kw["samples_out"] = torch.empty((K, env.n_envs, env.levels), dtype=torch.float32, device=DEV)
    return env.rollout_policy(packed, None, K, clip=c["clip"], std=kw.pop("std", std), return_actions=full, return_obs=full,
                              return_rewards=full, return_features=full, **kw)


def _assert_same_result(a, b, rows=slice(None), envs=slice(None), samples=True):
    """Result a equals rows `rows`, envs `envs` of result b."""
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if f == "samples" and not samples:
            continue
        assert x is not None and y is not None, f
        y = y[envs] if f == "reward_sum" else y[rows, envs]
        assert x.dtype == y.dtype and x.shape == y.shape, f
        if f == "samples":
            assert np.array_equal(_bits(x), _bits(y)), f
        else:
            assert torch.equal(x, y), f


# ---- 1. draw_noise is the reference ----------------------------------------------------------------
@pytest.mark.parametrize("env_offset", [0, 64])
@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 8])
def test_draw_noise_equals_the_numpy_rows(L, env_offset):
    env = _env2(N, levels=L, initial_inventory=INVENTORY[:L], env_offset=env_offset)
    env.reset()
    K = 3
    for i, row in enumerate((0, 5, 2 ** 32 - 3)):
        seed = (2 ** 64 - 1, 0, 0x0123456789ABCDEF)[i]
        got = env.draw_noise(seed, K, row)
        assert got.dtype == torch.float32 and tuple(got.shape) == (K, N, L) and got.device.type == "cuda"
        want = noise_ref.rows(seed, K, N, L, row0=row, env_offset=env_offset)
        assert np.array_equal(_bits(got), want.view(np.uint32)), (L, row)
        out = torch.empty_like(got)
        assert env.draw_noise(seed, K, row, out=out) is out and torch.equal(out, got)
    assert tuple(env.draw_noise(7, 0).shape) == (0, N, L)
    env.check_errors()


def test_draw_noise_on_the_variant_1_env():
    c = CASES["v1-L4-H16-gauss-sampled-list"]
    env = _make_env(c)
    env.reset()
    got = env.draw_noise(3, 2, 9)
    assert np.array_equal(_bits(got), noise_ref.rows(3, 2, N, 4, row0=9).view(np.uint32))


# ---- 2. the seeded loop is the tensor loop ---------------------------------------------------------
@pytest.mark.parametrize("name", list(SAMPLED))
def test_seeded_equals_the_tensor_loop(name):
    c = SAMPLED[name]
    K = c["K"]
    seed, row = DRAW[name]
    env, twin = _make_env(c), _make_env(c)
    in_lds = env.ring_slots * c["L"] * 256 * 4 <= 64 * 1024
    assert in_lds == (c["delays"] is not HBM_DELAYS)
    env.reset()
    twin.reset()
    noise = twin.draw_noise(seed, K, row)
    kept = noise.clone()
    want = _run(twin, c, K, noise=noise)
    got = _run(env, c, K, noise_seed=seed, noise_row=row)
    _assert_same_result(got, want)
    _assert_same_state(env, twin)
    assert (env.week, env.episode) == (K % c["weeks"], K // c["weeks"])
    assert torch.equal(noise, kept)
    # u = z + std * eps with eps the drawn rows: the noise did enter
    assert not np.array_equal(_bits(got.samples), _bits(_run(_reset(_make_env(c)), c, K, noise_seed=seed ^ 1, noise_row=row).samples))
    env.check_errors()


def _reset(env):
    env.reset()
    return env


def test_the_cases_cover_the_grid():
    cs = list(SAMPLED.values())
    assert {c["L"] for c in cs} >= {1, 2, 3, 4, 5, 8}
    for variant in (1, 2):
        assert any(c["variant"] == variant for c in cs) and any(c["variant"] == variant for c in NEW_CASES.values())
    assert any(c["delays"] is HBM_DELAYS for c in cs) and any(c["delays"] is LIST_DELAYS for c in cs)
    assert any(c["delays"] is STOCHASTIC and c["K"] > T for c in cs)          # auto-reset inside the call
    assert any(c["delays"] is STOCHASTIC for c in NEW_CASES.values())
    big = [n for n, c in SAMPLED.items() if c["K"] > 128]                      # across the launch cut, rows counted on
    assert big and all(DRAW[n][1] != 0 for n in big)
    assert all(0 <= DRAW[n][1] and DRAW[n][1] + c["K"] <= 2 ** 32 for n, c in SAMPLED.items())


# ---- 3. against the formula directly: the oracles fed noise_ref.rows -------------------------------
ORACLE_DRAW = {"v1-L4-H16-gauss-sampled-list": (41, 3), "v2-L4-H16-gauss-sampled-stochastic": (2 ** 63 + 5, 2 ** 32 - 100)}


@functools.lru_cache(maxsize=None)
def _oracle_plan(name):
    """The case's expected streams over its K weeks from reset with eps = noise_ref.rows, from the
    per-env oracles and the NumPy float32 MLP: computed once and left unchanged."""
    c = CASES[name]
    K, n, L = c["K"], c["n"], c["L"]
    seed, row = ORACLE_DRAW[name]
    *net, std, _ = _network(c)
    noise = noise_ref.rows(seed, K, n, L, row0=row)
    lo, hi = _clip(c)
    orc = _make_oracles(c, K // c["weeks"] + 2)
    orc.reset()
    out = dict(features=[], samples=[], actions=[], obs=[], rewards=[])
    for k in range(K):
        f, u, a = orc.act_mlp(net, lo, hi, std, noise[k])
        o, r = orc.step(a)
        for key, v in zip(out, (f, u, a, o, r)):
            out[key].append(v)
    return {key: np.stack(v) for key, v in out.items()}


@pytest.mark.parametrize("name", list(ORACLE_DRAW))
def test_seeded_equals_the_oracles_fed_the_numpy_rows(name):
    c, want = CASES[name], _oracle_plan(name)
    seed, row = ORACLE_DRAW[name]
    env = _make_env(c)
    env.reset()
    res = _run(env, c, c["K"], noise_seed=seed, noise_row=row)
    assert np.array_equal(_bits(res.samples), want["samples"].view(np.uint32))
    for f in ("actions", "obs", "rewards", "features"):
        assert np.array_equal(getattr(res, f).cpu().numpy(), want[f]), f
    assert np.array_equal(res.reward_sum.cpu().numpy(), want["rewards"].sum(0))
    env.check_errors()


# ---- 4. a shard draws its rows of the batch --------------------------------------------------------
def test_a_shard_draws_its_rows_of_the_batch():
    c = CASES["v2-L4-H16-gauss-sampled-stochastic"]
    K, (seed, row) = c["K"], (77, 2 ** 32 - 50)
    batch = _make_env(c)
    shard = _env2(100, levels=c["L"], initial_inventory=INVENTORY[:c["L"]], shipment_delays=c["delays"], weeks=c["weeks"],
                  env_offset=64)
    assert (shard.env_offset, shard.n_envs, batch.n_envs) == (64, 100, N)
    batch.reset()
    shard.reset()
    whole = _run(batch, c, K, noise_seed=seed, noise_row=row)
    part = _run(shard, c, K, noise_seed=seed, noise_row=row)
    _assert_same_result(part, whole, envs=slice(64, 164))
    assert np.array_equal(_bits(shard.draw_noise(seed, K, row)), _bits(batch.draw_noise(seed, K, row)[:, 64:164]))
    for t in ("inventory", "backlog", "orders_placed"):
        assert torch.equal(getattr(shard, t), getattr(batch, t)[64:164]), t


# ---- 5. rows count on across calls and resets ------------------------------------------------------
def test_cut_calls_count_the_rows_on():
    name = "v2-L4-H16-gauss-sampled-stochastic"   # two episodes and three weeks
    c = CASES[name]
    K, (seed, row) = c["K"], (2 ** 40 + 9, 2 ** 32 - 1000)
    one, cut = _make_env(c), _make_env(c)
    one.reset()
    cut.reset()
    whole = _run(one, c, K, noise_seed=seed, noise_row=row)
    for k0, k1 in ((0, 5), (5, 7), (7, K)):
        part = _run(cut, c, k1 - k0, noise_seed=seed, noise_row=row + k0)
        for f in FIELDS[:-1]:
            x, y = getattr(part, f), getattr(whole, f)[k0:k1]
            assert np.array_equal(_bits(x), _bits(y)) if f == "samples" else torch.equal(x, y), (f, k0)
        assert torch.equal(part.reward_sum, whole.rewards[k0:k1].sum(0, dtype=torch.int64))
        assert (cut.week, cut.episode) == (k1 % T, k1 // T)
    _assert_same_state(cut, one)


def test_the_week_after_an_auto_reset_uses_the_next_row_not_row_zero():
    name = "v2-L4-H16-gauss-sampled-stochastic"
    c = CASES[name]
    K, (seed, row) = c["K"], (12345, 17)
    assert K > T
    env = _make_env(c)
    env.reset()
    res = _run(env, c, K, noise_seed=seed, noise_row=row)
    # week T of the call starts from the reset state: its features are week 0's, so z is week 0's
    # and u - z = std * eps differs exactly when the row differs
    assert torch.equal(res.features[T], res.features[0])
    twin = _make_env(c)
    twin.reset()
    noise = torch.as_tensor(noise_ref.rows(seed, K, c["n"], c["L"], row0=row), device=DEV)
    want = _run(twin, c, K, noise=noise)
    assert np.array_equal(_bits(res.samples[T]), _bits(want.samples[T]))      # row noise_row + T
    wrong = noise.clone()
    wrong[T] = noise[0]                                                        # what restarting the rows would draw
    twin2 = _make_env(c)
    twin2.reset()
    assert not np.array_equal(_bits(res.samples[T]), _bits(_run(twin2, c, K, noise=wrong).samples[T]))
    assert (env.week, env.episode) == (K % T, K // T)


# ---- 6. std = 0 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v2-L4-H16-gauss-sampled-stochastic", "v1-L4-H16-gauss-sampled-list"])
def test_std_zero_is_the_deterministic_loop(name):
    c = CASES[name]
    K = c["K"]
    env, twin = _make_env(c), _make_env(c)
    env.reset()
    twin.reset()
    got = _run(env, c, K, noise_seed=99, noise_row=4, std=0.0)
    packed, _ = _mlp(twin, c)
    want = twin.rollout_policy(packed, None, K, clip=c["clip"], return_actions=True, return_obs=True, return_rewards=True,
                               return_features=True)
    for f in ("actions", "obs", "rewards", "features", "reward_sum"):   # the samples may differ in the sign of a zero
        assert torch.equal(getattr(got, f), getattr(want, f)), f
    _assert_same_state(env, twin)


# ---- 7. the last rows ------------------------------------------------------------------------------
def test_the_call_may_end_on_the_last_row():
    c = NEW_CASES["v2-L2-H16-gauss-drawn-list"]
    K, seed = 5, 2 ** 64 - 1
    row = 2 ** 32 - K
    env, twin = _make_env(c), _make_env(c)
    env.reset()
    twin.reset()
    noise = env.draw_noise(seed, K, row)
    assert np.array_equal(_bits(noise), noise_ref.rows(seed, K, c["n"], c["L"], row0=row).view(np.uint32))
    got = _run(env, c, K, noise_seed=seed, noise_row=row)
    want = _run(twin, c, K, noise=noise)
    _assert_same_result(got, want)
    _assert_same_state(env, twin)
    with pytest.raises(ValueError):
        _run(env, c, K, noise_seed=seed, noise_row=row + 1)
    with pytest.raises(ValueError):
        env.draw_noise(seed, K, row + 1)
    _assert_same_state(env, twin)


# ---- 8. argument errors ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [1, 2])
def test_python_argument_errors(variant):
    c, net = _small(variant)
    n, L, K = c["n"], c["L"], 2
    make = functools.partial(_make_env, c)
    clip = (0, 30)
    noise = lambda: torch.zeros((K, n, L), dtype=torch.float32, device=DEV)  # noqa: E731
    run = lambda e, **kw: e.rollout_policy(e.pack_local_mlp(*net), None, K, **{"clip": clip, **kw})  # noqa: E731
    bad_calls = [
        lambda e: run(e, noise=noise(), noise_seed=7, std=0.5),               # noise with noise_seed
        lambda e: run(e, noise_seed=7),                                       # noise_seed without std
        lambda e: run(e, noise_seed=7, samples_out=noise()),
        lambda e: run(e, noise_seed=True, std=0.5),
        lambda e: run(e, noise_seed=-1, std=0.5),
        lambda e: run(e, noise_seed=2 ** 64, std=0.5),
        lambda e: run(e, noise_seed=7.0, std=0.5),
        lambda e: run(e, noise_seed=7, noise_row=-1, std=0.5),
        lambda e: run(e, noise_seed=7, noise_row=True, std=0.5),
        lambda e: run(e, noise_seed=7, noise_row=2 ** 32 - K + 1, std=0.5),
        lambda e: run(e, noise_seed=7, std=-1.0),
        lambda e: run(e, noise_seed=7, std=0.5, samples_out=noise()[:1]),
    ]
    W4, b4 = np.array([[-1, -1, 0, 0]] * L, dtype=np.int32), np.full(L, 40, dtype=np.int32)
    for pack in (lambda e: e.pack_local_policy(W4, b4), lambda e: e.pack_policy(np.zeros((L, L), dtype=np.int32), b4)):
        bad_calls += [lambda e, pack=pack: e.rollout_policy(pack(e), None, K, clip=clip, noise_seed=7),
                      lambda e, pack=pack: e.rollout_policy(pack(e), None, K, clip=clip, noise_seed=7, std=0.5)]
    for call in bad_calls:
        _assert_refused_then_steps_on(make, call)
    # the good call, for contrast: samples_out is optional
    env = make()
    env.reset()
    res = run(env, noise_seed=7, std=0.5, noise_row=2 ** 32 - K)
    assert res.samples is None and res.actions is None and res.reward_sum.dtype == torch.int64
    none = env.rollout_policy(env.pack_local_mlp(*net), None, 0, clip=clip, noise_seed=7, std=0.5, noise_row=2 ** 32)
    assert not none.reward_sum.any() and env.week == K   # no weeks: no rows, whatever the first row
