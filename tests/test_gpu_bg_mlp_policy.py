"""BeerGameVecEnv / BeerGame2VecEnv .rollout_policy with a pack_local_mlp() result
(scg_bg_rollout_mlp: bg_rollout_kernel with the float32 MLP policy as its source, both variants,
ring in LDS or in HBM, deterministic and sampled).

As in test_gpu_bg_local_policy.py every expected value comes from the CPU oracles, one oracle
object per env: the features from the oracle's attributes (tests/bg_local_ref.py), u and the
actions from the NumPy float32 restatement of the formula (tests/bg_mlp_ref.py), the observations
and rewards from the oracle's own step. The expected side needs no GPU (BeerGameVecEnv reads its
customer demand from a per-env table drawn on the host, BeerGame2VecEnv's Philox draws are
restated by oracle.gen_golden_bg2), is computed once per case and left unchanged. The twin is an
env stepped with step() on the expected actions; before week k its policy_features() must equal
features[k], and at the end it supplies the state tensors. Every comparison is exact, the samples
bit for bit. N = 300 is one full 256-lane block and a 44-lane tail.

Two parameter recipes. "gauss": w1 ~ N/40, b1 ~ N, w2 ~ 2N/sqrt(H), b2 ~ 8 + N, std ~ 2 exp(0.3 N),
noise ~ N: general float32 values, on which a fused multiply-add or another summation order gives
other bits. "tie": w1 in {-1, 0, 1} (about 40 % non-zero), integer b1 in +-20, w2 multiples of
0.5 / max(H // 4, 1), b2 multiples of 0.5 in 4..12, std = 0.5, integer noise in +-6: every value
exact, and u lands on k + 0.5. Each case asserts on its expected side that both bounds, an
interior action, a dead and a live hidden unit, a non-zero in-transit term and (L > 1) a non-zero
upstream-backlog term occur, for "tie" an interior tie and for "gauss" a z whose bits differ from
b2 + w2 @ relu(b1 + w1 @ x) computed in float64 and rounded once."""
import functools

import numpy as np
import pytest
import torch

import bg_local_ref
import bg_mlp_ref
from oracle.beergame import BeerGame2Oracle, BeerGameOracle
from test_gpu_bg_local_policy import DEV, INVENTORY, LIST_DELAYS, SEED, SHIFT, T, Oracles, _assert_same_state, _env2

pytestmark = pytest.mark.gpu
N = 300
F32 = np.float32
HBM_DELAYS = [9 if i == 1 else d for i, d in enumerate(LIST_DELAYS)]   # 10 slots * 8 levels * 1 KiB > 64 KiB
STOCHASTIC = (0, 5)


# ---- the cases ---------------------------------------------------------------------------------------
def _case(variant, L, H, recipe, sampled, delays=LIST_DELAYS, K=T + 5, clip=None, n=N, weeks=T, seed=0):
    return dict(variant=variant, L=L, H=H, recipe=recipe, sampled=sampled, delays=delays, K=K, clip=clip, n=n,
                weeks=weeks, seed=seed)


CASES = {
    # BeerGame2VecEnv, the default clip (0, max_order); two episodes and three weeks: auto-reset inside the call
    "v2-L4-H16-gauss-sampled-stochastic": _case(2, 4, 16, "gauss", True, STOCHASTIC, K=2 * T + 3),
    "v2-L4-H33-tie-sampled-list": _case(2, 4, 33, "tie", True),
    "v2-L4-H16-gauss-det-list": _case(2, 4, 16, "gauss", False),
    "v2-L1-H1-gauss-sampled-list": _case(2, 1, 1, "gauss", True, clip=(4, 12), seed=9),
    "v2-L8-H64-gauss-sampled-lds": _case(2, 8, 64, "gauss", True, seed=2),
    "v2-L8-H16-tie-sampled-hbm": _case(2, 8, 16, "tie", True, HBM_DELAYS),
    "v2-L8-H1-tie-det-stochastic": _case(2, 8, 1, "tie", False, STOCHASTIC, clip=(3, 9), seed=4),
    # BeerGameVecEnv: the actions are increments over the incoming order
    "v1-L4-H16-gauss-sampled-list": _case(1, 4, 16, "gauss", True, clip=(-3, 12), seed=1),
    "v1-L3-H33-gauss-det-list": _case(1, 3, 33, "gauss", False, clip=(-3, 12), seed=1),
    "v1-L1-H64-tie-sampled-list": _case(1, 1, 64, "tie", True, clip=(-3, 12), seed=6),
    "v1-L8-H16-tie-det-hbm": _case(1, 8, 16, "tie", False, HBM_DELAYS, clip=(-3, 12)),
    # 140 weeks in one call: launches of 128 + 12 weeks
    "v1-L4-H16-gauss-sampled-140": _case(1, 4, 16, "gauss", True, [1 + i % 6 for i in range(140)], K=140,
                                         clip=(-3, 12), n=70, weeks=140),
}


def _network(c):
    """(w1, b1, w2, b2, std, noise [K, n, L]) of the case's recipe, float32."""
    L, H, K, n = c["L"], c["H"], c["K"], c["n"]
    rs = np.random.RandomState(1000 * L + H + 7919 * c["seed"])
    if c["recipe"] == "gauss":
        w1, b1 = rs.randn(H, 4 * L) / 40, rs.randn(H)
        w2, b2 = 2 * rs.randn(L, H) / np.sqrt(H), 8 + rs.randn(L)
        std, noise = 2 * np.exp(0.3 * rs.randn(L)), rs.randn(K, n, L)
    else:
        w1 = rs.randint(-1, 2, size=(H, 4 * L)) * (rs.rand(H, 4 * L) < 0.6)
        b1 = rs.randint(-20, 21, size=H)
        w2 = rs.randint(-3, 4, size=(L, H)) * (0.5 / max(H // 4, 1))
        b2 = rs.randint(8, 25, size=L) * 0.5
        std, noise = np.full(L, 0.5), rs.randint(-6, 7, size=(K, n, L))
    return tuple(np.ascontiguousarray(x, dtype=F32) for x in (w1, b1, w2, b2, std, noise))


def _demand1(c):
    """BeerGameVecEnv's per-env customer demand [weeks, n], drawn on the host."""
    return np.random.RandomState(77 + c["L"]).poisson(6.0, size=(c["weeks"], c["n"])).astype(np.int32)


def _make_env(c):
    if c["variant"] == 2:
        return _env2(c["n"], levels=c["L"], initial_inventory=INVENTORY[:c["L"]], shipment_delays=c["delays"],
                     weeks=c["weeks"])
    from gym_supplychain_amd import BeerGameVecEnv
    info = dict(levels=c["L"], initial_inventory=INVENTORY[:c["L"]], customer_demand=[0] * c["weeks"],
                shipment_delays=c["delays"])
    return BeerGameVecEnv(c["n"], info, demand=torch.as_tensor(_demand1(c), device=DEV), seed=SEED, device=DEV,
                          track_history=True)


def _make_oracles(c, episodes):
    L, n = c["L"], c["n"]
    if c["variant"] == 2:
        from oracle.gen_golden_bg2 import STREAM_BG2_DELAY, STREAM_BG2_DEMAND, uniform_table
        demand = [uniform_table(SEED, n, ep, c["weeks"], 0, 16, STREAM_BG2_DEMAND) for ep in range(episodes)]
        if isinstance(c["delays"], tuple):
            table = [uniform_table(SEED, n, ep, c["weeks"], *c["delays"], STREAM_BG2_DELAY) for ep in range(episodes)]
            delays = lambda i, ep: table[ep][i].tolist()  # noqa: E731
        else:
            delays = lambda i, ep: list(c["delays"])  # noqa: E731
        return MlpOracles(lambda i, ep: BeerGame2Oracle(weeks=c["weeks"], levels=L, initial_inventory=INVENTORY[:L],
                                                        customer_demand=demand[ep][i], shipment_delays=delays(i, ep)),
                          n, max_stock=100)
    demand = _demand1(c)
    return MlpOracles(lambda i, ep: BeerGameOracle(dict(levels=L, initial_inventory=INVENTORY[:L],
                                                        customer_demand=demand[:, i], shipment_delays=c["delays"])), n)


def _clip(c):
    return c["clip"] or (0, 30)   # BeerGame2VecEnv's default: (0, max_order)


# ---- the expected side: one oracle per env, no GPU -------------------------------------------------------
class MlpOracles(Oracles):
    """The lock-step oracles of test_gpu_bg_local_policy.py with the MLP's actions, and what the
    cases must exercise."""

    def __init__(self, make, n, max_stock=0):
        super().__init__(make, n, max_stock)
        self.mlp_seen = dict(lo=False, hi=False, inside=False, dead=False, live=False, transit=False, upstream=False,
                             tie=0, order=0)

    def act_mlp(self, net, lo, hi, std=None, eps=None):
        """(features int32 [n, L, 4], u float32 [n, L], actions int32 [n, L]) for the oracles' states."""
        w1, b1, w2, b2 = net
        f = self.features()
        x = bg_mlp_ref.inputs(f)
        hid = bg_mlp_ref.hidden(w1, b1, x)
        z = bg_mlp_ref.z_values(w1, b1, w2, b2, x)
        u = z if eps is None else bg_mlp_ref.sample(z, std, eps)
        a = bg_mlp_ref.finish(u, lo, hi)
        parts = np.stack([bg_local_ref.line_parts(o) for o in self.o])   # [n, 3, L]
        interior = (u > lo) & (u < hi)
        s = self.mlp_seen
        for k, v in dict(lo=(a == lo).any(), hi=(a == hi).any(), inside=((a > lo) & (a < hi)).any(), dead=(hid == 0).any(),
                         live=(hid > 0).any(), upstream=(parts[:, 1] != 0).any(), transit=(parts[:, 2] != 0).any()).items():
            s[k] = s[k] or bool(v)
        s["tie"] += int((interior & (u - np.floor(u) == 0.5)).sum())
        s["order"] += int((z.view(np.uint32) != bg_mlp_ref.one_expression(w1, b1, w2, b2, x).view(np.uint32)).sum())
        return f.astype(np.int32), u, a

    def assert_mlp_exercised(self, L, recipe):
        s = self.mlp_seen
        want = {k for k in s if k not in ("tie", "order") and not (k == "upstream" and L == 1)}
        assert all(s[k] for k in want), f"the case must exercise every one of {sorted(want)}: {s}"
        assert s["tie" if recipe == "tie" else "order"] > 0, s


@functools.lru_cache(maxsize=None)
def _plan(name):
    """The case's expected streams over its K weeks from reset, computed once and left unchanged."""
    c = CASES[name]
    K, n, L = c["K"], c["n"], c["L"]
    *net, std, noise = _network(c)
    lo, hi = _clip(c)
    orc = _make_oracles(c, K // c["weeks"] + 2)
    reset_obs = orc.reset()
    feats, us, acts, obs, rew = [], [], [], [], []
    for k in range(K):
        f, u, a = orc.act_mlp(net, lo, hi, std, noise[k]) if c["sampled"] else orc.act_mlp(net, lo, hi)
        o, r = orc.step(a)
        feats.append(f), us.append(u), acts.append(a), obs.append(o), rew.append(r)
    orc.assert_mlp_exercised(L, c["recipe"])
    return dict(case=c, net=net, std=std, noise=noise, clip=(lo, hi), reset_obs=reset_obs, oracles=orc,
                features=np.stack(feats), samples=np.stack(us), actions=np.stack(acts), obs=np.stack(obs),
                rewards=np.stack(rew), final_features=orc.features())


@functools.lru_cache(maxsize=None)
def _twin(name):
    """An env stepped with step() on the plan's actions: its observations and rewards are the
    oracles', and before week k its policy_features() are features[k]."""
    p = _plan(name)
    twin = _make_env(p["case"])
    assert np.array_equal(twin.reset().cpu().numpy(), p["reset_obs"])
    for k in range(p["case"]["K"]):
        assert np.array_equal(twin.policy_features().cpu().numpy(), p["features"][k]), k
        o, r, _, _ = twin.step(torch.as_tensor(p["actions"][k], device=DEV))
        assert np.array_equal(o.cpu().numpy(), p["obs"][k]) and np.array_equal(r.cpu().numpy(), p["rewards"][k]), k
    assert np.array_equal(twin.policy_features().cpu().numpy(), p["final_features"])
    twin.check_errors()
    return twin


def _packed(env, p):
    return env.pack_local_mlp(*(torch.as_tensor(x) for x in p["net"]))


def _run(env, p, k0=0, k1=None, samples_out="new", **kw):
    """Weeks k0..k1 of the plan on env; samples_out "new", "alias" (the noise tensor itself) or None."""
    c = p["case"]
    k1 = c["K"] if k1 is None else k1
    if c["sampled"]:
        noise = torch.as_tensor(p["noise"][k0:k1], device=DEV).contiguous()
        kw.update(noise=noise, std=torch.as_tensor(p["std"]),
                  samples_out={"new": torch.empty_like(noise), "alias": noise, None: None}[samples_out])
    return env.rollout_policy(_packed(env, p), None, k1 - k0, clip=c["clip"], return_actions=True, return_obs=True,
                              return_rewards=True, return_features=True, **kw)


def _assert_result(res, p, k0=0, k1=None, samples=True):
    sl = slice(k0, k1)
    assert res.actions.dtype == torch.int32 and np.array_equal(res.actions.cpu().numpy(), p["actions"][sl])
    assert res.features.dtype == torch.int32 and np.array_equal(res.features.cpu().numpy(), p["features"][sl])
    assert np.array_equal(res.obs.cpu().numpy(), p["obs"][sl])
    assert np.array_equal(res.rewards.cpu().numpy(), p["rewards"][sl])
    assert res.reward_sum.dtype == torch.int64
    assert np.array_equal(res.reward_sum.cpu().numpy(), p["rewards"][sl].sum(0))
    if p["case"]["sampled"] and samples:
        assert res.samples.dtype == torch.float32
        assert np.array_equal(res.samples.cpu().numpy().view(np.uint32), p["samples"][sl].view(np.uint32))
    else:
        assert res.samples is None


def _counters(c):
    return c["K"] % c["weeks"], c["K"] // c["weeks"]


# ---- 1. every case against the oracle-driven twin ---------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_oracle_driven_twin(name):
    p, twin = _plan(name), _twin(name)
    c = p["case"]
    env = _make_env(c)
    in_lds = env.ring_slots * c["L"] * 256 * 4 <= 64 * 1024
    assert in_lds == (c["delays"] is not HBM_DELAYS)
    env.reset()
    res = _run(env, p)
    _assert_result(res, p)
    _assert_same_state(env, twin)
    assert (env.week, env.episode) == _counters(c)
    env.check_errors()


def test_the_cases_cover_the_grid():
    cs = list(CASES.values())
    assert {c["variant"] for c in cs} == {1, 2} and {c["L"] for c in cs} >= {1, 4, 8}
    assert {c["H"] for c in cs} == {1, 16, 33, 64} and all(c["L"] in (3, 4) for c in cs if c["H"] == 33)
    for variant in (1, 2):
        mine = [c for c in cs if c["variant"] == variant]
        assert {c["sampled"] for c in mine} == {True, False} and {c["recipe"] for c in mine} == {"gauss", "tie"}
        assert any(c["delays"] is HBM_DELAYS for c in mine) and any(c["delays"] is LIST_DELAYS for c in mine)
    assert any(c["delays"] is STOCHASTIC and c["K"] > T for c in cs)      # stochastic delays, auto-reset inside the call
    assert any(c["K"] > 128 for c in cs)                                   # across the launch cut


# ---- 2. samples_out aliasing noise, and no samples_out ----------------------------------------------------
@pytest.mark.parametrize("name", ["v2-L4-H33-tie-sampled-list", "v1-L4-H16-gauss-sampled-list", "v2-L8-H16-tie-sampled-hbm"])
def test_samples_out_may_be_the_noise_tensor(name):
    p, twin = _plan(name), _twin(name)
    env = _make_env(p["case"])
    env.reset()
    res = _run(env, p, samples_out="alias")
    _assert_result(res, p)
    _assert_same_state(env, twin)
    env = _make_env(p["case"])   # (a fresh env: reset() would go on with the next episode's draws)
    env.reset()
    none = _run(env, p, samples_out=None)
    _assert_result(none, p, samples=False)
    _assert_same_state(env, twin)


# ---- 3. an episode cut into two calls ---------------------------------------------------------------------
@pytest.mark.parametrize("name,cut", [("v2-L4-H16-gauss-sampled-stochastic", 7), ("v1-L4-H16-gauss-sampled-list", 5),
                                      ("v2-L4-H16-gauss-det-list", 13)])
def test_two_calls_equal_one(name, cut):
    """The second call starts mid-episode (or just after an auto-reset): its in-transit sums and
    last demand come from the state alone."""
    p, twin = _plan(name), _twin(name)
    env = _make_env(p["case"])
    env.reset()
    _assert_result(_run(env, p, 0, cut), p, 0, cut)
    assert (env.week, env.episode) == (cut % T, cut // T)
    _assert_result(_run(env, p, cut, None), p, cut, None)
    _assert_same_state(env, twin)


# ---- 4. afterwards the env goes on as the oracles do ------------------------------------------------------
@pytest.mark.parametrize("name", ["v2-L4-H16-gauss-sampled-stochastic", "v1-L4-H16-gauss-sampled-list"])
def test_step_and_the_integer_policy_go_on_from_there(name):
    p = _plan(name)
    c = p["case"]
    n, L = c["n"], c["L"]
    env = _make_env(c)
    env.reset()
    _run(env, p)
    orc = _make_oracles(c, c["K"] // c["weeks"] + 3)
    orc.reset()
    for k in range(c["K"]):
        orc.step(p["actions"][k])
    lo, hi = p["clip"]
    acts = np.random.RandomState(3).randint(max(lo, 0), hi + 1, size=(2, n, L)).astype(np.int32)
    for a in acts:
        o, r, _, _ = env.step(torch.as_tensor(a, device=DEV))
        wo, wr = orc.step(a)
        assert np.array_equal(o.cpu().numpy(), wo) and np.array_equal(r.cpu().numpy(), wr)
    assert np.array_equal(env.policy_features().cpu().numpy(), orc.features())
    rs = np.random.RandomState(29)
    W, b = rs.randint(-64, 65, size=(n, L, 4)).astype(np.int32), rs.randint(-2000, 2001, size=(n, L)).astype(np.int32)
    want_a, want_o, want_r = [], [], []
    for _ in range(T):   # across the next episode end
        a = orc.act(W, b, lo, hi)
        o, r = orc.step(a)
        want_a.append(a), want_o.append(o), want_r.append(r)
    res = env.rollout_policy(env.pack_local_policy(W, b), None, T, shift=SHIFT, clip=(lo, hi), return_actions=True,
                             return_obs=True, return_rewards=True)
    assert np.array_equal(res.actions.cpu().numpy(), np.stack(want_a))
    assert np.array_equal(res.obs.cpu().numpy(), np.stack(want_o))
    assert np.array_equal(res.rewards.cpu().numpy(), np.stack(want_r))
    assert res.samples is None and res.features is None
    env.check_errors()


# ---- 5. outputs are optional ------------------------------------------------------------------------------
def test_reward_sum_alone_and_no_weeks():
    name = "v2-L4-H16-gauss-sampled-stochastic"
    p, twin = _plan(name), _twin(name)
    c = p["case"]
    env = _make_env(c)
    env.reset()
    noise = torch.as_tensor(p["noise"], device=DEV)
    res = env.rollout_policy(_packed(env, p), None, c["K"], noise=noise, std=torch.as_tensor(p["std"]))
    assert res.actions is None and res.obs is None and res.rewards is None and res.samples is None and res.features is None
    assert np.array_equal(res.reward_sum.cpu().numpy(), p["rewards"].sum(0))
    assert torch.equal(noise.cpu(), torch.as_tensor(p["noise"]))     # the noise is only read
    _assert_same_state(env, twin)
    none = env.rollout_policy(_packed(env, p), None, 0, noise=noise[:0], std=0.5, samples_out=noise[:0],
                              return_features=True)
    assert not none.reward_sum.any() and (env.week, env.episode) == _counters(c)
    assert tuple(none.features.shape) == (0, c["n"], c["L"], 4) and tuple(none.samples.shape) == (0, c["n"], c["L"])


# ---- 6. argument errors -----------------------------------------------------------------------------------
def _small(variant, n=16, **kw):
    c = _case(variant, 4, 3, "tie", True, n=n, **kw)
    w1, b1, w2, b2, _, _ = _network(c)
    return c, [torch.as_tensor(x) for x in (w1, b1, w2, b2)]


def _assert_refused_then_steps_on(make, call):
    """`call(env)` raises ValueError and leaves the env as its untouched twin."""
    env, twin = make(), make()
    env.reset()
    twin.reset()
    a = torch.ones((env.n_envs, env.levels), dtype=torch.int32, device=DEV)
    env.step(a)
    twin.step(a)
    with pytest.raises(ValueError):
        call(env)
    assert (env.week, env.episode) == (twin.week, twin.episode) == (1, 0)
    o, r, _, _ = env.step(a)
    to, tr, _, _ = twin.step(a)
    assert torch.equal(o, to) and torch.equal(r, tr)
    _assert_same_state(env, twin)


@pytest.mark.parametrize("variant", [1, 2])
def test_python_argument_errors(variant):
    c, net = _small(variant)
    n, L, K = c["n"], c["L"], 2
    make = functools.partial(_make_env, c)
    clip = (0, 30)
    noise = lambda *shape: torch.zeros(shape or (K, n, L), dtype=torch.float32, device=DEV)  # noqa: E731
    w1, b1, w2, b2 = net
    bad_packs = [
        lambda e: e.pack_local_mlp(w1[:, :-1], b1, w2, b2),                  # w1 not [H, 4L]
        lambda e: e.pack_local_mlp(w1, b1[:-1], w2, b2),
        lambda e: e.pack_local_mlp(w1, b1, w2.t(), b2),
        lambda e: e.pack_local_mlp(w1, b1, w2, b2[:-1]),
        lambda e: e.pack_local_mlp(w1.expand(n, *w1.shape), b1, w2, b2),     # per-env weights
        lambda e: e.pack_local_mlp(w1.expand(n, *w1.shape), b1.expand(n, -1), w2.expand(n, *w2.shape), b2.expand(n, -1)),
        lambda e: e.pack_local_mlp(torch.zeros(65, 4 * L), torch.zeros(65), torch.zeros(L, 65), b2),   # H = 65
        lambda e: e.pack_local_mlp(torch.zeros(0, 4 * L), torch.zeros(0), torch.zeros(L, 0), b2),      # H = 0
        lambda e: e.pack_local_mlp(w1.double() + 1e-12, b1, w2, b2),         # not exactly float32
    ]
    run = lambda e, **kw: e.rollout_policy(e.pack_local_mlp(*net), None, K, **{"clip": clip, **kw})  # noqa: E731
    bad_calls = [
        lambda e: run(e, noise=noise()),                                      # noise without std
        lambda e: run(e, std=0.5),                                            # std without noise
        lambda e: run(e, samples_out=noise()),                                # samples_out without noise
        lambda e: run(e, noise=noise(K, n, L + 1), std=0.5),                  # wrong shapes
        lambda e: run(e, noise=noise(K + 1, n, L), std=0.5),
        lambda e: run(e, noise=noise(), std=0.5, samples_out=noise(K, n + 1, L)),
        lambda e: run(e, noise=noise(), std=torch.ones(L + 1)),
        lambda e: run(e, noise=noise().double(), std=0.5),
        lambda e: run(e, noise=noise().cpu(), std=0.5),
        lambda e: run(e, noise=noise(), std=-1.0),
        lambda e: run(e, noise=noise(), std=float("nan")),
        lambda e: run(e, shift=1),                                            # shift != 0
        lambda e: run(e, clip=(5, 4)),
        lambda e: run(e, clip=(0, 2 ** 24 + 1)),
        lambda e: run(e, clip=(-2 ** 24 - 1, 0)),
        lambda e: e.rollout_policy(e.pack_local_mlp(*net), torch.zeros(L), K, clip=clip),   # a packed policy carries its bias
        lambda e: e.rollout_policy(_make_env(_small(variant, n=n + 1)[0]).pack_local_mlp(*net), None, K, clip=clip),
    ]
    W4, b4 = np.array([[-1, -1, 0, 0]] * L, dtype=np.int32), np.full(L, 40, dtype=np.int32)
    integer = [lambda e: e.pack_local_policy(W4, b4), lambda e: e.pack_policy(np.zeros((L, L), dtype=np.int32), b4)]
    for pack in integer:   # the new keyword arguments with an integer policy
        bad_calls += [lambda e, pack=pack: e.rollout_policy(pack(e), None, K, clip=clip, noise=noise(), std=0.5),
                      lambda e, pack=pack: e.rollout_policy(pack(e), None, K, clip=clip, std=0.5),
                      lambda e, pack=pack: e.rollout_policy(pack(e), None, K, clip=clip, samples_out=noise()),
                      lambda e, pack=pack: e.rollout_policy(pack(e), None, K, clip=clip, return_features=True)]
    for call in bad_packs + bad_calls:
        _assert_refused_then_steps_on(make, call)
    # clip=None: (0, max_order) on BeerGame2VecEnv; refused on BeerGameVecEnv, whose default is the int32 range
    if variant == 1:
        _assert_refused_then_steps_on(make, lambda e: run(e, clip=None))
    else:
        env = make()
        env.reset()
        res = run(env, clip=None, return_actions=True)
        assert 0 <= int(res.actions.min()) and int(res.actions.max()) <= env.max_order == 30


@pytest.mark.parametrize("what", ["delay-65", "full_table", "9-levels"])
def test_config_refusals_leave_the_env_stepping_on(what):
    from gym_supplychain_amd import BeerGameVecEnv
    n = 16
    _, net = _small(1)
    call = lambda e: e.rollout_policy(e.pack_local_mlp(*net), None, 2, clip=(0, 30))  # noqa: E731
    base = dict(levels=4, initial_inventory=INVENTORY[:4], customer_demand=[4] * T, shipment_delays=LIST_DELAYS)
    if what == "delay-65":
        delays = list(LIST_DELAYS)
        delays[2] = 65
        make = functools.partial(BeerGameVecEnv, n, dict(base, shipment_delays=delays), demand="fixed", device=DEV)
    elif what == "full_table":
        make = functools.partial(BeerGameVecEnv, n, base, demand="fixed", device=DEV, full_table=True)
    else:
        make = functools.partial(BeerGameVecEnv, n, dict(levels=9, initial_inventory=[12] * 9), device=DEV)
        call = lambda e: e.pack_local_mlp(torch.zeros(3, 36), torch.zeros(3), torch.zeros(9, 3), torch.zeros(9))  # noqa: E731
    _assert_refused_then_steps_on(make, call)
