"""The chains of the fused-rollout fuzz (tests/test_gpu_sc_rollout_fuzz.py on the device,
tests/test_sc_rollout_fuzz_inputs.py on the host): seeds of tests/sc_fuzz.py random_chain(seed,
T=6) with the shape scg_sc_prepare derives for each, written down so that a change to the chain
generator or to the admission rules fails a host test instead of emptying the device tests.

The node-parallel block's size, LDS layout, loop trip counts and row ownership all follow the
chain's shape; `why` says what each chain reaches that sc-2perstage-v0 (8 nodes, 8 waves, P = 1,
A = 14, O = 27), its two-product variant and the [1, 1, 1, w] chains do not.

Sizes of every case: 130 envs (two full 64-env tiles and a 2-env tail), 6-step episodes, 15
steps per call (two auto-resets, ending mid-episode), envs 0, 63, 64 and 129 against the oracle.
"""
from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

T, K, N_ENVS = 6, 15, 130
SAMPLE = (0, 63, 64, 129)

# kernel: what kernel="auto" of the device tests' env is expected to be ("nodes": the env is built
# with kernel="nodes"; "staged": with kernel="auto", kernel="nodes" refusing the chain for LDS).
# waves / inbox: `group` and `inbox_size` under kernel="nodes" (inbox of a staged case: under "auto").
# bucket: the destination-list instantiation (max_dests rounded up to 2, 4, 8).
# f64: whether kernel="nodes" admits float64 observations (float32 it admits on every "nodes" case).
Case = namedtuple("Case", "seed nodes waves P A O heap_cap inbox bucket stochastic avg_lt max_lt kernel f64 why")
CASES = [
    Case(13, 5, 5, 1, 7, 12, 8, 5, 2, True, 1, 3, "nodes", True, "fewest waves; Poisson lead times 1..3"),
    Case(45, 5, 5, 2, 10, 25, 2, 8, 2, False, 1, 1, "nodes", True, "heaps of two slots"),
    Case(2, 6, 6, 2, 12, 55, 4, 10, 4, False, 3, 3, "nodes", True, "destination bucket 4; O in two chunks"),
    Case(36, 7, 7, 3, 30, 49, 4, 24, 2, False, 1, 1, "nodes", True,
         "three products; A > 4 W (the stage's tail loop); float64 block of 161,280 B"),
    Case(47, 7, 7, 3, 27, 49, 4, 21, 2, False, 1, 1, "nodes", True, "three products; A = 4 W - 1 (no stage tail)"),
    Case(48, 7, 7, 2, 22, 61, 8, 20, 2, False, 3, 3, "nodes", False,
         "float32 block of 155,648 B; float64 observations are refused by design"),
    Case(30, 6, 6, 2, 16, 41, 8, 14, 2, True, 2, 3, "nodes", True, "Poisson lead times; two products; A > 2 W"),
    Case(23, 8, 8, 1, 12, 26, 9, 9, 2, True, 2, 2, "nodes", True, "stochastic with avg = max lead time"),
    Case(6, 10, 8, 1, 24, 32, 12, 21, 4, True, 2, 3, "nodes", True,
         "waves own two nodes; Poisson; O = 32 exactly; A > 2 W; float64 block of 159,744 B"),
    Case(10, 10, 8, 1, 24, 22, 9, 21, 4, True, 1, 2, "nodes", True, "waves own two nodes; Poisson with avg 1"),
    Case(38, 11, 8, 1, 27, 25, 6, 24, 4, False, 1, 1, "nodes", True, "H = 64 fits the hidden tile"),
    Case(57, 10, 8, 1, 19, 42, 12, 16, 4, False, 3, 3, "nodes", True,
         "a 4-destination node on a wave that owns two nodes"),
    Case(4, 9, 0, 3, 42, 91, 9, 33, 4, False, 2, 2, "staged", False, "refused for LDS: the per-step action kernels"),
    Case(33, 11, 0, 3, 57, 142, 15, 51, 4, True, 3, 4, "staged", False,
         "refused for LDS; O in five chunks; Poisson lead times"),
]
BY_SEED = {c.seed: c for c in CASES}
NODES_CASES = [c for c in CASES if c.kernel == "nodes"]
STAGED_CASES = [c for c in CASES if c.kernel == "staged"]
LDS_MESSAGE = "exceed the node-parallel kernel's LDS"


def hidden_bound(case):
    """The fused kernel's hidden tile: H <= 2 (E + NN) (csrc/scg_sc_mlp.h)."""
    return 2 * (case.inbox + case.nodes)


def dtypes(case, cfg=None):
    """Observation dtypes the device tests run a case with: float64 wherever it is admitted; float32
    on the chain that refuses float64 (every loop), and on the two blocks at the edge of LDS and the
    smallest chain for the open loop and one closed loop each, the sampled one with the most in it (the
    policy reads float32(observation) either way, so the reference is the same; what float32 changes
    is the block's LDS layout, which seed 48 runs under all four closed loops)."""
    if case.kernel != "nodes":
        return ["f64"]
    f32 = case.seed == 48 or (case.seed in (36, 6, 13) and (cfg is None or cfg == closed_configs(case)[-1]))
    return (["f64"] if case.f64 else []) + (["f32"] if f32 else [])


# The closed loops the device tests run per chain, and the host test checks the inputs of:
# (policy, hidden width or None, shared, sampled).
def closed_configs(case):
    if case.kernel == "staged":
        return [("linear", None, False, False), ("mlp", 16, False, False), ("mlp", 16, False, True)]
    bound = hidden_bound(case)
    out = [("linear", None, False, False)]
    if case.seed in (13, 36, 6):
        out.append(("linear", None, True, False))
    widths = [min(16, bound)] + ([bound] if bound <= 64 and bound != min(16, bound) else []) + ([64] if case.seed == 38 else [])
    out += [("mlp", h, False, False) for h in widths]
    out.append(("linear", None, False, True))
    if case.A > 2 * case.waves:  # the sampled loop's noise tail, under both policies
        out.append(("mlp", min(16, bound), False, True))
    return out


def config_id(cfg):
    policy, hidden, shared, sampled = cfg
    return "-".join(x for x in (policy + (str(hidden) if hidden else ""), "shared" if shared else "", "sampled" if sampled else "") if x)


def chain(case):
    from sc_fuzz import random_chain
    return random_chain(case.seed, T=T)


def prepare(case, kernel, f64):
    """scg_sc_prepare of the case's chain (host only): (rc, config, error text)."""
    import ctypes

    from gym_supplychain_amd import _native as nat
    from gym_supplychain_amd.envs import SupplyChainSpec
    nodes, env_kw = chain(case)
    spec = SupplyChainSpec(nodes, **env_kw)
    c = nat.ScConfig()
    c.n_nodes, c.n_products, c.n_retailers = len(spec.nodes), spec.P, spec.n_retailers
    c.total_time_steps, c.avg_leadtime, c.max_leadtime = spec.total_time_steps, spec.avg_leadtime, spec.max_leadtime
    c.stochastic_leadtimes = int(spec.stochastic_leadtimes)
    c.demand_lo, c.demand_hi = spec.demand_models[0].lo, spec.demand_models[0].hi
    for k, v in spec.penalties.items():
        setattr(c, k, v)
    if spec.stochastic_leadtimes:
        c.leadtime_poisson_len = len(nat.poisson_table(spec.avg_leadtime - 1))
    c.obs_f64 = int(f64)
    c.kernel = {"nodes": nat.SC_KERNEL_NODES, "auto": nat.SC_KERNEL_AUTO}[kernel]
    rc = nat.lib.scg_sc_prepare(ctypes.byref(c), spec.node_table())
    return rc, c, nat.last_error() if rc else ""


@lru_cache(maxsize=None)
def open_loop_actions(case):
    """float32 actions [K, N, A] in [-1.1, 1.1] (sc_fuzz.random_actions' draw); shared, read only."""
    from sc_fuzz import random_actions
    return random_actions(case.seed, K, N_ENVS, case.A)


@lru_cache(maxsize=None)
def policy_inputs(case, cfg):
    """(params, eps, std) of a closed loop: the existing device tests' generators (their scales:
    weights N(0, 0.35), biases N(0, 0.5), second layer N(0, 1.4 / sqrt(H)); noise N(0, 1), std in
    [0.05, 0.6] with one element exactly 0) at this chain's sizes. eps, std are None unless sampled. Shared, read only."""
    from test_gpu_sc_mlp_rollout import _params as mlp_params
    from test_gpu_sc_policy_rollout import _params as linear_params
    from test_gpu_sc_sampled_rollout import _noise
    policy, hidden, shared, sampled = cfg
    shape = SimpleNamespace(n_envs=N_ENVS, n_actions=case.A, n_obs=case.O)
    params = linear_params(shape, shared=shared) if policy == "linear" else mlp_params(shape, hidden, shared=shared)
    eps, std = _noise(shape, K) if sampled else (None, None)
    return params, eps, std


_REFS = {}


def reference(case, cfg=None):
    """{env: sc_closed_ref.rollout of that env} for the sampled envs: the open loop of
    open_loop_actions (cfg None) or the closed loop cfg of policy_inputs. Computed once per
    (chain, cfg) and shared by the tests; read only."""
    import sc_closed_ref as ref
    key = (case.seed, cfg)
    if key not in _REFS:
        nodes, env_kw = chain(case)
        from gym_supplychain_amd.envs import SupplyChainSpec
        n_lt = SupplyChainSpec(nodes, **env_kw).n_leadtimes
        out = {}
        if cfg is None:
            acts = open_loop_actions(case)
            for n in SAMPLE:
                out[n] = ref.rollout(nodes, env_kw, 99 + case.seed, n, n_lt, K, actions=acts[:, n])
        else:
            params, eps, std = policy_inputs(case, cfg)
            for n in SAMPLE:
                out[n] = ref.rollout(nodes, env_kw, 99 + case.seed, n, n_lt, K, params=ref.env_params(params, n),
                                     eps=None if eps is None else eps[:, n], std=std)
        _REFS[key] = out
    return _REFS[key]


def bits(x):
    a = np.ascontiguousarray(x)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
