"""The SupplyChain closed loop on the host, in NumPy and on the oracle: the one statement of the
float32 policy formulas (include/scgpu.h scg_sc_rollout_policy / _mlp / _sampled,
csrc/scg_sc_policy.h) that the device tests compare against, and a rollout of one env that
uses them.

Every product and every sum is rounded to float32 on its own, terms in ascending index:

    z[a] = b[a];  for j in range(len(x)): z[a] = z[a] + w[a][j] * x[j]
    hidden: h[i] = z1[i] if z1[i] > 0 else +0.0
    sampled: u[a] = z[a] + (std[a] * eps[a])
    action[a] = lo if not v[a] >= lo else min(v[a], hi)        (v = z, or u when sampled)

rollout() runs K steps of one env on oracle/supplychain.py with the device's own draws
(tests/sc_fuzz.py oracle_for), open loop (actions given) or closed (a policy's parameters
given), with the auto-reset the device does: at a terminal step the row's observation is the
next episode's reset observation and the terminal one is kept apart.
"""
from types import SimpleNamespace

import numpy as np

LO, HI = np.float32(-1.0), np.float32(1.0)


def layer(x, w, b):
    """z [N, R] = b, then + w[:, :, j] * x[:, j] in ascending j, each product and sum rounded to float32.
    x float32 [N, J]; w [N, R, J] or [R, J] (shared), b [N, R] or [R]."""
    n = x.shape[0]
    w = np.broadcast_to(w, (n,) + w.shape[-2:])
    z = np.broadcast_to(b, (n, w.shape[1])).astype(np.float32).copy()
    with np.errstate(all="ignore"):
        for j in range(x.shape[1]):
            z = (z + (w[:, :, j] * x[:, None, j]).astype(np.float32)).astype(np.float32)
    return z


def clamp(v, lo=LO, hi=HI):
    """lo where not v >= lo (a NaN too), hi where v > hi, else v."""
    return np.where(~(v >= lo), lo, np.where(v > hi, hi, v)).astype(np.float32)


def relu(pre):
    return np.where(pre > 0, pre, np.float32(0.0)).astype(np.float32)


def policy_z(obs, params):
    """(hidden or None, z): the policy's value before its clamp of obs [N, O] (any float type; it
    goes to float32 first). params: linear (w, b) or one-hidden-layer ReLU (w1, b1, w2, b2)."""
    x = obs.astype(np.float32)
    if len(params) == 2:
        return None, layer(x, *params)
    w1, b1, w2, b2 = params
    hid = relu(layer(x, w1, b1))
    return hid, layer(hid, w2, b2)


def sample(z, std, eps, lo=LO, hi=HI):
    """(u, action) of the sampled formula: the product rounded to float32, then the sum, then the clamp."""
    with np.errstate(all="ignore"):
        u = (z + (std[None, :] * eps).astype(np.float32)).astype(np.float32)
    return u, clamp(u, lo, hi)


def env_params(params, n):
    """Env n's own parameters of a per-env set (leading axis N), a shared set as it is."""
    shared = params[0].ndim == 2
    return tuple(p if shared else p[n] for p in params)


def rollout(nodes, env_kw, draw_seed, env_id, n_leadtimes, k, actions=None, params=None, eps=None, std=None,
            lo=LO, hi=HI):
    """K steps of env `env_id` from its first reset. Open loop: actions float32 [K, A]. Closed
    loop: params of this env, (w [A, O], b [A]) or (w1 [H, O], b1 [H], w2 [A, H], b2 [A]); with
    eps float32 [K, A] and std float32 [A] the actions are sampled.

    Returns a namespace: obs0 (the reset observation), actions [K, A] float32, samples [K, A]
    float32 (None unless sampled), hidden [K, H] float32 (None unless an MLP), obs [K, O]
    float64 (a terminal step's row is the next episode's reset observation), rewards [K]
    float64, dones [K] bool, term_obs {step index: the terminal observation}, reward_sum (the
    rewards added in step order in float64), stocks [node][product] and heaps
    [node][product] -> [(time, amount)] in storage order after the last step, time_step and
    episode."""
    from sc_fuzz import oracle_for
    T = env_kw["total_time_steps"]
    episode = 0
    o, obs = oracle_for(nodes, env_kw, draw_seed, env_id, episode, n_leadtimes)
    out = SimpleNamespace(obs0=obs, actions=[], samples=[], hidden=[], obs=[], rewards=[], dones=[], term_obs={},
                          reward_sum=np.float64(0.0))
    for j in range(k):
        if actions is not None:
            act = np.asarray(actions[j], dtype=np.float32)
        else:
            hid, z = policy_z(obs[None], params)
            if hid is not None:
                out.hidden.append(hid[0])
            if eps is not None:
                u, act = sample(z, std, eps[j][None], lo, hi)
                out.samples.append(u[0])
            else:
                act = clamp(z, lo, hi)
            act = act[0]
        out.actions.append(act)
        obs, reward, done, _ = o.step(act.copy())
        assert done == (o.t == T)
        out.rewards.append(np.float64(reward))
        out.reward_sum = out.reward_sum + np.float64(reward)
        out.dones.append(bool(done))
        if done:
            out.term_obs[j] = obs
            episode += 1
            o, obs = oracle_for(nodes, env_kw, draw_seed, env_id, episode, n_leadtimes)
        out.obs.append(obs)
    out.actions = np.stack(out.actions)
    out.samples = np.stack(out.samples) if out.samples else None
    out.hidden = np.stack(out.hidden) if out.hidden else None
    out.obs = np.stack(out.obs).astype(np.float64)
    out.rewards = np.asarray(out.rewards, dtype=np.float64)
    out.dones = np.asarray(out.dones)
    out.stocks = [[float(s) for s in nd.stock] for nd in o.nodes]
    out.heaps = [[[(int(t), float(v)) for t, v in h] for h in node] for node in o.heaps()]
    out.time_step, out.episode = o.t, episode
    return out
