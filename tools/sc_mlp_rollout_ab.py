"""SupplyChain closed loop with a one-hidden-layer ReLU policy: step() per step with the network
in torch against one rollout_policy() per episode, A/B in one process.

    python tools/sc_mlp_rollout_ab.py [--envs 65536] [--steps 360] [--episodes 8] [--rounds 5] [--hidden 16] [--wide 40]

sc-2perstage-v0 (A = 14, O = 27), float32 observations, auto-reset, the node-parallel kernel,
every env with its own MLP of `--hidden` units (W1 N(0, 0.1), b1 N(0, 0.3), W2 N(0, 0.3), b2
N(0, 0.3), clip (-1, 1)) and, for the shared paths, env 0's. A sample is the wall clock of
`--episodes` episodes of `--steps` steps between two device synchronisations:
  step_loop        (a) the closed loop as it can be written without rollout_policy(): per step
                   the network as torch float32 ops on the device (two baddbmm and a relu), then
                   step(). torch's products add in another order than the formula, so this
                   path's actions differ from the others' in the last bits; it is timed on its
                   own envs;
  mlp_per_env      (b) one rollout_policy() per episode, per-env parameters packed once, no output
                   but reward_sum;
  mlp_shared       (c) the same with one shared MLP;
  linear_per_env   (d) rollout_policy() with a per-env linear policy (DESIGN §6.11's (b));
  rollout          (e) the open-loop rollout() (last observation only) of the actions (b) took;
  mlp_per_env_wide, mlp_shared_wide   (b) and (c) at `--wide` hidden units (40: the fused
                   kernel's hidden tile exactly full on this scenario).
The paths alternate, `--rounds` times, after one untimed sample of each. Before that one episode
is compared bit for bit at the timed size: rollout_policy's actions against the formula written
as sequential torch float32 multiplies and adds (one product and one sum per term, the formula's
order), a step() loop fed those actions against rollout_policy's observations, rewards and
reward_sum, the open-loop replay against both, and the final states; for the wide and shared
MLPs the actions against the formula. Prints one JSON line per sample and a summary line:
medians and max - min of the microseconds per step of the batch.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SCG_PKG_ROOT") or os.path.join(REPO, "gym-supplychain_amd"))
sys.path.insert(0, REPO)

SEED = 0x5EED0000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=360)
    ap.add_argument("--episodes", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=16)
    ap.add_argument("--wide", type=int, default=40)
    a = ap.parse_args()

    import torch

    import gym_supplychain_amd as gsa
    dev = torch.device("cuda", 0)
    N, T = a.envs, a.steps

    def make():
        env = gsa.make_vec("sc-2perstage-v0", N, seed=SEED, device=dev, kernel="nodes", total_time_steps=T,
                           obs_dtype=torch.float32)
        env.reset()
        return env

    names = ("step_loop", "mlp_per_env", "mlp_shared", "linear_per_env", "rollout", "mlp_per_env_wide", "mlp_shared_wide")
    envs = {k: make() for k in names}
    closed = envs["mlp_per_env"]
    A, O = closed.n_actions, closed.n_obs
    gen = torch.Generator(device="cpu").manual_seed(SEED)

    def draw(H):
        return ((torch.randn((N, H, O), generator=gen) * 0.1).to(dev), (torch.randn((N, H), generator=gen) * 0.3).to(dev),
                (torch.randn((N, A, H), generator=gen) * 0.3).to(dev), (torch.randn((N, A), generator=gen) * 0.3).to(dev))

    net, wide = draw(a.hidden), draw(a.wide)
    W, b = (torch.randn((N, A, O), generator=gen) * 0.1).to(dev), (torch.randn((N, A), generator=gen) * 0.3).to(dev)
    if not (closed.mlp_fused(a.hidden) and closed.mlp_fused(a.wide)):
        raise SystemExit("these hidden widths do not run fused on this scenario")
    packed = {"mlp_per_env": closed.pack_mlp(*net), "mlp_shared": closed.pack_mlp(*(p[0] for p in net)),
              "linear_per_env": closed.pack_policy(W, b), "mlp_per_env_wide": closed.pack_mlp(*wide),
              "mlp_shared_wide": closed.pack_mlp(*(p[0] for p in wide))}

    def layer(w, bias, x):  # the formula of include/scgpu.h (scg_sc_mlp), term by term
        z = bias.expand(x.shape[0], -1).clone()
        for j in range(w.shape[-1]):
            z = z + w[..., j] * x[:, j:j + 1]
        return z

    def exact_mlp(p, obs):
        pre = layer(p[0], p[1], obs)
        hid = torch.where(pre > 0, pre, torch.zeros_like(pre))
        z = layer(p[2], p[3], hid)
        return torch.where(~(z >= -1.0), torch.full_like(z, -1.0), torch.where(z > 1.0, torch.full_like(z, 1.0), z))

    w1, b1, w2, b2 = net

    def torch_mlp(obs):  # what a user writes
        hid = torch.baddbmm(b1.unsqueeze(2), w1, obs.unsqueeze(2)).relu_()
        return torch.baddbmm(b2.unsqueeze(2), w2, hid).squeeze(2).clamp_(-1.0, 1.0)

    # one episode of every path, bit for bit, at the timed size
    stepped, replayed = envs["step_loop"], envs["rollout"]
    res = closed.rollout_policy(packed["mlp_per_env"], None, T, return_actions=True, return_obs=True, return_rewards=True)
    obs = stepped._obs
    sums = torch.zeros(N, dtype=torch.float64, device=dev)
    for k in range(T):
        act = exact_mlp(net, obs)
        if not torch.equal(act, res.actions[k]):
            raise SystemExit(f"rollout_policy's actions differ from the formula at step {k + 1}")
        obs, r, _, _ = stepped.step(act)
        sums = sums + r
        if not (torch.equal(obs, res.obs[k]) and torch.equal(r, res.rewards[k])):
            raise SystemExit(f"rollout_policy and the step loop differ at step {k + 1}")
    if not torch.equal(sums, res.reward_sum):
        raise SystemExit("rollout_policy's reward_sum differs from the step loop's rewards")
    acts = res.actions
    last = torch.empty((N, O), dtype=torch.float32, device=dev)
    plan_rew = torch.empty((T, N), dtype=torch.float64, device=dev)
    replayed.rollout(acts, last, plan_rew, last_obs_only=True)
    if not (torch.equal(last, res.obs[-1]) and torch.equal(plan_rew, res.rewards) and torch.equal(last, res.last_obs)):
        raise SystemExit("the open-loop replay of the actions taken differs")
    for t in ("_stock", "_heap_size", "_ret", "_final_ret", "_term_obs"):
        if not (torch.equal(getattr(stepped, t), getattr(closed, t)) and torch.equal(getattr(replayed, t), getattr(closed, t))):
            raise SystemExit(f"the paths differ in {t}")
    del res
    for name, p in (("mlp_shared", tuple(x[:1] for x in net)), ("mlp_per_env_wide", wide),
                    ("mlp_shared_wide", tuple(x[:1] for x in wide))):
        env = envs[name]
        first = env._obs.clone()
        got = env.rollout_policy(packed[name], None, T, return_actions=True, return_obs=True)
        prev = torch.cat([first[None], got.obs[:-1]])
        for k in range(0, T, 7):
            if not torch.equal(exact_mlp(p, prev[k]), got.actions[k]):
                raise SystemExit(f"{name}: rollout_policy's actions differ from the formula at step {k + 1}")
        del got, prev
    envs["linear_per_env"].rollout_policy(packed["linear_per_env"], None, T)
    print(json.dumps({"checked": "one episode of every path, bit for bit", "n_envs": N, "steps": T}), flush=True)

    def step_loop(episodes):
        o = stepped._obs
        for _ in range(episodes * T):
            o = stepped.step(torch_mlp(o))[0]

    def closed_loop(name):
        def run(episodes):
            for _ in range(episodes):
                envs[name].rollout_policy(packed[name], None, T)
        return run

    def rollout(episodes):
        for _ in range(episodes):
            replayed.rollout(acts, last, plan_rew, last_obs_only=True)

    def sample(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn(a.episodes)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / (a.episodes * T) * 1e6  # us per step of the batch

    paths = {k: (step_loop if k == "step_loop" else rollout if k == "rollout" else closed_loop(k)) for k in names}
    for fn in paths.values():
        sample(fn)
    got = {k: [] for k in paths}
    for rnd in range(a.rounds):
        for name, fn in paths.items():
            us = sample(fn)
            got[name].append(us)
            print(json.dumps({"round": rnd, "path": name, "us_per_step": us}), flush=True)
    for env in envs.values():
        env.check_errors()
    med = {k: statistics.median(v) for k, v in got.items()}
    words = {h: h * (O + 1) + A * (h + 1) for h in (a.hidden, a.wide)}
    out = {"n_envs": N, "steps": T, "episodes_per_sample": a.episodes, "rounds": a.rounds, "hidden": a.hidden, "wide": a.wide,
           "param_bytes_per_env": 4 * words[a.hidden], "param_bytes_per_env_wide": 4 * words[a.wide],
           "param_mb_per_step_per_env_mlp": 4e-6 * words[a.hidden] * N}
    for k in paths:
        out[f"{k}_median_us_per_step"] = med[k]
        out[f"{k}_max_minus_min"] = max(got[k]) - min(got[k])
    out["mlp_per_env_minus_rollout_us"] = med["mlp_per_env"] - med["rollout"]
    out["mlp_shared_minus_rollout_us"] = med["mlp_shared"] - med["rollout"]
    out["step_loop_over_mlp_per_env"] = med["step_loop"] / med["mlp_per_env"]
    out["per_env_param_read_gb_per_s"] = 4e-3 * words[a.hidden] * N / med["mlp_per_env"]
    out["per_env_param_read_gb_per_s_wide"] = 4e-3 * words[a.wide] * N / med["mlp_per_env_wide"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
