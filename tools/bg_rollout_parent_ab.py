"""The BeerGame rollouts of this tree against a build of another commit (the parent), alternating
processes.

    python tools/bg_rollout_parent_ab.py --parent-root DIR [--rounds 5] [--envs 65536] [--episodes 4000]

DIR holds the other build's package (DIR/gym_supplychain_amd with its libscgpu.so), as
SCG_PKG_ROOT names it for the other tools. Each round starts one fresh process on the other
build and one on this tree (never two at a time); a process makes its envs (L = 4, 35 weeks,
auto-reset), runs one untimed sample of each path and then three alternating samples of each, a
sample being the wall clock of `--episodes` calls of 35 weeks between two device synchronisations:
  rollout1         BeerGameVecEnv.rollout, Poisson demand, a delay list;
  rollout2         BeerGame2VecEnv.rollout, demand (0, 16), delays (0, 5);
  rollout_policy1  rollout_policy on the first env, no output but reward_sum;
  rollout_policy2  rollout_policy on the second;
  rollout_local1, rollout_local2            the same with a pack_local_policy() policy;
  rollout_mlp_det2, rollout_mlp_sampled2    the second env with a pack_local_mlp() policy of H = 16,
                   deterministic, and sampled with noise= and samples_out= preallocated.
The policy draw is that of tools/bg_policy_rollout_ab.py: per-env weights in [-64, 64], biases in
[-2000, 2000], shift 4; BeerGameVecEnv's order increments are clamped to (-3, 7). The MLP draw is
that of tools/bg_mlp_rollout_ab.py. A process
reports the median of its three samples per path, in microseconds per week of the batch. The
summary gives, per path and build, the median, minimum and maximum of the rounds' figures, and
whether this tree's median lies inside the other build's minimum .. maximum, else by how much
it lies outside.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ("rollout1", "rollout2", "rollout_policy1", "rollout_policy2", "rollout_local1", "rollout_local2",
         "rollout_mlp_det2", "rollout_mlp_sampled2")
LEVELS, WEEKS, SEED, SHIFT, HIDDEN = 4, 35, 0x5EED0000, 4, 16
CHILD_TIMEOUT = 900  # the four first paths fit 300 s; an MLP week costs about three linear ones
DELAYS = [2, 0, 3, 1, 1, 4, 2] * 5
CLIP1 = (-3, 7)  # BeerGameEnv's actions are increments over the incoming order


def child(a):
    sys.path.insert(0, os.environ.get("SCG_PKG_ROOT") or os.path.join(REPO, "gym-supplychain_amd"))
    import torch

    from gym_supplychain_amd import BeerGame2VecEnv, BeerGameVecEnv
    dev = torch.device("cuda", 0)
    N, L, T = a.envs, LEVELS, WEEKS
    info = dict(levels=L, customer_demand=[0] * T, shipment_delays=DELAYS)
    envs = {}
    for k in PATHS:
        if k.endswith("1"):
            envs[k] = BeerGameVecEnv(N, info, demand="poisson", poisson_lambda=6.0, seed=SEED, device=dev)
        else:
            envs[k] = BeerGame2VecEnv(N, weeks=T, levels=L, customer_demand=(0, 16), shipment_delays=(0, 5), seed=SEED,
                                      device=dev)
        envs[k].reset()
    gen = torch.Generator(device="cpu").manual_seed(SEED)
    W = torch.randint(-64, 65, (N, L, L), generator=gen, dtype=torch.int32).to(dev)
    b = torch.randint(-2000, 2001, (N, L), generator=gen, dtype=torch.int32).to(dev)
    packed = {"policy": envs["rollout_policy1"].pack_policy(W, b)}
    acts = {"rollout1": torch.randint(-3, 8, (T, N, L), generator=gen, dtype=torch.int32).to(dev),
            "rollout2": torch.randint(0, 16, (T, N, L), generator=gen, dtype=torch.int32).to(dev)}
    obs = torch.empty((T, N, L), dtype=torch.int32, device=dev)
    rew = torch.empty((T, N), dtype=torch.int32, device=dev)
    W4 = torch.randint(-64, 65, (N, L, 4), generator=gen, dtype=torch.int32).to(dev)
    packed["local"] = envs["rollout_local1"].pack_local_policy(W4, b)
    gen = torch.Generator(device="cpu").manual_seed(SEED)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float32)  # noqa: E731
    H = HIDDEN
    w1, b1, w2, b2 = rnd(H, 4 * L) / 40, rnd(H), 2 * rnd(L, H) / H ** 0.5, 8 + rnd(L)
    std, noise = (2 * torch.exp(0.3 * rnd(L))).to(dev), rnd(T, N, L).to(dev)
    mlp = envs["rollout_mlp_det2"].pack_local_mlp(*(x.to(dev) for x in (w1, b1, w2, b2)))
    sampled = dict(noise=noise, std=std, samples_out=torch.empty_like(noise))

    def run(name):
        if name in acts:
            envs[name].rollout(acts[name], obs, rew)
        elif "mlp" in name:
            envs[name].rollout_policy(mlp, None, T, **(sampled if "sampled" in name else {}))
        else:
            envs[name].rollout_policy(packed[name[len("rollout_"):-1]], None, T, shift=SHIFT,
                                      clip=CLIP1 if name.endswith("1") else None)

    def sample(name):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(a.episodes):
            run(name)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / (a.episodes * T) * 1e6

    for k in PATHS:
        sample(k)
    got = {k: [] for k in PATHS}
    for _ in range(3):
        for k in PATHS:
            got[k].append(sample(k))
    for env in envs.values():
        env.check_errors()
    print(json.dumps({k: statistics.median(v) for k, v in got.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--episodes", type=int, default=4000)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_root or not os.path.isdir(os.path.join(a.parent_root, "gym_supplychain_amd")):
        raise SystemExit("--parent-root must hold the other build's gym_supplychain_amd package")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--envs", str(a.envs), "--episodes", str(a.episodes)]
    builds = (("parent", os.path.abspath(a.parent_root)), ("this tree", os.path.join(REPO, "gym-supplychain_amd")))
    got = {name: {k: [] for k in PATHS} for name, _ in builds}
    for r in range(a.rounds):
        for name, root in builds:
            p = subprocess.run(cmd, env=dict(os.environ, SCG_PKG_ROOT=root), capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
            if p.returncode != 0:  # a process that failed ends the run: nothing more is started
                raise SystemExit(f"round {r + 1} {name}: exit status {p.returncode}\n{p.stderr[-2000:]}")
            res = json.loads(p.stdout.strip().splitlines()[-1])
            print(f"round {r + 1} {name} {json.dumps(res)}", flush=True)
            for k in PATHS:
                got[name][k].append(res[k])
    for k in PATHS:
        pa, me = got["parent"][k], got["this tree"][k]
        med = statistics.median(me)
        off = med - max(pa) if med > max(pa) else min(pa) - med if med < min(pa) else 0.0
        where = "inside the parent's spread" if off == 0.0 else \
            f"{off:.4f} us {'above' if med > max(pa) else 'below'} the parent's spread"
        print(f"# {k} us/week: parent median {statistics.median(pa):.4f} min {min(pa):.4f} max {max(pa):.4f}; "
              f"this tree median {med:.4f} min {min(me):.4f} max {max(me):.4f}: {where}", flush=True)


if __name__ == "__main__":
    main()
