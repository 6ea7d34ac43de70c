"""The existing SupplyChain rollouts of this tree against a build of another commit (the parent),
alternating processes.

    python tools/sc_closed_parent_ab.py --parent-root DIR [--rounds 5] [--envs 65536] [--steps 360] [--episodes 6]

DIR holds the other build's package (DIR/gym_supplychain_amd with its libscgpu.so), as
SCG_PKG_ROOT names it for the other tools. Each round starts one fresh process on the other
build and one on this tree (never two at a time); a process makes its envs (sc-2perstage-v0,
float32 observations, auto-reset, the node-parallel kernel), runs one untimed episode of each
path and then three alternating samples of each, a sample being the wall clock of `--episodes`
episodes of `--steps` steps between two device synchronisations:
  rollout          rollout(steps) of fixed actions, last observation only;
  linear_per_env   rollout_policy(steps) with a linear policy per env;
  linear_shared    the same with one shared policy;
  mlp_per_env      rollout_policy(steps) with a 16-unit MLP per env;
  linear_sampled   linear_per_env with sampled actions: noise [steps, N, A] drawn once, std 0.1,
                   no samples_out;
  mlp_sampled      mlp_per_env with the same noise and std.
A process reports the median of its three samples per path, in microseconds per step of the
batch. The summary gives, per path and build, the median, minimum and maximum of the rounds'
figures, and whether this tree's median lies inside the other build's minimum .. maximum, else
by how much it lies outside.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ("rollout", "linear_per_env", "linear_shared", "mlp_per_env", "linear_sampled", "mlp_sampled")
SEED = 0x5EED0000


def child(a):
    sys.path.insert(0, os.environ.get("SCG_PKG_ROOT") or os.path.join(REPO, "gym-supplychain_amd"))
    import torch

    import gym_supplychain_amd as gsa
    dev = torch.device("cuda", 0)
    N, T, H = a.envs, a.steps, 16
    envs = {}
    for k in PATHS:
        envs[k] = gsa.make_vec("sc-2perstage-v0", N, seed=SEED, device=dev, kernel="nodes", total_time_steps=T,
                               obs_dtype=torch.float32)
        envs[k].reset()
    e = envs["rollout"]
    A, O = e.n_actions, e.n_obs
    gen = torch.Generator(device="cpu").manual_seed(SEED)

    def rnd(shape, scale):
        return (torch.randn(shape, generator=gen) * scale).to(dev)

    W, b = rnd((N, A, O), 0.1), rnd((N, A), 0.3)
    packed = {"linear_per_env": e.pack_policy(W, b), "linear_shared": e.pack_policy(W[0], b[0]),
              "mlp_per_env": e.pack_mlp(rnd((N, H, O), 0.1), rnd((N, H), 0.3), rnd((N, A, H), 0.3), rnd((N, A), 0.3))}
    packed["linear_sampled"], packed["mlp_sampled"] = packed["linear_per_env"], packed["mlp_per_env"]
    noise = torch.randn((T, N, A), generator=torch.Generator(device=dev).manual_seed(SEED + 1), device=dev)
    acts = torch.rand((T, N, A), generator=torch.Generator(device=dev).manual_seed(SEED), device=dev) * 2 - 1
    last = torch.empty((N, O), dtype=torch.float32, device=dev)
    rew = torch.empty((T, N), dtype=torch.float64, device=dev)

    def run(name):
        if name == "rollout":
            envs[name].rollout(acts, last, rew, last_obs_only=True)
        elif name.endswith("_sampled"):
            envs[name].rollout_policy(packed[name], None, T, noise=noise, std=0.1)
        else:
            envs[name].rollout_policy(packed[name], None, T)

    def sample(name):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(a.episodes):
            run(name)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / (a.episodes * T) * 1e6

    for k in PATHS:
        run(k)
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
    ap.add_argument("--steps", type=int, default=360)
    ap.add_argument("--episodes", type=int, default=6)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_root or not os.path.isdir(os.path.join(a.parent_root, "gym_supplychain_amd")):
        raise SystemExit("--parent-root must hold the other build's gym_supplychain_amd package")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--envs", str(a.envs), "--steps", str(a.steps), "--episodes",
           str(a.episodes)]
    builds = (("parent", os.path.abspath(a.parent_root)), ("this tree", os.path.join(REPO, "gym-supplychain_amd")))
    got = {name: {k: [] for k in PATHS} for name, _ in builds}
    for r in range(a.rounds):
        for name, root in builds:
            p = subprocess.run(cmd, env=dict(os.environ, SCG_PKG_ROOT=root), capture_output=True, text=True, timeout=600)
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
            f"{off:.3f} us {'above' if med > max(pa) else 'below'} the parent's spread"
        print(f"# {k} us/step: parent median {statistics.median(pa):.3f} min {min(pa):.3f} max {max(pa):.3f}; "
              f"this tree median {med:.3f} min {min(me):.3f} max {max(me):.3f}: {where}", flush=True)


if __name__ == "__main__":
    main()
