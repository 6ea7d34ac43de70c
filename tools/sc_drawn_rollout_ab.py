"""SupplyChain sampled closed loop with its noise drawn on the device (rollout_policy(noise_seed=,
std=)) beside the loop fed a noise tensor (rollout_policy(noise=, std=)), A/B in one process.

    python tools/sc_drawn_rollout_ab.py [--envs 65536] [--steps 360] [--episodes 4] [--rounds 5] [--hidden 16]

sc-2perstage-v0 (A = 14, O = 27), float32 observations, auto-reset, the node-parallel kernel, one
shared linear policy (W N(0, 0.1), b N(0, 0.3)) and one shared MLP of `--hidden` units (W1 N(0,
0.1), b1 N(0, 0.3), W2 N(0, 0.3), b2 N(0, 0.3)), clip (-1, 1), std U[0.05, 0.6] per action. A
sample is the wall clock of `--episodes` episodes of `--steps` steps between two device
synchronisations, per policy P in (linear, mlp):
  P_tensor            (a) rollout_policy(noise, std) reading one [steps, N, A] tensor drawn before;
  P_tensor_randn      (a) the same with the torch.randn that fills the tensor timed in, once per episode;
  P_seed              (b) rollout_policy(noise_seed, std): no tensor;
  P_tensor_samples    (c) (a) with samples_out;
  P_seed_samples      (c) (b) with samples_out;
and, once, draw_noise of one episode's rows (what a learning pass that wants the tensor pays).
The paths alternate, `--rounds` times, after one untimed sample of each. Before that one episode
is compared bit for bit at the timed size: the seeded loops against the tensor loops fed
draw_noise's rows (samples, actions, rewards, reward_sum, last observation, state). (d) The peak
device memory of one episode of (a), noise tensor included, and of (b) is taken after the timing
with torch.cuda.max_memory_allocated, each after freeing the other's buffers. Prints one JSON
line per sample and a summary line: medians, min and max of the microseconds per step of the batch.
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
NOISE_SEED = 0x9E3779B97F4A7C15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=360)
    ap.add_argument("--episodes", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hidden", type=int, default=16)
    a = ap.parse_args()

    import torch

    import gym_supplychain_amd as gsa
    dev = torch.device("cuda", 0)
    N, T, H = a.envs, a.steps, a.hidden

    def make():
        env = gsa.make_vec("sc-2perstage-v0", N, seed=SEED, device=dev, kernel="nodes", total_time_steps=T,
                           obs_dtype=torch.float32)
        env.reset()
        return env

    kinds = ("tensor", "tensor_randn", "seed", "tensor_samples", "seed_samples")
    names = tuple(f"{p}_{k}" for p in ("linear", "mlp") for k in kinds)
    envs = {k: make() for k in names}
    first = envs["linear_seed"]
    A, O = first.n_actions, first.n_obs
    gen = torch.Generator(device="cpu").manual_seed(SEED)

    def rnd(shape, scale):
        return (torch.randn(shape, generator=gen) * scale).to(dev)

    W, b = rnd((A, O), 0.1), rnd((A,), 0.3)
    w1, b1, w2, b2 = rnd((H, O), 0.1), rnd((H,), 0.3), rnd((A, H), 0.3), rnd((A,), 0.3)
    std = (torch.rand(A, generator=gen) * 0.55 + 0.05).to(dev)
    if not first.mlp_fused(H):
        raise SystemExit("this hidden width does not run fused on this scenario")
    packed = {"linear": first.pack_policy(W, b), "mlp": first.pack_mlp(w1, b1, w2, b2)}
    noise = first.draw_noise(NOISE_SEED, T)
    samples = torch.empty_like(noise)

    # one episode of the seeded loop against the tensor loop on the same rows, bit for bit, at the timed size
    out = dict(return_actions=True, return_rewards=True)
    for p in ("linear", "mlp"):
        e1, e2 = envs[f"{p}_seed"], envs[f"{p}_tensor"]
        s2 = torch.empty_like(noise)
        r1 = e1.rollout_policy(packed[p], None, T, noise_seed=NOISE_SEED, std=std, samples_out=samples, **out)
        r2 = e2.rollout_policy(packed[p], None, T, noise=noise, std=std, samples_out=s2, **out)
        same = torch.equal(samples, s2) and all(torch.equal(getattr(r1, f), getattr(r2, f))
                                                for f in ("actions", "rewards", "reward_sum", "last_obs"))
        same = same and all(torch.equal(getattr(e1, t), getattr(e2, t)) for t in ("_stock", "_heap_size", "_ret", "_final_ret", "_term_obs"))
        if not same:
            raise SystemExit(f"the seeded {p} loop differs from the tensor loop on draw_noise's rows")
        del r1, r2, s2
    print(json.dumps({"checked": "one episode of the seeded paths against the tensor paths, bit for bit", "n_envs": N, "steps": T,
                      "noise_mean": float(noise.mean()), "noise_var": float(noise.var())}), flush=True)

    def path(name):
        env = envs[name]
        p, kind = name.split("_", 1)
        so = samples if kind.endswith("samples") else None

        def run(episodes):
            for ep in range(episodes):
                if kind.startswith("seed"):
                    env.rollout_policy(packed[p], None, T, noise_seed=NOISE_SEED, noise_row=ep * T, std=std, samples_out=so)
                else:
                    if kind == "tensor_randn":
                        noise.normal_()
                    env.rollout_policy(packed[p], None, T, noise=noise, std=std, samples_out=so)
        return run

    def sample(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn(a.episodes)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / (a.episodes * T) * 1e6  # us per step of the batch

    paths = {k: path(k) for k in names}
    paths["draw_noise"] = lambda episodes: [first.draw_noise(NOISE_SEED, T, out=noise) for _ in range(episodes)]
    for fn in paths.values():
        sample(fn)
    got = {k: [] for k in paths}
    for r in range(a.rounds):
        for name, fn in paths.items():
            us = sample(fn)
            got[name].append(us)
            print(json.dumps({"round": r, "path": name, "us_per_step": us}), flush=True)
    for env in envs.values():
        env.check_errors()

    # (d) peak device memory of one linear episode, above what the envs and policies hold
    del noise, samples
    peak = {}
    for kind in ("seed", "tensor"):
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        if kind == "seed":
            envs["linear_seed"].rollout_policy(packed["linear"], None, T, noise_seed=NOISE_SEED, std=std)
        else:
            eps = torch.randn((T, N, A), device=dev)
            envs["linear_tensor"].rollout_policy(packed["linear"], None, T, noise=eps, std=std)
            del eps
        torch.cuda.synchronize(dev)
        peak[kind] = torch.cuda.max_memory_allocated(dev) - base

    med = {k: statistics.median(v) for k, v in got.items()}
    res = {"n_envs": N, "steps": T, "episodes_per_sample": a.episodes, "rounds": a.rounds, "hidden": H,
           "noise_bytes_per_env_step": 4 * A, "noise_gb_per_episode": 4e-9 * A * N * T,
           "peak_bytes_above_envs_tensor": peak["tensor"], "peak_bytes_above_envs_seed": peak["seed"]}
    for k in paths:
        res[f"{k}_median_us_per_step"] = med[k]
        res[f"{k}_min"] = min(got[k])
        res[f"{k}_max"] = max(got[k])
    for p in ("linear", "mlp"):
        res[f"{p}_seed_minus_tensor_us"] = med[f"{p}_seed"] - med[f"{p}_tensor"]
        res[f"{p}_seed_minus_tensor_randn_us"] = med[f"{p}_seed"] - med[f"{p}_tensor_randn"]
        res[f"{p}_seed_samples_minus_tensor_samples_us"] = med[f"{p}_seed_samples"] - med[f"{p}_tensor_samples"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
