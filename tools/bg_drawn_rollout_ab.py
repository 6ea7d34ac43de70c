"""BeerGameEnv2 sampled closed loop with its noise drawn on the device (rollout_policy(noise_seed=,
std=)) beside the loop fed a noise tensor (rollout_policy(noise=, std=)), A/B in one process.

    python tools/bg_drawn_rollout_ab.py [--envs 65536] [--episodes 2000] [--rounds 5]

The README's BeerGame2 configuration: BeerGame2VecEnv at L = 4, 35 weeks, customer_demand=(0, 16),
shipment_delays=(0, 5) (random demand and per-env random delays, ledgers and returns kept,
auto-reset), one shared network of H = 16 hidden units, the draw of tools/bg_mlp_rollout_ab.py:
w1 ~ N/40, b1 ~ N, w2 ~ 2N/sqrt(H), b2 ~ 8 + N, std ~ 2 exp(0.3 N), clamp (0, max_order). A sample
is the wall clock of `--episodes` 35-week episodes between two device synchronisations:
  tensor          (a)  rollout_policy(noise, std) reading one [35, N, L] tensor drawn before;
  tensor_randn    (a') the same with the torch.randn that fills the tensor timed in, once per episode;
  seed            (b)  rollout_policy(noise_seed, std): no tensor; noise_row counts on per episode;
  tensor_collect  (c)  (a) with every PPO buffer written: samples_out, return_features, actions, rewards;
  seed_collect    (c)  (b) with the same buffers;
  draw_noise      (d)  draw_noise of one episode's rows alone (what a learning pass that wants the
                       tensor pays).
The paths alternate, `--rounds` times, after one untimed sample of each. Before that one episode
is compared bit for bit at the timed size: the seeded loop against the tensor loop fed
draw_noise's rows (samples, actions, obs, rewards, features, reward_sum and the state). (e) The
peak device memory of one episode of (a), noise tensor included, and of (b), above what the envs
hold, is taken after the timing with torch.cuda.max_memory_allocated, each after freeing the
other's buffers. Prints one JSON line per sample and a summary line: median, minimum and maximum
of each path's rounds in microseconds per week of the batch.
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

LEVELS, WEEKS, HIDDEN, SEED = 4, 35, 16, 0x5EED0000
NOISE_SEED = 0x9E3779B97F4A7C15
STATE = ("inventory", "backlog", "orders_placed", "inventory_costs", "backlog_costs", "penalty_costs", "episode_return",
         "final_return", "_ring")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--episodes", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()

    import torch

    from gym_supplychain_amd import BeerGame2VecEnv
    dev = torch.device("cuda", 0)
    N, L, T, H = a.envs, LEVELS, WEEKS, HIDDEN

    def make():
        env = BeerGame2VecEnv(N, weeks=T, levels=L, customer_demand=(0, 16), shipment_delays=(0, 5), seed=SEED,
                              device=dev)
        env.reset()
        return env

    names = ("tensor", "tensor_randn", "seed", "tensor_collect", "seed_collect")
    envs = {k: make() for k in names}
    first = envs["seed"]
    gen = torch.Generator(device="cpu").manual_seed(SEED)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float32)  # noqa: E731
    w1, b1 = (rnd(H, 4 * L) / 40).to(dev), rnd(H).to(dev)
    w2, b2 = (2 * rnd(L, H) / H ** 0.5).to(dev), (8 + rnd(L)).to(dev)
    std = (2 * torch.exp(0.3 * rnd(L))).to(dev)
    mlp = first.pack_local_mlp(w1, b1, w2, b2)
    noise = first.draw_noise(NOISE_SEED, T)
    samples = torch.empty_like(noise)

    # one episode of the seeded loop against the tensor loop on the same rows, bit for bit, at the timed size
    out = dict(return_actions=True, return_obs=True, return_rewards=True, return_features=True)
    e1, e2 = envs["seed"], envs["tensor"]
    s2 = torch.empty_like(noise)
    r1 = e1.rollout_policy(mlp, None, T, noise_seed=NOISE_SEED, std=std, samples_out=samples, **out)
    r2 = e2.rollout_policy(mlp, None, T, noise=noise, std=std, samples_out=s2, **out)
    same = torch.equal(samples.view(torch.int32), s2.view(torch.int32)) and \
        all(torch.equal(getattr(r1, f), getattr(r2, f)) for f in ("actions", "obs", "rewards", "features", "reward_sum"))
    same = same and all(torch.equal(getattr(e1, t), getattr(e2, t)) for t in STATE if getattr(e1, t) is not None)
    same = same and (e1.week, e1.episode) == (e2.week, e2.episode)
    if not same:
        raise SystemExit("the seeded loop differs from the tensor loop on draw_noise's rows")
    print(json.dumps({"checked": "one episode of the seeded path against the tensor path, bit for bit, state included",
                      "n_envs": N, "weeks": T, "noise_mean": float(noise.mean()), "noise_var": float(noise.var()),
                      "clamped_fraction": float(((r1.actions == 0) | (r1.actions == first.max_order)).float().mean())}),
          flush=True)
    del r1, r2, s2

    collect = dict(samples_out=samples, return_features=True, return_actions=True, return_rewards=True)

    def path(name):
        env = envs[name]
        kw = collect if name.endswith("collect") else {}

        def run(episodes):
            for ep in range(episodes):
                if name.startswith("seed"):
                    env.rollout_policy(mlp, None, T, noise_seed=NOISE_SEED, noise_row=ep * T, std=std, **kw)
                else:
                    if name == "tensor_randn":
                        noise.normal_()
                    env.rollout_policy(mlp, None, T, noise=noise, std=std, **kw)
        return run

    def sample(fn, episodes):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn(episodes)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / (episodes * T) * 1e6  # us per week of the batch

    paths = {k: path(k) for k in names}
    paths["draw_noise"] = lambda episodes: [first.draw_noise(NOISE_SEED, T, out=noise) for _ in range(episodes)]
    for fn in paths.values():
        sample(fn, max(a.episodes // 4, 1))
    got = {k: [] for k in paths}
    for r in range(a.rounds):
        for name, fn in paths.items():
            us = sample(fn, a.episodes)
            got[name].append(us)
            print(json.dumps({"round": r, "path": name, "us_per_week": us, "ns_per_env_step": us * 1e3 / N}), flush=True)
    for env in envs.values():
        env.check_errors()

    # (e) peak device memory of one episode, above what the envs and the policy hold
    del noise, samples, collect
    peak = {}
    for kind in ("seed", "tensor"):
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        if kind == "seed":
            envs["seed"].rollout_policy(mlp, None, T, noise_seed=NOISE_SEED, std=std)
        else:
            eps = torch.randn((T, N, L), device=dev)
            envs["tensor"].rollout_policy(mlp, None, T, noise=eps, std=std)
            del eps
        torch.cuda.synchronize(dev)
        peak[kind] = torch.cuda.max_memory_allocated(dev) - base

    med = {k: statistics.median(v) for k, v in got.items()}
    res = {"n_envs": N, "levels": L, "weeks": T, "hidden": H, "episodes_per_sample": a.episodes, "rounds": a.rounds,
           "noise_bytes_per_env_week": 4 * L, "noise_mb_per_episode": 4e-6 * L * N * T,
           "peak_bytes_above_envs_tensor": peak["tensor"], "peak_bytes_above_envs_seed": peak["seed"]}
    for k in paths:
        res[f"{k}_median_us_per_week"] = med[k]
        res[f"{k}_min"] = min(got[k])
        res[f"{k}_max"] = max(got[k])
    res["seed_minus_tensor_us"] = med["seed"] - med["tensor"]
    res["seed_minus_tensor_randn_us"] = med["seed"] - med["tensor_randn"]
    res["seed_collect_minus_tensor_collect_us"] = med["seed_collect"] - med["tensor_collect"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
