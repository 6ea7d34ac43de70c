"""BeerGameEnv2 closed loop: rollout_policy() with the local-information policy against the
linear policy, A/B on one env in one process.

    python tools/bg_local_rollout_ab.py [--envs 65536] [--launch-episodes 4000] [--rounds 5]

BeerGame2VecEnv at L = 4, 35 weeks, customer_demand=(0, 16), shipment_delays=(0, 5) (random
demand and per-env random delays, ledgers and returns kept, auto-reset), every env with its own
policy of 20 words: weights in [-64, 64], biases in [-2000, 2000], shift 4, clamp (0, max_order).
A sample is the wall clock of `--launch-episodes` calls of 35 weeks between two device
synchronisations, no output but reward_sum:
  local   rollout_policy(pack_local_policy(...)): four features per level (net stock, supply
          line, downstream order, own order), scg_bg_rollout_local;
  linear  rollout_policy(pack_policy(...)): the L observations per level, scg_bg_rollout_policy.
Both do 16 multiply-adds per env-week at L = 4; the local one adds the feature sums and one pass
over the live ring rows per launch. The two alternate, `--rounds` times, after one untimed
sample of each; before that one episode of each is compared bit for bit with the open-loop
rollout() of the actions it took, on a second env. Prints one JSON line per sample and a summary
line: median, minimum and maximum of each path's rounds in microseconds per week of the batch,
and whether the local median lies inside the linear path's minimum .. maximum, else by how much
it lies outside and whether that is more than the linear path's own maximum - minimum.
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

LEVELS, WEEKS, SEED, SHIFT = 4, 35, 0x5EED0000, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--launch-episodes", type=int, default=4000)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()

    import torch

    from gym_supplychain_amd import BeerGame2VecEnv
    dev = torch.device("cuda", 0)
    N, L, T = a.envs, LEVELS, WEEKS

    def make():
        env = BeerGame2VecEnv(N, weeks=T, levels=L, customer_demand=(0, 16), shipment_delays=(0, 5), seed=SEED,
                              device=dev)
        env.reset()
        return env

    closed, replayed = make(), make()
    gen = torch.Generator(device="cpu").manual_seed(SEED)
    W = torch.randint(-64, 65, (N, L, L), generator=gen, dtype=torch.int32).to(dev)
    b = torch.randint(-2000, 2001, (N, L), generator=gen, dtype=torch.int32).to(dev)
    # at L = 4 one [N, 4, 4] draw serves both layouts
    packed = {"local": closed.pack_local_policy(W, b), "linear": closed.pack_policy(W, b)}

    # one episode of each on the same env, each equal to the open-loop replay of its actions
    plan_obs = torch.empty((T, N, L), dtype=torch.int32, device=dev)
    plan_rew = torch.empty((T, N), dtype=torch.int32, device=dev)
    taken = {}
    for name in ("local", "linear"):
        res = closed.rollout_policy(packed[name], None, T, shift=SHIFT, return_actions=True, return_obs=True,
                                    return_rewards=True)
        replayed.rollout(res.actions, plan_obs, plan_rew)
        if not (torch.equal(plan_obs, res.obs) and torch.equal(plan_rew, res.rewards)):
            raise SystemExit(f"the open-loop replay of the {name} policy's actions differs")
        if not torch.equal(res.reward_sum, res.rewards.to(torch.int64).sum(0)):
            raise SystemExit(f"the {name} policy's reward_sum differs from its rewards")
        for t in ("inventory", "backlog", "orders_placed", "final_return", "_ring"):
            if not torch.equal(getattr(replayed, t), getattr(closed, t)):
                raise SystemExit(f"the {name} policy and its replay differ in {t}")
        taken[name] = res.actions
    if torch.equal(taken["local"], taken["linear"]):
        raise SystemExit("the two policies took the same actions: the A/B compares nothing")

    def run(name):
        def fn(episodes):
            for _ in range(episodes):
                closed.rollout_policy(packed[name], None, T, shift=SHIFT)
        return fn

    def sample(fn, episodes):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn(episodes)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / (episodes * T) * 1e6  # us per week of the batch

    paths = {"local": run("local"), "linear": run("linear")}
    for fn in paths.values():
        sample(fn, a.launch_episodes)
    got = {k: [] for k in paths}
    for rnd in range(a.rounds):
        for name, fn in paths.items():
            us = sample(fn, a.launch_episodes)
            got[name].append(us)
            print(json.dumps({"round": rnd, "path": name, "episodes": a.launch_episodes, "us_per_week": us,
                              "ns_per_env_step": us * 1e3 / N}), flush=True)
    closed.check_errors()
    out = {"n_envs": N, "levels": L, "weeks": T, "launch_episodes_per_sample": a.launch_episodes, "rounds": a.rounds}
    for k, v in got.items():
        out[f"{k}_median_us_per_week"] = statistics.median(v)
        out[f"{k}_min_us_per_week"] = min(v)
        out[f"{k}_max_us_per_week"] = max(v)
    med, lo, hi = out["local_median_us_per_week"], out["linear_min_us_per_week"], out["linear_max_us_per_week"]
    out["local_over_linear"] = med / out["linear_median_us_per_week"]
    out["local_median_inside_linear_min_max"] = lo <= med <= hi
    out["local_median_outside_by_us"] = 0.0 if lo <= med <= hi else (med - hi if med > hi else med - lo)
    out["local_median_above_linear_max_by_more_than_its_spread"] = med - hi > hi - lo
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
