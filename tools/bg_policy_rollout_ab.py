"""BeerGameEnv2 closed loop: step() per week with the policy in torch against one
rollout_policy() per episode, A/B in one process.

    python tools/bg_policy_rollout_ab.py [--envs 65536] [--episodes 200] [--launch-episodes 4000] [--pairs 5]

BeerGame2VecEnv at L = 4, 35 weeks, customer_demand=(0, 16), shipment_delays=(0, 5) (random
demand and per-env random delays, ledgers and returns kept, auto-reset), every env with its own
linear policy: weights in [-64, 64], biases in [-2000, 2000], shift 4, clamp (0, max_order). A
sample is the wall clock of whole episodes between two device synchronisations, `--episodes` of
them for the step loop and `--launch-episodes` for the two one-launch paths (a third of a second
of work each at the defaults):
  step_loop       the closed loop as it can be written without rollout_policy(): per week the
                  policy in torch int64 ops on the device (observation -> action), then step();
  rollout_policy  one rollout_policy() of 35 weeks per episode, parameters packed once, no
                  output but reward_sum;
  rollout         the open-loop rollout() of 35 weeks per episode fed the actions that
                  rollout_policy took: what the 36 B per env-week of action, observation and
                  reward rows cost beside it (a yardstick, not a closed loop).
step_loop and rollout_policy alternate, `--pairs` times, with a rollout sample after each pair,
after one untimed sample of each; before that one episode of the two closed loops is compared
bit for bit, and the open-loop replay against both. Prints one JSON line per sample and a
summary line: medians and max - min of the time per env-step, and the host's time to enqueue one
call of each one-launch path on an idle device (below the call's device time, the host is hidden).
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
    ap.add_argument("--episodes", type=int, default=200)
    ap.add_argument("--launch-episodes", type=int, default=4000)
    ap.add_argument("--pairs", type=int, default=5)
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

    stepped, closed, replayed = make(), make(), make()
    gen = torch.Generator(device="cpu").manual_seed(SEED)
    W = torch.randint(-64, 65, (N, L, L), generator=gen, dtype=torch.int32).to(dev)
    b = torch.randint(-2000, 2001, (N, L), generator=gen, dtype=torch.int32).to(dev)
    packed = closed.pack_policy(W, b)
    W64, b64 = W.to(torch.int64), b.to(torch.int64)
    lo, hi = 0, stepped.max_order

    def torch_policy(obs):  # the formula of include/scgpu.h (scg_bg_policy) in torch int64 ops
        z = b64 + (W64 * obs.to(torch.int64).unsqueeze(1)).sum(dim=2)
        return (z >> SHIFT).clamp_(lo, hi).to(torch.int32)

    # the two closed loops compute the same episode (at the timed size); so does the replay
    res = closed.rollout_policy(packed, None, T, shift=SHIFT, return_actions=True, return_obs=True, return_rewards=True)
    obs = stepped._obs
    sums = torch.zeros(N, dtype=torch.int64, device=dev)
    for w in range(T):
        act = torch_policy(obs)
        if not torch.equal(act, res.actions[w]):
            raise SystemExit(f"rollout_policy and the step loop differ in the action of week {w + 1}")
        obs, r, _, _ = stepped.step(act)
        sums += r
        if not (torch.equal(obs, res.obs[w]) and torch.equal(r, res.rewards[w])):
            raise SystemExit(f"rollout_policy and the step loop differ at week {w + 1}")
    if not torch.equal(sums, res.reward_sum):
        raise SystemExit("rollout_policy's reward_sum differs from the step loop's rewards")
    acts = res.actions
    plan_obs = torch.empty((T, N, L), dtype=torch.int32, device=dev)
    plan_rew = torch.empty((T, N), dtype=torch.int32, device=dev)
    replayed.rollout(acts, plan_obs, plan_rew)
    if not (torch.equal(plan_obs, res.obs) and torch.equal(plan_rew, res.rewards)):
        raise SystemExit("the open-loop replay of the actions taken differs")
    for t in ("inventory", "backlog", "orders_placed", "final_return", "_ring"):
        if not (torch.equal(getattr(stepped, t), getattr(closed, t)) and
                torch.equal(getattr(replayed, t), getattr(closed, t))):
            raise SystemExit(f"the paths differ in {t}")

    def step_loop(episodes):
        o = stepped._obs
        for _ in range(episodes):
            for _w in range(T):
                o = stepped.step(torch_policy(o))[0]

    def rollout_policy(episodes):
        for _ in range(episodes):
            closed.rollout_policy(packed, None, T, shift=SHIFT)

    def rollout(episodes):
        for _ in range(episodes):
            replayed.rollout(acts, plan_obs, plan_rew)

    def sample(fn, episodes):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn(episodes)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / (episodes * T * N) * 1e9  # ns per env-step

    def enqueue_us(fn, calls=50):  # host time to enqueue one call on an idle device (no synchronise inside)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn(calls)
        t1 = time.perf_counter()
        torch.cuda.synchronize(dev)
        return (t1 - t0) / calls * 1e6

    paths = {"step_loop": (step_loop, a.episodes), "rollout_policy": (rollout_policy, a.launch_episodes),
             "rollout": (rollout, a.launch_episodes)}
    for fn, episodes in paths.values():
        sample(fn, episodes)
    got = {k: [] for k in paths}
    for pair in range(a.pairs):
        for name, (fn, episodes) in paths.items():
            ns = sample(fn, episodes)
            got[name].append(ns)
            print(json.dumps({"pair": pair, "path": name, "episodes": episodes, "ns_per_env_step": ns,
                              "us_per_episode": ns * T * N / 1e3}), flush=True)
    host = {"rollout_policy": enqueue_us(rollout_policy), "rollout": enqueue_us(rollout)}
    for env in (stepped, closed, replayed):
        env.check_errors()
    med = {k: statistics.median(v) for k, v in got.items()}
    spread = {k: max(v) - min(v) for k, v in got.items()}
    out = {"n_envs": N, "levels": L, "weeks": T, "episodes_per_sample": a.episodes,
           "launch_episodes_per_sample": a.launch_episodes, "pairs": a.pairs}
    for k in paths:
        out[f"{k}_median_ns_per_env_step"] = med[k]
        out[f"{k}_max_minus_min"] = spread[k]
        out[f"{k}_median_us_per_week"] = med[k] * N / 1e3
    for k, v in host.items():
        out[f"{k}_host_enqueue_us_per_call"] = v
    out["step_loop_over_rollout_policy"] = med["step_loop"] / med["rollout_policy"]
    out["rollout_over_rollout_policy"] = med["rollout"] / med["rollout_policy"]
    out["rollout_policy_below_step_loop_by_more_than_its_spread"] = \
        med["step_loop"] - med["rollout_policy"] > spread["step_loop"]
    out["rollout_policy_below_rollout_by_more_than_its_spread"] = med["rollout"] - med["rollout_policy"] > spread["rollout"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
