"""The slab step kernel by demand mode: back-to-back launches at 65,536 envs (ledgers, history,
returns, auto-reset on) in FIXED / TABLE / POISSON mode, alternating. Per mode and repetition:
the event-bracketed region time per step (as tools/floor_probe.py times its wall figure) and
the kernel's own dispatch duration over every 7th launch. FIXED has no Philox and no threshold
table, so it bounds what the POISSON kernel can reach (profiles/r07a_bg_demand_mode_ceiling.log).

    REPS=7 python tools/demand_mode_probe.py
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SCG_PKG_ROOT") or os.path.join(REPO, "gym-supplychain_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import bench  # noqa: E402
from gym_supplychain_amd import BeerGameVecEnv  # noqa: E402

N, L, T = 65536, bench.LEVELS, bench.WEEKS
K = 3500
REPS = int(os.environ.get("REPS", "7"))
dev = torch.device("cuda", 0)
kw = dict(seed=bench.SEED, device=dev, auto_reset=True, track_costs=True, track_history=True, track_returns=True)
table = torch.randint(0, 17, (T, N), dtype=torch.int32, device=dev)
envs = {
    "FIXED": BeerGameVecEnv(N, {}, demand="fixed", **kw),
    "TABLE": BeerGameVecEnv(N, {}, demand=table, **kw),
    "POISSON": BeerGameVecEnv(N, {}, demand="poisson", poisson_lambda=bench.LAMBDA, **kw),
}
acts = torch.randint(0, 9, (T, N, L), dtype=torch.int32, device=dev)
week = list(acts.unbind(0))


def timed(env, k):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(350):
        env.step(week[env.week])
    torch.cuda.synchronize()
    s.record()
    for _ in range(k):
        env.step(week[env.week])
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / k * 1e3


from gym_supplychain_amd import _native as nat  # noqa: E402

EV = [(nat.hip_event(), nat.hip_event()) for _ in range(K // 7 + 1)]


def stamped(env, k):
    """Mean of the kernel's own dispatch duration over every 7th of k back-to-back launches."""
    for _ in range(350):
        env.step(week[env.week])
    torch.cuda.synchronize()
    used = 0
    for i in range(k):
        if i % 7 == 0:
            env.step(week[env.week], EV[used])
            used += 1
        else:
            env.step(week[env.week])
    torch.cuda.synchronize()
    d = sorted(nat.hip_event_elapsed_ms(s, e) * 1e3 for s, e in EV[:used])
    return sum(d) / used, d[used // 2]


for env in envs.values():
    env.reset()
res = {m: [] for m in envs}
ker = {m: [] for m in envs}
for r in range(REPS):
    for m, env in envs.items():
        us = timed(env, K)
        mean, med = stamped(env, K)
        res[m].append(us)
        ker[m].append(mean)
        print(json.dumps({"rep": r, "mode": m, "region_us_per_step": round(us, 4), "kernel_mean_us": round(mean, 4),
                          "kernel_median_us": round(med, 4)}), flush=True)
for name, table in (("region_us_per_step", res), ("kernel_mean_us", ker)):
    for m, v in table.items():
        v = sorted(v)
        print(json.dumps({"quantity": name, "mode": m, "median": round(v[len(v) // 2], 4), "min": round(v[0], 4),
                          "max": round(v[-1], 4), "spread": round(v[-1] - v[0], 4), "launches": K, "reps": REPS,
                          "n_envs": N}), flush=True)
