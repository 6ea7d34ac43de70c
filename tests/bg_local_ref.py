"""The BeerGame local-information policy (include/scgpu.h, scg_bg_local_policy) restated for the
tests of csrc/scg_bg_local.h and of BeerGameVecEnv.rollout_policy / policy_features: the four
features from a CPU oracle's attributes (oracle.beergame.BeerGameOracle / BeerGame2Oracle), the
actions in NumPy int64, the parameter-word index and the live-row mask."""
import numpy as np

FEATURES = 4
MAX_DELAY = 64


def _wrap32(x):
    """An int64 array reduced to int32 two's complement."""
    return ((np.asarray(x, dtype=np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int64)


def line_parts(o):
    """(orders_placed, upstream backlog, in transit) of every level, int64 [3, L]: the three
    terms of `line` for the oracle's state after its week o.week, horizon o.max_weeks."""
    L, w, T = o.levels, o.week, o.max_weeks
    up = np.zeros(L, dtype=np.int64)
    up[:-1] = o.backlog[1:]
    transit = np.asarray(o.shipments[w + 1:T + 1], dtype=np.int64).reshape(-1, L).sum(axis=0)
    return np.stack([np.asarray(o.orders_placed, dtype=np.int64), up, transit])


def features_from(net, backlog, orders_placed, transit, last_demand):
    """int64 [L, 4] (net, line, down, own), each wrapped to int32, from per-level arrays [L]."""
    net, bk, op, tr = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (net, backlog, orders_placed, transit))
    up = np.append(bk[1:], 0)
    down = np.append(np.int64(last_demand), op[:-1])
    return _wrap32(np.stack([net, op + up + tr, down, op], axis=1))


def features(o, max_stock=0):
    """int64 [L, 4] (net, line, down, own) of the oracle `o`; max_stock as BeerGameEnv2 adds it
    to the observation (0 for BeerGameEnv)."""
    last = o.customer_demand[o.week - 1] if o.week > 0 else o.orders_value
    net = np.asarray(o.inventory, dtype=np.int64) - np.asarray(o.backlog, dtype=np.int64) + max_stock
    want = features_from(net, o.backlog, o.orders_placed, line_parts(o)[2], last)
    assert np.array_equal(want[:, 1], _wrap32(line_parts(o).sum(axis=0)))
    return want


def pre_shift(weights, bias, f):
    """z[..., l] = bias[..., l] + sum_j weights[..., l, j] * f[..., l, j] in int64 arrays, which
    wrap on overflow as two's complement."""
    w, b, f = (np.asarray(x, dtype=np.int64) for x in (weights, bias, f))
    with np.errstate(over="ignore"):
        return b + (w * f).sum(axis=-1)


def actions(weights, bias, f, shift, lo, hi):
    """min(max(z >> shift, lo), hi) as int32; >> on int64 is arithmetic (floor)."""
    return np.clip(pre_shift(weights, bias, f) >> np.int64(shift), lo, hi).astype(np.int32)


def word(l, j):
    """Parameter word of W[l][j] (j < 4) or b[l] (j == 4)."""
    return l * (FEATURES + 1) + j


def live_weeks(delays, T, w0):
    """The weeks v in w0+1..T that weeks <= w0 of the episode have scheduled: the initial
    pipeline 1..min(d_0, T), and w + d_w for every week 1 <= w <= w0 with d_w > 0."""
    live = {v for v in range(1, min(int(delays[0]), T) + 1)}
    live |= {w + int(delays[w]) for w in range(1, w0 + 1) if delays[w] > 0}
    return sorted(v for v in live if w0 < v <= T)


def live_mask(delays, T, w0):
    """Bit j-1 set for every live week w0 + j (all within 64 weeks when no delay exceeds 64)."""
    assert max(int(d) for d in delays[:T + 1]) <= MAX_DELAY
    return sum(1 << (v - w0 - 1) for v in live_weeks(delays, T, w0))


def live_mask_stochastic(R, T, w0):
    """Every j <= min(R - 1, T - w0)."""
    return (1 << max(min(R - 1, T - w0, MAX_DELAY), 0)) - 1
