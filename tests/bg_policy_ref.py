"""The BeerGame linear policy (include/scgpu.h, scg_bg_policy) restated in NumPy int64, for the
tests of csrc/scg_bg_policy.h and of BeerGameVecEnv.rollout_policy."""
import numpy as np


def pre_shift(weights, bias, obs):
    """z[..., l] = bias[..., l] + sum_j weights[..., l, j] * obs[..., j] in int64 arrays, which
    wrap on overflow as two's complement."""
    w, b, o = (np.asarray(x, dtype=np.int64) for x in (weights, bias, obs))
    with np.errstate(over="ignore"):
        return b + (w * o[..., None, :]).sum(axis=-1)


def actions(weights, bias, obs, shift, lo, hi):
    """min(max(z >> shift, lo), hi) as int32; >> on int64 is arithmetic (floor)."""
    return np.clip(pre_shift(weights, bias, obs) >> np.int64(shift), lo, hi).astype(np.int32)
