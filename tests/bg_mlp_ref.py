"""The BeerGame float32 MLP policy (include/scgpu.h, scg_bg_mlp; csrc/scg_bg_mlp.h) restated in
NumPy float32 for the tests: loops over the hidden units i and the inputs j, vectorised over
envs, every multiply and every add a float32 operation of its own. The features are those of
tests/bg_local_ref.py, input l*4+j being feature j of level l."""
import numpy as np

MAX_HIDDEN = 64
MAX_BOUND = 2 ** 24
F32 = np.float32


def n_words(L, H):
    return H * (4 * L + 1) + L * (H + 1)


def word(L, H, layer, r, k):
    """The word of (layer 0, unit r, input k <= 4L) or (layer 1, action r, unit k <= H)."""
    I = 4 * L
    return r * (I + 1) + k if layer == 0 else H * (I + 1) + r * (H + 1) + k


def pack(w1, b1, w2, b2):
    """float32 [Q] from w1 [H, 4L], b1 [H], w2 [L, H], b2 [L]."""
    w1, b1, w2, b2 = (np.asarray(x, dtype=F32) for x in (w1, b1, w2, b2))
    return np.concatenate([np.concatenate([w1, b1[:, None]], axis=1).ravel(),
                           np.concatenate([w2, b2[:, None]], axis=1).ravel()])


def inputs(f):
    """int features [..., L, 4] to float32 [..., 4L] (round to nearest even)."""
    f = np.asarray(f)
    return f.reshape(f.shape[:-2] + (-1,)).astype(np.int32).astype(F32)


def hidden(w1, b1, x):
    """The hidden units after the ReLU, float32 [..., H]."""
    w1, b1, x = np.asarray(w1, dtype=F32), np.asarray(b1, dtype=F32), np.asarray(x, dtype=F32)
    H, I = w1.shape
    out = np.empty(x.shape[:-1] + (H,), dtype=F32)
    with np.errstate(all="ignore"):
        for i in range(H):
            h = np.full(x.shape[:-1], b1[i], dtype=F32)
            for j in range(I):
                h = (h + (w1[i, j] * x[..., j]).astype(F32)).astype(F32)
            out[..., i] = np.where(h > 0, h, F32(0.0))
    return out


def z_values(w1, b1, w2, b2, x):
    """z [..., L] in the formula's order: unit i is folded into every z_a before unit i+1."""
    w2, b2 = np.asarray(w2, dtype=F32), np.asarray(b2, dtype=F32)
    hid = hidden(w1, b1, x)
    L, H = w2.shape
    z = np.broadcast_to(b2, hid.shape[:-1] + (L,)).astype(F32).copy()
    with np.errstate(all="ignore"):
        for i in range(H):
            for a in range(L):
                z[..., a] = (z[..., a] + (w2[a, i] * hid[..., i]).astype(F32)).astype(F32)
    return z


def sample(z, std, eps):
    """u = z + (std * eps), the product rounded first."""
    with np.errstate(all="ignore"):
        d = (np.asarray(std, dtype=F32) * np.asarray(eps, dtype=F32)).astype(F32)
        return (np.asarray(z, dtype=F32) + d).astype(F32)


def finish(u, lo, hi):
    """int32 actions: lo when not u >= lo (a NaN too), hi when u >= hi, else rint (ties to even)."""
    u = np.asarray(u, dtype=F32)
    assert -MAX_BOUND <= lo <= hi <= MAX_BOUND
    with np.errstate(all="ignore"):
        low, high = ~(u >= F32(lo)), u >= F32(hi)
        mid = np.rint(np.where(low | high, F32(0.0), u)).astype(np.int32)
    return np.where(low, np.int32(lo), np.where(high, np.int32(hi), mid)).astype(np.int32)


def one_expression(w1, b1, w2, b2, x):
    """b2 + w2 @ relu(b1 + w1 @ x) in float64, rounded to float32 once: what the formula's order
    is told apart from."""
    w1, b1, w2, b2, x = (np.asarray(v, dtype=np.float64) for v in (w1, b1, w2, b2, x))
    return (b2 + np.maximum(b1 + x @ w1.T, 0.0) @ w2.T).astype(F32)
