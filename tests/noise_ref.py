"""The project's float32 normal (csrc/scg_normal.h) restated in NumPy — TEST INFRASTRUCTURE ONLY.

Element (row k, env id e, action a) of the exploration noise of a 64-bit seed:

    blk      = philox4x32_10(ctr = (e, k, a >> 2, STREAM_SC_NOISE), key = (seed & 0xffffffff, seed >> 32))
    (w1, w2) = (blk.x, blk.y) for pair (a >> 1) & 1 == 0, (blk.z, blk.w) for pair 1
    m = (w1 >> 8) + 1            u = m * 2^-24 in (0, 1]
    v = w2 >> 8                  theta = 2 pi v * 2^-24
    eps = r cos(theta) for even a, r sin(theta) for odd a,   r = sqrt(-2 ln u)

r, cos and sin come from float32 adds, subtracts, multiplies, divides and square roots alone, each
rounded on its own (no FMA, no libm), and integer work; every operation below carries its own
.astype(np.float32). Philox is oracle/philox.py's."""
import numpy as np

from oracle.philox import philox4x32_10, seed_key

STREAM_SC_NOISE = 6
F = np.float32

LN2_HI = np.uint32(0x3F317180).view(F)  # 0.693138122558594: 15 significant bits, an exponent times it is exact
LN2_LO = np.uint32(0x3717F7D1).view(F)  # ln 2 - LN2_HI
SQRT2_MANT = 0x3504F3                   # mantissa bits of sqrt(2)
LOG_P = [F(1.0) / F(3.0), F(1.0) / F(5.0), F(1.0) / F(7.0), F(1.0) / F(9.0)]  # the rounded quotients
# sin(pi/4 t) = t (S0 + S1 t^2 + S2 t^4 + S3 t^6), cos(pi/4 t) = 1 + t^2 (C0 + C1 t^2 + C2 t^4 + C3 t^6) on t in [0, 1]
SIN_HI, SIN_LO = np.uint32(0x3F490FDB).view(F), np.uint32(0xB2D088A5).view(F)  # S0 in two words
SIN_S = [np.uint32(x).view(F) for x in (0xBDA55DDD, 0x3B232F62, 0xB816CDA0)]
COS_C = [np.uint32(x).view(F) for x in (0xBE9DE9E6, 0x3C81E0F5, 0xB9AAE5CC, 0x366DB249)]

# The transform's worst errors against float64 over all 2^24 inputs of each factor
# (tests/test_noise_host.py recomputes them): |r - r64| and |sin - sin64|, |cos - cos64|.
R_MAX = float(np.sqrt(48.0 * np.log(2.0)))


def _mul(a, b):
    return (a * b).astype(F)


def _add(a, b):
    return (a + b).astype(F)


def radius(m):
    """r = sqrt(-2 ln(m * 2^-24)) for uint32 m in [1, 2^24], float32."""
    m = np.asarray(m, dtype=np.uint32)
    bits = m.astype(F).view(np.uint32)  # exact: m <= 2^24
    mant = bits & np.uint32(0x7FFFFF)
    fold = mant > np.uint32(SQRT2_MANT)
    e = (bits >> np.uint32(23)).astype(np.int32) - 127 - 24 + fold.astype(np.int32)
    f = (mant | np.where(fold, np.uint32(0x3F000000), np.uint32(0x3F800000))).astype(np.uint32).view(F)  # [sqrt 1/2, sqrt 2)
    ef = e.astype(F)
    s = ((f - F(1.0)).astype(F) / (f + F(1.0)).astype(F)).astype(F)
    s2 = _mul(s, s)
    p = LOG_P[3]
    for c in (LOG_P[2], LOG_P[1], LOG_P[0]):
        p = _add(_mul(p, s2), c)
    two_s = _add(s, s)
    lnf = _add(two_s, _mul(two_s, _mul(s2, p)))
    lnu = _add(_mul(ef, LN2_HI), _add(_mul(ef, LN2_LO), lnf))
    return np.sqrt(_mul(F(-2.0), lnu)).astype(F)


def cos_sin(v):
    """(cos, sin) of 2 pi v * 2^-24 for uint32 v in [0, 2^24), float32."""
    v = np.asarray(v, dtype=np.uint32)
    quad = v >> np.uint32(22)
    rem = v & np.uint32(0x3FFFFF)
    refl = rem > np.uint32(0x200000)
    rem = np.where(refl, np.uint32(0x400000) - rem, rem).astype(np.uint32)
    t = _mul(rem.astype(F), F(2.0 ** -21))  # exact, in [0, 1]: the angle is pi/4 t
    t2 = _mul(t, t)
    ps = SIN_S[2]
    for c in (SIN_S[1], SIN_S[0], SIN_LO):
        ps = _add(_mul(ps, t2), c)
    sn = _add(_mul(t, SIN_HI), _mul(t, ps))
    pc = COS_C[3]
    for c in (COS_C[2], COS_C[1], COS_C[0]):
        pc = _add(_mul(pc, t2), c)
    cs = _add(F(1.0), _mul(t2, pc))
    sa = np.where(refl, cs, sn)  # of the angle within the quadrant
    ca = np.where(refl, sn, cs)
    c = np.where(quad == 0, ca, np.where(quad == 1, -sa, np.where(quad == 2, -ca, sa)))
    s = np.where(quad == 0, sa, np.where(quad == 1, ca, np.where(quad == 2, -sa, -ca)))
    return c.astype(F), s.astype(F)


def from_words(w1, w2):
    """(r cos, r sin) of the pair of Philox words, float32."""
    w1 = np.asarray(w1, dtype=np.uint32)
    w2 = np.asarray(w2, dtype=np.uint32)
    r = radius((w1 >> np.uint32(8)) + np.uint32(1))
    c, s = cos_sin(w2 >> np.uint32(8))
    return _mul(r, c), _mul(r, s)


def element(seed, k, e, a):
    """Element (k, e, a), broadcast over uint32-valued integer arrays."""
    k, e, a = np.broadcast_arrays(np.asarray(k, dtype=np.uint64), np.asarray(e, dtype=np.uint64), np.asarray(a, dtype=np.uint64))
    ctr = np.zeros(k.shape + (4,), dtype=np.uint32)
    ctr[..., 0] = (e & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[..., 1] = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[..., 2] = (a >> np.uint64(2)).astype(np.uint32)
    ctr[..., 3] = np.uint32(STREAM_SC_NOISE)
    blk = philox4x32_10(ctr, seed_key(seed))
    second = ((a >> np.uint64(1)) & np.uint64(1)).astype(bool)
    w1 = np.where(second, blk[..., 2], blk[..., 0])
    w2 = np.where(second, blk[..., 3], blk[..., 1])
    c, s = from_words(w1, w2)
    return np.where((a & np.uint64(1)).astype(bool), s, c).astype(F)


def rows(seed, n_steps, n_envs, n_actions, row0=0, env_offset=0):
    """float32 [K, N, A]: rows row0 .. row0 + K - 1 of envs env_offset .. env_offset + N - 1."""
    G = (n_actions + 3) // 4  # element()'s numbers, one Philox block per 4 actions
    ctr = np.zeros((n_steps, n_envs, G, 4), dtype=np.uint32)
    ctr[..., 0] = ((np.arange(n_envs, dtype=np.uint64) + np.uint64(env_offset)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)[None, :, None]
    ctr[..., 1] = ((np.arange(n_steps, dtype=np.uint64) + np.uint64(row0)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None, None]
    ctr[..., 2] = np.arange(G, dtype=np.uint32)[None, None, :]
    ctr[..., 3] = np.uint32(STREAM_SC_NOISE)
    blk = philox4x32_10(ctr, seed_key(seed))
    out = np.empty((n_steps, n_envs, G, 4), dtype=F)
    out[..., 0], out[..., 1] = from_words(blk[..., 0], blk[..., 1])
    out[..., 2], out[..., 3] = from_words(blk[..., 2], blk[..., 3])
    return np.ascontiguousarray(out.reshape(n_steps, n_envs, 4 * G)[:, :, :n_actions])
