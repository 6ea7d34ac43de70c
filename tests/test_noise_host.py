"""The project's float32 normal (csrc/scg_normal.h) on the host, against its NumPy restatement
(tests/noise_ref.py), and the restatement against float64 and against the normal distribution.

A stand-alone program with its own main (tests/native/noise_main.cpp) includes the header alone
and prints the radius over all 2^24 m and cos / sin over all 2^24 v as a checksum plus every
4,099th value, the edge words, and elements (k, e, a) of three seeds through Philox. It is built
with -fsanitize=address,undefined as tests/test_sc_sampled_host.py builds its own (a plain
executable; nothing here is loaded into Python). Every printed value is recomputed here.

Accuracy is a property of the transform alone and is measured exhaustively, so it is
deterministic: E_R and E_T below are the measured maxima, and the bound they give on
|eps - eps64| must lie within 2^-18.

The distribution checks take 2^22 elements drawn as rows [32, 9363, 14] cut to 2^22 (32 * 9362 * 14
is 128 short of 2^22, so one more env than a division rounded down gives). Their bounds are 6
sigma of the exact sampling distributions (the Kolmogorov bound 1.95 / sqrt(n) is the 0.1 % point),
so a true normal sample passes: NumPy's own does, below."""
import os
import subprocess

import numpy as np
import pytest
from scipy.special import ndtr

import noise_ref
from conftest import PKG_ROOT, REPO

SRC = os.path.join(REPO, "tests", "native", "noise_main.cpp")
OUT = os.path.join(REPO, "tests", "native", "_build", "noise")
CSRC = os.path.join(PKG_ROOT, "csrc")

# max |r - r64| over m = 1 .. 2^24 and max(|sin - sin64|, |cos - cos64|) over v = 0 .. 2^24 - 1
E_R = float.fromhex("0x1.7acfd3bp-22")   # 3.528e-7, at m = 3060
E_T = float.fromhex("0x1.45082ba8p-24")  # 7.568e-8
# The float64 references come from the platform's log / sin / cos, good to an ulp or so of values
# below 6 (2^-50): the measured maxima are compared to the recorded ones within 2^-40, five
# orders below the errors themselves.
E_SLACK = 2.0 ** -40

N24 = 1 << 24


def build():
    deps = [SRC, os.path.join(REPO, "include", "scgpu.h"), os.path.join(CSRC, "scg_normal.h"),
            os.path.join(CSRC, "scg_philox.h")]
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    tmp = f"{OUT}.{os.getpid()}.tmp"  # concurrent test workers: build aside, rename into place
    subprocess.run(["hipcc", "-std=c++17", "-O1", "-g", "--offload-host-only", "-Wall", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I", os.path.join(REPO, "include"), "-I", CSRC, "-o", tmp, SRC], check=True)
    os.replace(tmp, OUT)
    return OUT


@pytest.fixture(scope="module")
def lines():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([build()], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    out = []
    for line in r.stdout.strip().splitlines():
        kind, *kv = line.split()
        out.append((kind, dict(x.split("=") for x in kv)))
    return out


@pytest.fixture(scope="module")
def sweeps():
    """The restatement over every input: radius [2^24] for m = 1 .. 2^24, cos and sin [2^24]."""
    r = noise_ref.radius(np.arange(1, N24 + 1, dtype=np.uint32))
    c, s = noise_ref.cos_sin(np.arange(N24, dtype=np.uint32))
    return {"radius": r, "cos": c, "sin": s}


def _of(lines, kind):
    return [d for k, d in lines if k == kind]


def _bits(x):
    return int(np.asarray(x, dtype=np.float32).view(np.uint32))


def test_the_host_sweeps_equal_the_numpy_loop(lines, sweeps):
    got = {d["name"]: d for d in _of(lines, "sweep")}
    assert set(got) == {"radius", "cos", "sin"}
    weight = 2 * np.arange(N24, dtype=np.uint64) + np.uint64(1)
    for name, want in sweeps.items():
        d = got[name]
        b = want.view(np.uint32)
        assert int(d["n"]) == N24
        every = np.array([int(x, 16) for x in d["every"].split(",")], dtype=np.uint32)
        assert np.array_equal(every, b[::4099]), name
        with np.errstate(over="ignore"):
            total = int((b.astype(np.uint64) * weight).sum(dtype=np.uint64))  # mod 2^64
        assert int(d["sum"], 16) == total, name


def test_edge_words(lines, sweeps):
    ms = _of(lines, "edge_m")
    assert [int(d["m"]) for d in ms] == [1, 2, 1 << 23, N24 - 1, N24]
    for d in ms:
        assert int(d["r"], 16) == _bits(noise_ref.radius(np.uint32(int(d["m"])))), d
    assert int(ms[-1]["r"], 16) == 0x80000000  # m = 2^24: ln u = 0 and r = sqrt(-0.0) = -0.0, everywhere
    assert _bits(sweeps["radius"][0]) == int(ms[0]["r"], 16) and float(sweeps["radius"][0]) == float(sweeps["radius"].max())
    vs = _of(lines, "edge_v")
    want_v = [((o << 21) + d) % N24 for o in range(9) for d in (-1, 0, 1)]
    assert [int(d["v"]) for d in vs] == want_v
    for d in vs:
        c, s = noise_ref.cos_sin(np.uint32(int(d["v"])))
        assert (int(d["c"], 16), int(d["s"], 16)) == (_bits(c), _bits(s)), d
    # the axes are exact, and the two polynomials meet at the octant's end within an ulp of 0.7
    by_v = {int(d["v"]): (np.uint32(int(d["c"], 16)).view(np.float32), np.uint32(int(d["s"], 16)).view(np.float32)) for d in vs}
    assert [tuple(float(x) for x in by_v[q << 22]) for q in range(4)] == [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]
    assert abs(float(by_v[1 << 21][0]) - float(by_v[1 << 21][1])) <= 2.0 ** -23
    ws = _of(lines, "words")
    assert len(ws) == 35
    for d in ws:
        c, s = noise_ref.from_words(np.uint32(int(d["w1"])), np.uint32(int(d["w2"])))
        assert (int(d["c"], 16), int(d["s"], 16)) == (_bits(c), _bits(s)), d
        assert [int(x, 16) for x in d["one"].split(",")] == [_bits(c), _bits(s)], d


def test_elements_through_philox(lines):
    got = _of(lines, "elem")
    want = [(seed, k, e, a) for seed in (0, 1, 2 ** 64 - 1) for k in (0, 1, 2 ** 32 - 1) for e in (0, 129, 2 ** 32 - 1)
            for a in (0, 1, 2, 3, 4, 5, 6, 7, 13, 27)]
    assert [(int(d["seed"]), int(d["k"]), int(d["e"]), int(d["a"])) for d in got] == want
    for d, (seed, k, e, a) in zip(got, want):
        assert int(d["x"], 16) == _bits(noise_ref.element(seed, k, e, a)), d
    assert len({d["x"] for d in got}) > 260  # seeds, rows, envs and actions all reach the counter or the key


def test_rows_are_the_elements():
    """rows() draws a block per four actions; element() is the definition."""
    for A, row0, off in ((14, 0, 0), (27, 2 ** 32 - 3, 64), (1, 5, 2 ** 32 - 2)):
        got = noise_ref.rows(7, 3, 2, A, row0=row0, env_offset=off)
        assert got.shape == (3, 2, A) and got.dtype == np.float32
        for k in range(3):
            for n in range(2):
                want = noise_ref.element(7, row0 + k, (off + n) % 2 ** 32, np.arange(A))
                assert np.array_equal(got[k, n].view(np.uint32), want.view(np.uint32))


def test_accuracy_against_float64(sweeps):
    m = np.arange(1, N24 + 1, dtype=np.float64)
    r64 = np.sqrt(-2.0 * (np.log(m) - 24.0 * np.log(2.0)))
    e_r = float(np.abs(sweeps["radius"].astype(np.float64) - r64).max())
    th = np.arange(N24, dtype=np.float64) * (2.0 * np.pi / N24)
    e_s = float(np.abs(sweeps["sin"].astype(np.float64) - np.sin(th)).max())
    e_c = float(np.abs(sweeps["cos"].astype(np.float64) - np.cos(th)).max())
    e_t = max(e_s, e_c)
    print(f"e_r {e_r!r} ({e_r.hex()})  e_sin {e_s!r}  e_cos {e_c!r}  bound {e_r + noise_ref.R_MAX * e_t!r}")
    assert abs(e_r - E_R) <= E_SLACK and abs(e_t - E_T) <= E_SLACK
    assert float(sweeps["radius"].max()) <= noise_ref.R_MAX + E_R
    assert E_R + noise_ref.R_MAX * E_T <= 2.0 ** -18


N_DIST = 1 << 22
DIST_SHAPE = (32, 9363, 14)


def _corr(x, y):
    x = x.ravel().astype(np.float64)
    y = y.ravel().astype(np.float64)
    x = x - x.mean()
    y = y - y.mean()
    return float((x * y).sum() / np.sqrt((x * x).sum() * (y * y).sum()))


def _distribution(x):
    """The checks' statistics of a [K, N, A] normal sample: the moments and the Kolmogorov distance
    of its first 2^22 elements, the correlations of neighbours over all of it."""
    assert x.shape == DIST_SHAPE
    f = x.ravel()[:N_DIST].astype(np.float64)
    n = f.size
    mean = f.mean()
    d = f - mean
    var = (d * d).sum() / (n - 1)
    kurt = (d ** 4).mean() / ((d * d).mean() ** 2)
    cdf = ndtr(np.sort(f))
    i = np.arange(1, n + 1, dtype=np.float64)
    ks = max(float((i / n - cdf).max()), float((cdf - (i - 1) / n).max()))
    return {"mean": mean, "var": var, "kurtosis": kurt, "ks": ks,
            "corr_pair": _corr(x[:, :, 0::2], x[:, :, 1::2]), "corr_a": _corr(x[:, :, :-1], x[:, :, 1:]),
            "corr_n": _corr(x[:, :-1], x[:, 1:]), "corr_k": _corr(x[:-1], x[1:])}


def _check_distribution(st):
    n = float(N_DIST)
    print({k: float(v) for k, v in st.items()})
    assert abs(st["mean"]) <= 6.0 / np.sqrt(n)
    assert abs(st["var"] - 1.0) <= 6.0 * np.sqrt(2.0 / n)
    assert abs(st["kurtosis"] - 3.0) <= 6.0 * np.sqrt(24.0 / n)
    assert st["ks"] <= 1.95 / np.sqrt(n)
    for k in ("corr_pair", "corr_a", "corr_n", "corr_k"):
        assert abs(st[k]) <= 6.0 / np.sqrt(n), k


def test_distribution():
    K, N, A = DIST_SHAPE
    x = noise_ref.rows(0x5C6E015E, K, N, A)
    assert np.isfinite(x).all() and float(np.abs(x).max()) <= noise_ref.R_MAX
    _check_distribution(_distribution(x))


def test_numpys_normal_passes_the_same_checks():
    """The checks reject a generator, not the Gaussian."""
    x = np.random.default_rng(0).standard_normal(DIST_SHAPE).astype(np.float32)
    _check_distribution(_distribution(x))


def test_the_checks_reject_a_coarse_or_shifted_sample():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(DIST_SHAPE).astype(np.float32)
    with pytest.raises(AssertionError):
        _check_distribution(_distribution((x + np.float32(0.004)).astype(np.float32)))
    y = x.copy()
    y[:, :, 1::2] = (0.99 * y[:, :, 1::2] + 0.01 * y[:, :, 0::2]).astype(np.float32)  # a pair's members leak into each other
    with pytest.raises(AssertionError):
        _check_distribution(_distribution(y))
