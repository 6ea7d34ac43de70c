"""The sampled SupplyChain policies (csrc/scg_sc_policy.h, csrc/scg_sc_mlp.h) on the host: a
stand-alone program with its own main (tests/native/sc_sampled_main.cpp), which includes those
headers alone and prints u and the action of a table of cases next to the bits of their inputs:
random rows of the linear policy and the MLP in both parameter layouts, with the noise read at
(k, n, a) of a [K][N][A] block; std = 0; lo == hi; noise of +inf, -inf and NaN, 0 * inf, a NaN
std; noise that only just binds each clamp. The test restates the formula,

    u = z + (std * eps)       the product rounded to float32, then the sum
    action = lo if not u >= lo else (hi if u > hi else u)

as a NumPy float32 loop and compares the bits. The program is built with
-fsanitize=address,undefined as tests/test_sc_policy_host.py builds its own (a plain
executable; nothing here is loaded into Python)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO

SRC = os.path.join(REPO, "tests", "native", "sc_sampled_main.cpp")
OUT = os.path.join(REPO, "tests", "native", "_build", "sc_sampled")
CSRC = os.path.join(PKG_ROOT, "csrc")
SHAPES = [(14, 27, 0), (14, 27, 16), (1, 1, 0), (3, 5, 2), (2, 40, 0), (5, 40, 33)]


def build():
    deps = [SRC, os.path.join(REPO, "include", "scgpu.h"), os.path.join(CSRC, "scg_sc_policy.h"),
            os.path.join(CSRC, "scg_sc_mlp.h")]
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    tmp = f"{OUT}.{os.getpid()}.tmp"  # concurrent test workers: build aside, rename into place
    subprocess.run(["hipcc", "-std=c++17", "-O1", "-g", "--offload-host-only", "-Wall", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I", os.path.join(REPO, "include"), "-I", CSRC, "-o", tmp, SRC], check=True)
    os.replace(tmp, OUT)
    return OUT


def _f32(v):
    return np.array([int(x, 16) for x in v.split(",")], dtype=np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def cases():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([build()], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    out = []
    for line in r.stdout.strip().splitlines():
        kind, *kv = line.split()
        d = dict(x.split("=") for x in kv)
        if kind == "index":
            out.append((kind, {"at": [int(x) for x in d["at"].split(",")]}))
            continue
        floats = ("o", "p", "s", "e", "u", "a", "lo", "hi")
        out.append((kind, {k: (_f32(v) if k in floats else int(v)) for k, v in d.items()}))
    return out


def _of(cases, kind):
    return [c for k, c in cases if k == kind]


def _row_sums(rows, x):
    """z [R] = bias, then + rows[:, j] * x[j] in ascending j, every product and sum rounded to float32."""
    n = rows.shape[1] - 1
    z = rows[:, n].copy()
    with np.errstate(all="ignore"):
        for j in range(n):
            z = (z + (rows[:, j] * x[j]).astype(np.float32)).astype(np.float32)
    return z


def _z(c):
    A, O, H = c["A"], c["O"], c["H"]
    p = c["p"]
    if H == 0:
        assert p.size == A * (O + 1)
        return _row_sums(p.reshape(A, O + 1), c["o"])
    assert p.size == H * (O + 1) + A * (H + 1)
    pre = _row_sums(p[:H * (O + 1)].reshape(H, O + 1), c["o"])
    hid = np.array([x if x > 0 else np.float32(0.0) for x in pre], dtype=np.float32)
    return _row_sums(p[H * (O + 1):].reshape(A, H + 1), hid)


def _want(c):
    z = _z(c)
    lo, hi = c["lo"][0], c["hi"][0]
    with np.errstate(all="ignore"):
        u = (z + (c["s"] * c["e"]).astype(np.float32)).astype(np.float32)
    return u, np.array([lo if not x >= lo else (hi if x > hi else x) for x in u], dtype=np.float32)


KINDS = ("random", "clamp", "std0", "equal", "special", "edge")


def test_every_case_equals_the_numpy_loop(cases):
    n = 0
    for kind in KINDS:
        for c in _of(cases, kind):
            assert c["differ"] == 0, (kind, c)  # every chunk size agrees; std 0 with noise 0 is the deterministic action
            u, act = _want(c)
            assert np.array_equal(c["u"].view(np.uint32), u.view(np.uint32)), (kind, c)
            assert np.array_equal(c["a"].view(np.uint32), act.view(np.uint32)), (kind, c)
            n += 1
    assert n == 2 * 3 * 2 * len(SHAPES) + 2 * 2 * 5
    for kind in ("random", "clamp"):
        got = {(c["A"], c["O"], c["H"], c["shared"]) for c in _of(cases, kind)}
        assert got == {(a, o, h, s) for a, o, h in SHAPES for s in (0, 1)}
        assert {c["n"] for c in _of(cases, kind)} == {0, 1, 2} and {c["k"] for c in _of(cases, kind)} == {0, 1}


def test_the_product_is_rounded_before_the_sum(cases):
    """A fused multiply-add, or the sum in float64 rounded once, gives other bits somewhere."""
    other = 0
    for c in _of(cases, "random") + _of(cases, "clamp"):
        z = _z(c)
        fused = (z.astype(np.float64) + c["s"].astype(np.float64) * c["e"].astype(np.float64)).astype(np.float32)
        other += int((fused.view(np.uint32) != c["u"].view(np.uint32)).sum())
    assert other > 0


def test_both_clamps_bind_and_the_noise_moves_actions_across_them(cases):
    below = above = inside = crossed = 0
    for c in _of(cases, "random") + _of(cases, "clamp"):
        z = _z(c)
        u = c["u"]
        lo, hi = c["lo"][0], c["hi"][0]
        below += int((u < lo).sum())
        above += int((u > hi).sum())
        inside += int(((u >= lo) & (u <= hi)).sum())
        crossed += int((((z >= lo) & (z <= hi)) != ((u >= lo) & (u <= hi))).sum())  # the clamp is taken of u, not of z
        assert ((c["a"] >= lo) & (c["a"] <= hi)).all()
    assert below > 20 and above > 20 and inside > 20 and crossed > 20


def test_std_zero_equal_bounds_and_the_edges(cases):
    got = _of(cases, "std0")
    assert len(got) == 4 and {(c["shared"], c["H"]) for c in got} == {(0, 0), (0, 5), (1, 0), (1, 5)}
    for c in got:
        assert (c["s"] == 0).all() and (c["e"] != 0).any()
        assert np.array_equal(c["u"], _z(c))  # compares equal: a -0 z would come out +0
    for c in _of(cases, "equal"):
        assert c["lo"][0] == c["hi"][0] == np.float32(0.375) and (c["a"] == np.float32(0.375)).all()
    got = _of(cases, "edge")
    assert len(got) == 4
    for c in got:  # z = 0, std = 1: u is the noise; +-1 stay, one ulp beyond is clamped to the same value
        assert (_z(c) == 0).all()
        assert c["u"].view(np.uint32).tolist() == c["e"].view(np.uint32).tolist()
        assert c["a"].tolist() == [1.0, 1.0, -1.0, -1.0] and c["u"][1] > 1.0 and c["u"][3] < -1.0


def test_infinite_and_nan_noise(cases):
    got = _of(cases, "special")
    assert len(got) == 8 and {c["shared"] for c in got} == {0, 1} and {c["H"] for c in got} == {0, 5}
    for c in got:
        lo, hi = c["lo"][0], c["hi"][0]
        u = c["u"]
        assert u[0] == np.inf and u[1] == -np.inf and np.isnan(u[2:]).all()  # 0 * inf and a NaN std are NaN
        assert c["a"].tolist() == [hi, lo, lo, lo, lo, lo]                   # a NaN u gives lo


def test_sample_index(cases):
    assert _of(cases, "index") == [{"at": [0, (2 * 130 + 129) * 14 + 13, (4095 * 65536 + 65535) * 14 + 13]}]
    assert (4095 * 65536 + 65535) * 14 + 13 > 2 ** 31  # a 64-bit index
