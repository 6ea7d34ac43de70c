"""The BeerGame linear policy (csrc/scg_bg_policy.h) on the host: a stand-alone program with its
own main (tests/native/bg_policy_main.cpp), which includes that header alone and prints, for
L = 1, 4 and 8, the actions of a table of cases next to their inputs: negative pre-shift values
(floor, not truncation), values on each clamp bound and one past it, shifts 0 and 30, products
of 2^62 whose sum wraps, and the parameter-word index of every (l, j) at N = 3. The test
restates the formula in NumPy int64 (tests/bg_policy_ref.py) and compares; it also checks on
the expected side that each case shows what it is there for. No sanitizer: a plain program."""
import os
import subprocess

import numpy as np
import pytest

import bg_policy_ref
from conftest import PKG_ROOT, REPO

SRC = os.path.join(REPO, "tests", "native", "bg_policy_main.cpp")
OUT = os.path.join(REPO, "tests", "native", "_build", "bg_policy")
CSRC = os.path.join(PKG_ROOT, "csrc")
LEVELS = (1, 4, 8)
I32 = (-2 ** 31, 2 ** 31 - 1)


def build():
    deps = [SRC, os.path.join(REPO, "include", "scgpu.h"), os.path.join(CSRC, "scg_bg_policy.h")]
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    tmp = f"{OUT}.{os.getpid()}.tmp"  # concurrent test workers: build aside, rename into place
    subprocess.run(["hipcc", "-std=c++17", "-O1", "--offload-host-only", "-Wall", "-I", os.path.join(REPO, "include"),
                    "-I", CSRC, "-o", tmp, SRC], check=True)
    os.replace(tmp, OUT)
    return OUT


def _value(v):
    return np.array([int(x) for x in v.split(",")], dtype=np.int64) if "," in v else int(v)


@pytest.fixture(scope="module")
def cases():
    r = subprocess.run([build()], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for line in r.stdout.strip().splitlines():
        kind, *kv = line.split()
        out.append((kind, {k: _value(v) for k, v in (x.split("=") for x in kv)}))
    return out


def _of(cases, kind, L=None):
    return [c for k, c in cases if k == kind and (L is None or c["L"] == L)]


def _parts(c):
    """(W [L, L], b [L], o [L]) of a case line."""
    L = c["L"]
    p = np.atleast_1d(c["p"]).reshape(L, L + 1)
    return p[:, :L], p[:, L], np.atleast_1d(c["o"])


def _want(c):
    return bg_policy_ref.actions(*_parts(c), c["shift"], c["lo"], c["hi"])


def test_every_case_equals_the_numpy_restatement(cases):
    kinds = ("floor", "clamp", "shift0", "shift30")
    for L in LEVELS:
        assert [len(_of(cases, k, L)) for k in kinds] == [1, 4, 4, 2]
    for kind in kinds:
        for c in _of(cases, kind):
            assert np.array_equal(np.atleast_1d(c["a"]), _want(c)), (kind, c)
    assert {c["n"] for kind in kinds for c in _of(cases, kind)} == {0, 1, 2}  # every env column of the block


@pytest.mark.parametrize("L", LEVELS)
def test_negative_values_are_floored(cases, L):
    (c,) = _of(cases, "floor", L)
    z = bg_policy_ref.pre_shift(*_parts(c))
    assert c["shift"] > 0 and (z < 0).all() and (z % (1 << c["shift"]) != 0).all()
    floor, trunc = z >> c["shift"], -((-z) >> c["shift"])
    assert (floor == trunc - 1).all()
    assert np.array_equal(np.atleast_1d(c["a"]), floor)


@pytest.mark.parametrize("L", LEVELS)
def test_clamp_bounds_and_one_past(cases, L):
    seen = [set() for _ in range(L)]
    for c in _of(cases, "clamp", L):
        lo, hi = c["lo"], c["hi"]
        s = bg_policy_ref.pre_shift(*_parts(c)) >> c["shift"]
        for l in range(L):
            seen[l].add(int(s[l]))
        assert np.array_equal(np.atleast_1d(c["a"]), np.clip(s, lo, hi))
    assert all(v == {lo - 1, lo, hi, hi + 1} for v in seen), seen


@pytest.mark.parametrize("L", LEVELS)
def test_shift_0_and_30(cases, L):
    seen = [set() for _ in range(L)]
    for c in _of(cases, "shift0", L):
        assert c["shift"] == 0 and (c["lo"], c["hi"]) == I32
        z = bg_policy_ref.pre_shift(*_parts(c))
        for l in range(L):
            seen[l].add(int(z[l]))
    assert all(v == {I32[1], I32[1] + 1, I32[0], I32[0] - 1} for v in seen), seen
    wrapped = 0
    for c in _of(cases, "shift30", L):
        assert c["shift"] == 30
        W, b, o = _parts(c)
        exact = [int(b[l]) + sum(int(W[l, j]) * int(o[j]) for j in range(L)) for l in range(L)]  # Python ints
        assert max(abs(int(W[l, j]) * int(o[j])) for l in range(L) for j in range(L)) >= 2 ** 62 - 2 ** 31
        z = bg_policy_ref.pre_shift(W, b, o)
        assert [(e + 2 ** 63) % 2 ** 64 - 2 ** 63 for e in exact] == z.tolist()
        wrapped += sum(e != v for e, v in zip(exact, z.tolist()))
    assert (wrapped > 0) == (L > 1)  # one product of at most 2^62 and an int32 bias cannot leave int64


@pytest.mark.parametrize("L", LEVELS)
def test_parameter_word_index(cases, L):
    got = _of(cases, "index", L)
    assert {(c["n"], c["l"], c["j"]) for c in got} == {(n, l, j) for n in range(3) for l in range(L) for j in range(L + 1)}
    for c in got:
        assert c["word"] == c["l"] * (L + 1) + c["j"]
        assert c["at"] == c["word"] * 3 + c["n"] and c["loaded"] == c["at"]


def test_argument_check(cases):
    assert _of(cases, "valid") == [{"ok": 1}]
