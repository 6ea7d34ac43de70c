"""The BeerGame local-information policy (csrc/scg_bg_local.h) on the host: a stand-alone program
with its own main (tests/native/bg_local_main.cpp), which includes that header alone and prints,
for L = 1, 4 and 8, the features and actions of a table of cases next to their inputs: negative
pre-shift values (floor, not truncation), values on each clamp bound and one past it, shifts 0
and 30, products of 2^62 whose sum wraps, a supply line that wraps; the parameter-word index of
every (l, j) at N = 3; and the live-row mask on delay lists with delay 0, colliding arrival
weeks, arrivals past T, d_0 > T, w0 = 0, w0 = T and a delay of exactly 64. The test restates all
of it in Python (tests/bg_local_ref.py) and compares; it also checks on the expected side that
each case shows what it is there for. No sanitizer: a plain program."""
import os
import subprocess

import numpy as np
import pytest

import bg_local_ref
from conftest import PKG_ROOT, REPO

SRC = os.path.join(REPO, "tests", "native", "bg_local_main.cpp")
OUT = os.path.join(REPO, "tests", "native", "_build", "bg_local")
CSRC = os.path.join(PKG_ROOT, "csrc")
LEVELS = (1, 4, 8)
I32 = (-2 ** 31, 2 ** 31 - 1)
KINDS = ("floor", "clamp", "shift0", "shift30", "wrapline")


def build():
    deps = [SRC, os.path.join(REPO, "include", "scgpu.h")] + \
        [os.path.join(CSRC, h) for h in ("scg_bg_local.h", "scg_bg_policy.h", "scg_bg_plan.h")]
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    tmp = f"{OUT}.{os.getpid()}.tmp"  # concurrent test workers: build aside, rename into place
    subprocess.run(["hipcc", "-std=c++17", "-O1", "--offload-host-only", "-Wall", "-I", os.path.join(REPO, "include"),
                    "-I", CSRC, "-o", tmp, SRC], check=True)
    os.replace(tmp, OUT)
    return OUT


def _value(v):
    if "," in v:
        return np.array([int(x) for x in v.split(",")], dtype=np.int64)
    return int(v) if v.lstrip("-").isdigit() else v


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
    """(W [L, 4], b [L], f [L, 4]) of a case line, the features restated from its inputs."""
    L = c["L"]
    p = np.atleast_1d(c["p"]).reshape(L, 5)
    f = bg_local_ref.features_from(*(np.atleast_1d(c[k]) for k in ("net", "bk", "op", "tr")), c["d"])
    return p[:, :4], p[:, 4], f


def _want(c):
    return bg_local_ref.actions(*_parts(c), c["shift"], c["lo"], c["hi"])


def test_every_case_equals_the_restatement(cases):
    for L in LEVELS:
        assert [len(_of(cases, k, L)) for k in KINDS] == [1, 4, 4, 2, 1]
    for kind in KINDS:
        for c in _of(cases, kind):
            assert np.array_equal(np.atleast_1d(c["f"]).reshape(c["L"], 4), _parts(c)[2]), (kind, c)
            assert np.array_equal(np.atleast_1d(c["a"]), _want(c)), (kind, c)
    assert {c["n"] for kind in KINDS for c in _of(cases, kind)} == {0, 1, 2}  # every env column of the block


@pytest.mark.parametrize("L", LEVELS)
def test_features_are_the_table(cases, L):
    """On the small state every term of `line` is non-zero where the level has it, and each
    feature is the table's entry, written out here term by term."""
    (c,) = _of(cases, "floor", L)
    net, bk, op, tr = (np.atleast_1d(c[k]) for k in ("net", "bk", "op", "tr"))
    f = np.atleast_1d(c["f"]).reshape(L, 4)
    assert (op != 0).all() and (tr != 0).all() and (bk[1:] != 0).all()
    for l in range(L):
        assert f[l, 0] == net[l]
        assert f[l, 1] == op[l] + (bk[l + 1] if l + 1 < L else 0) + tr[l]
        assert f[l, 2] == (op[l - 1] if l else c["d"])
        assert f[l, 3] == op[l]


@pytest.mark.parametrize("L", LEVELS)
def test_negative_values_are_floored(cases, L):
    (c,) = _of(cases, "floor", L)
    z = bg_local_ref.pre_shift(*_parts(c))
    assert c["shift"] > 0 and (z < 0).all() and (z % (1 << c["shift"]) != 0).all()
    floor, trunc = z >> c["shift"], -((-z) >> c["shift"])
    assert (floor == trunc - 1).all()
    assert np.array_equal(np.atleast_1d(c["a"]), floor)


@pytest.mark.parametrize("L", LEVELS)
def test_clamp_bounds_and_one_past(cases, L):
    seen = [set() for _ in range(L)]
    for c in _of(cases, "clamp", L):
        lo, hi = c["lo"], c["hi"]
        s = bg_local_ref.pre_shift(*_parts(c)) >> c["shift"]
        for l in range(L):
            seen[l].add(int(s[l]))
        assert np.array_equal(np.atleast_1d(c["a"]), np.clip(s, lo, hi))
    assert all(v == {lo - 1, lo, hi, hi + 1} for v in seen), seen


@pytest.mark.parametrize("L", LEVELS)
def test_shift_0_and_30(cases, L):
    seen = [set() for _ in range(L)]
    for c in _of(cases, "shift0", L):
        assert c["shift"] == 0 and (c["lo"], c["hi"]) == I32
        z = bg_local_ref.pre_shift(*_parts(c))
        for l in range(L):
            seen[l].add(int(z[l]))
    assert all(v == {I32[1], I32[1] + 1, I32[0], I32[0] - 1} for v in seen), seen
    wrapped = 0
    for c in _of(cases, "shift30", L):
        assert c["shift"] == 30
        W, b, f = _parts(c)
        assert (f == I32[0]).all()
        exact = [int(b[l]) + sum(int(W[l, j]) * int(f[l, j]) for j in range(4)) for l in range(L)]  # Python ints
        assert max(abs(int(W[l, j]) * int(f[l, j])) for l in range(L) for j in range(4)) >= 2 ** 62 - 2 ** 31
        z = bg_local_ref.pre_shift(W, b, f)
        assert [(e + 2 ** 63) % 2 ** 64 - 2 ** 63 for e in exact] == z.tolist()
        wrapped += sum(e != v for e, v in zip(exact, z.tolist()))
    assert (wrapped > 0) == (L > 1)  # level 0 has one product of at most 2^62: with an int32 bias it stays in int64


@pytest.mark.parametrize("L", LEVELS)
def test_the_supply_line_wraps_in_int32(cases, L):
    (c,) = _of(cases, "wrapline", L)
    op, bk, tr = (np.atleast_1d(c[k]) for k in ("op", "bk", "tr"))
    exact = op + np.append(bk[1:], 0) + tr
    assert (exact > I32[1]).all()
    assert np.array_equal(np.atleast_1d(c["a"]), exact - 2 ** 32)  # weight 1 on `line`, shift 0, no clamp


@pytest.mark.parametrize("L", LEVELS)
def test_parameter_word_index(cases, L):
    got = _of(cases, "index", L)
    assert {(c["n"], c["l"], c["j"]) for c in got} == {(n, l, j) for n in range(3) for l in range(L) for j in range(5)}
    for c in got:
        assert c["word"] == c["l"] * 5 + c["j"] == bg_local_ref.word(c["l"], c["j"])
        assert c["at"] == c["word"] * 3 + c["n"] and c["loaded"] == c["at"]


def test_live_mask_of_delay_lists(cases):
    got = _of(cases, "mask")
    names = {c["name"] for c in got}
    assert names == {"list", "d0-past-T", "all-zero", "delay-64"}
    for c in got:
        d, T, w0 = [int(x) for x in c["delays"]], c["T"], c["w0"]
        assert len(d) == T + 1
        assert c["live"] == bg_local_ref.live_mask(d, T, w0), c
    by = {name: [c for c in got if c["name"] == name] for name in names}
    for name, rows in by.items():
        assert [c["w0"] for c in rows] == list(range(rows[0]["T"] + 1))  # w0 = 0 .. T
        assert rows[-1]["live"] == 0                                      # nothing arrives after week T
    lst = [int(x) for x in by["list"][0]["delays"]]
    T = by["list"][0]["T"]
    arrivals = [w + lst[w] for w in range(1, T + 1) if lst[w] > 0]
    assert 0 in lst[1:] and len(set(arrivals)) < len(arrivals) and max(arrivals) > T   # delay 0, collisions, past T
    assert by["list"][0]["live"] == 0b11                                  # just reset: the initial pipeline
    assert by["list"][5]["live"] == 0b1 and by["list"][3]["live"] == 0b100  # weeks 3 and 5 ship into week 6, once
    d0 = by["d0-past-T"][0]
    assert int(d0["delays"][0]) > d0["T"] and d0["live"] == (1 << d0["T"]) - 1   # the pipeline stops at T
    assert all(c["live"] == 0 for c in by["all-zero"])
    d64 = by["delay-64"]
    assert d64[0]["live"] == 2 ** 64 - 1                                  # d_0 = 64: all 64 bits
    assert d64[3]["live"] >> 63 == 1 and d64[2]["live"] >> 63 == 0         # week 3 ships 64 weeks ahead
    assert d64[36]["live"] >> 63 == 1 and d64[37]["live"] >> 62 == 1       # week 36 arrives in week T = 100 ...
    assert d64[37]["live"] >> 63 == 0                                      # ... week 37 a week past it: dropped


def test_live_mask_with_stochastic_delays(cases):
    got = _of(cases, "smask")
    assert len(got) == 4 * 3 * 5
    for c in got:
        R, T, w0 = c["R"], c["T"], c["w0"]
        assert c["live"] == bg_local_ref.live_mask_stochastic(R, T, w0) == (1 << min(R - 1, T - w0)) - 1, c
    assert any(c["live"] == 2 ** 64 - 1 for c in got)


def test_argument_check(cases):
    assert _of(cases, "valid") == [{"ok": 1}]
