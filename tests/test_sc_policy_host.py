"""The SupplyChain linear policy (csrc/scg_sc_policy.h) on the host: a stand-alone program with
its own main (tests/native/sc_policy_main.cpp), which includes that header alone and prints the
action rows of a table of cases next to the bits of their inputs: random rows of several
(A, O), O = 1, A = 1 and rows longer than a chunk of parameter loads included, in both
parameter layouts; rows on which both clamps bind; z = NaN, +inf and -inf; lo == hi; and the
word index of every (a, j) in both layouts. The test restates the formula as a NumPy float32
loop and compares the bits. The program is built with -fsanitize=address,undefined (a plain
executable; nothing here is loaded into Python)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO

SRC = os.path.join(REPO, "tests", "native", "sc_policy_main.cpp")
OUT = os.path.join(REPO, "tests", "native", "_build", "sc_policy")
CSRC = os.path.join(PKG_ROOT, "csrc")
SHAPES = [(14, 27), (3, 5), (1, 1), (1, 7), (5, 1), (2, 40), (14, 111)]


def build():
    deps = [SRC, os.path.join(REPO, "include", "scgpu.h"), os.path.join(CSRC, "scg_sc_policy.h")]
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
        floats = () if kind in ("index", "valid") else ("o", "p", "a", "lo", "hi")  # (an index line's a is an int)
        out.append((kind, {k: (_f32(v) if k in floats else int(v)) for k, v in d.items()}))
    return out


def _of(cases, kind):
    return [c for k, c in cases if k == kind]


def _pre_clamp(c):
    """z [A] of a case line: the formula's loop, every product and sum rounded to float32."""
    A, O = c["A"], c["O"]
    p = c["p"].reshape(A, O + 1)
    z = p[:, O].copy()
    with np.errstate(all="ignore"):
        for j in range(O):
            term = (p[:, j] * c["o"][j]).astype(np.float32)
            z = (z + term).astype(np.float32)
    return z


def _want(c):
    z, lo, hi = _pre_clamp(c), c["lo"][0], c["hi"][0]
    return np.array([lo if not zz >= lo else (hi if zz > hi else zz) for zz in z], dtype=np.float32)


def test_every_case_equals_the_numpy_loop(cases):
    n = 0
    for kind in ("random", "clamp", "equal", "narrow", "special"):
        for c in _of(cases, kind):
            assert c["chunks_differ"] == 0, (kind, c)
            assert c["p"].size == c["A"] * (c["O"] + 1) and c["a"].size == c["A"]
            assert np.array_equal(c["a"].view(np.uint32), _want(c).view(np.uint32)), (kind, c)
            n += 1
    assert n == 2 * 3 * 2 * len(SHAPES) + 2 * 4
    for kind in ("random", "clamp"):
        got = {(c["A"], c["O"], c["shared"]) for c in _of(cases, kind)}
        assert got == {(a, o, s) for a, o in SHAPES for s in (0, 1)}
        assert {c["n"] for c in _of(cases, kind) if not c["shared"]} == {0, 1, 2}  # every env column of the block


def test_the_sum_is_sequential_float32(cases):
    """The cases tell the formula's order and rounding from their neighbours: a float64 sum
    rounded once, or the same terms added in descending order, give other bits somewhere."""
    other64 = other_order = 0
    for c in _of(cases, "random"):
        A, O = c["A"], c["O"]
        p = c["p"].reshape(A, O + 1).astype(np.float64)
        z64 = (p[:, O] + (p[:, :O] * c["o"].astype(np.float64)).sum(axis=1)).astype(np.float32)
        p32 = c["p"].reshape(A, O + 1)
        zrev = p32[:, O].copy()
        for j in reversed(range(O)):
            zrev = (zrev + (p32[:, j] * c["o"][j]).astype(np.float32)).astype(np.float32)
        z = _pre_clamp(c)
        other64 += int((z64.view(np.uint32) != z.view(np.uint32)).sum())
        other_order += int((zrev.view(np.uint32) != z.view(np.uint32)).sum())
    assert other64 > 0 and other_order > 0


def test_both_clamps_bind_and_inside_values_pass(cases):
    below = above = inside = 0
    for c in _of(cases, "clamp") + _of(cases, "narrow"):
        z, lo, hi = _pre_clamp(c), c["lo"][0], c["hi"][0]
        below += int((z < lo).sum())
        above += int((z > hi).sum())
        inside += int(((z >= lo) & (z <= hi)).sum())
        assert ((c["a"] >= lo) & (c["a"] <= hi)).all()
    assert below > 20 and above > 20 and inside > 20
    for c in _of(cases, "equal"):
        assert c["lo"][0] == c["hi"][0] == np.float32(0.375) and (c["a"] == np.float32(0.375)).all()
    assert len(_of(cases, "equal")) == 2


def test_nan_and_infinities(cases):
    got = _of(cases, "special")
    assert len(got) == 4 and {c["shared"] for c in got} == {0, 1}
    for c in got:
        z, lo, hi = _pre_clamp(c), c["lo"][0], c["hi"][0]
        assert np.isnan(z[:3]).all() and z[3] == np.inf and z[4] == -np.inf and z[5] == np.inf and z[7] == -np.inf
        assert np.isfinite(z[6]) and z[6] > hi
        assert c["a"].tolist() == [lo, lo, lo, hi, lo, hi, hi, lo]  # NaN gives lo


def test_parameter_word_index_of_both_layouts(cases):
    got = _of(cases, "index")
    assert {(c["shared"], c["n"], c["a"], c["j"]) for c in got} == {(s, n, a, j) for s in (0, 1) for n in range(3)
                                                                 for a in range(3) for j in range(5)}
    for c in got:
        assert c["word"] == c["a"] * (c["O"] + 1) + c["j"]
        assert c["at"] == (c["word"] if c["shared"] else c["word"] * c["N"] + c["n"])


def test_argument_check(cases):
    assert _of(cases, "valid") == [{"ok": 1, "words": 14 * 28}]
