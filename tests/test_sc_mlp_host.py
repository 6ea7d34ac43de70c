"""The SupplyChain one-hidden-layer ReLU policy (csrc/scg_sc_mlp.h) on the host: a stand-alone
program with its own main (tests/native/sc_mlp_main.cpp), which includes that header alone and
prints the hidden and action rows of a table of cases next to the bits of their inputs: random
rows of several (A, O, H) — (1, 1, 1), rows longer than a chunk of parameter loads in both
layers, H = 64 — in both parameter layouts; rows on which both clamps bind; lo == hi; a hidden
layer wholly negative; NaN, -0 and infinite pre-activations; and the word index of every
(layer, row, column) in both layouts. The test restates the formula as a NumPy float32 loop and
compares the bits. The program is built with -fsanitize=address,undefined (a plain executable;
nothing here is loaded into Python)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO

SRC = os.path.join(REPO, "tests", "native", "sc_mlp_main.cpp")
OUT = os.path.join(REPO, "tests", "native", "_build", "sc_mlp")
CSRC = os.path.join(PKG_ROOT, "csrc")
SHAPES = [(14, 27, 16), (1, 1, 1), (3, 5, 2), (2, 40, 33), (14, 27, 64)]


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
        floats = () if kind in ("index", "valid") else ("o", "p", "h", "a", "lo", "hi")
        out.append((kind, {k: (_f32(v) if k in floats else int(v)) for k, v in d.items()}))
    return out


def _of(cases, kind):
    return [c for k, c in cases if k == kind]


def _layers(c):
    A, O, H = c["A"], c["O"], c["H"]
    p = c["p"]
    assert p.size == H * (O + 1) + A * (H + 1)
    return p[:H * (O + 1)].reshape(H, O + 1), p[H * (O + 1):].reshape(A, H + 1)


def _row_sums(rows, x):
    """z [R] = bias, then + rows[:, j] * x[j] in ascending j, every product and sum rounded to float32."""
    n = rows.shape[1] - 1
    z = rows[:, n].copy()
    with np.errstate(all="ignore"):
        for j in range(n):
            z = (z + (rows[:, j] * x[j]).astype(np.float32)).astype(np.float32)
    return z


def _pre(c):
    """(hidden pre-activations, hidden units, z) of a case line by the formula."""
    l1, l2 = _layers(c)
    pre = _row_sums(l1, c["o"])
    hid = np.array([x if x > 0 else np.float32(0.0) for x in pre], dtype=np.float32)
    return pre, hid, _row_sums(l2, hid)


def _want(c):
    _, hid, z = _pre(c)
    lo, hi = c["lo"][0], c["hi"][0]
    return hid, np.array([lo if not zz >= lo else (hi if zz > hi else zz) for zz in z], dtype=np.float32)


KINDS = ("random", "clamp", "equal", "narrow", "negative", "zeros", "infs")


def test_every_case_equals_the_numpy_loop(cases):
    n = 0
    for kind in KINDS:
        for c in _of(cases, kind):
            assert c["chunks_differ"] == 0, (kind, c)
            hid, act = _want(c)
            assert np.array_equal(c["h"].view(np.uint32), hid.view(np.uint32)), (kind, c)
            assert np.array_equal(c["a"].view(np.uint32), act.view(np.uint32)), (kind, c)
            n += 1
    assert n == 2 * 3 * 2 * len(SHAPES) + 2 * 7
    for kind in ("random", "clamp"):
        got = {(c["A"], c["O"], c["H"], c["shared"]) for c in _of(cases, kind)}
        assert got == {(a, o, h, s) for a, o, h in SHAPES for s in (0, 1)}
        assert {c["n"] for c in _of(cases, kind) if not c["shared"]} == {0, 1, 2}  # every env column of the block


def test_the_sums_are_sequential_float32(cases):
    """A float64 sum rounded once, or a fused multiply-add, gives other bits somewhere."""
    other64 = 0
    for c in _of(cases, "random"):
        l1, l2 = _layers(c)
        pre, hid, z = _pre(c)
        pre64 = (l1[:, -1].astype(np.float64) + (l1[:, :-1].astype(np.float64) * c["o"]).sum(axis=1)).astype(np.float32)
        z64 = (l2[:, -1].astype(np.float64) + (l2[:, :-1].astype(np.float64) * hid).sum(axis=1)).astype(np.float32)
        other64 += int((pre64.view(np.uint32) != pre.view(np.uint32)).sum() + (z64.view(np.uint32) != z.view(np.uint32)).sum())
    assert other64 > 0


def test_relu_and_both_clamps(cases):
    below = above = inside = zero = positive = 0
    for c in _of(cases, "random") + _of(cases, "clamp") + _of(cases, "narrow"):
        pre, hid, z = _pre(c)
        lo, hi = c["lo"][0], c["hi"][0]
        below += int((z < lo).sum())
        above += int((z > hi).sum())
        inside += int(((z >= lo) & (z <= hi)).sum())
        zero += int((pre <= 0).sum())
        positive += int((pre > 0).sum())
        assert ((c["a"] >= lo) & (c["a"] <= hi)).all() and (c["h"] >= 0).all()
        assert not np.signbit(c["h"]).any()
    assert below > 20 and above > 20 and inside > 20 and zero > 100 and positive > 100
    for c in _of(cases, "equal"):
        assert c["lo"][0] == c["hi"][0] == np.float32(0.375) and (c["a"] == np.float32(0.375)).all()
    assert len(_of(cases, "equal")) == 2


def test_a_wholly_negative_hidden_layer_gives_the_clamped_output_bias(cases):
    got = _of(cases, "negative")
    assert len(got) == 2 and {c["shared"] for c in got} == {0, 1}
    for c in got:
        pre, _, _ = _pre(c)
        assert (pre < 0).all() and (c["h"].view(np.uint32) == 0).all()
        assert c["a"].tolist() == [-1.0, -0.25, 0.0, 0.75, 1.0]


def test_nan_negative_zero_and_infinities(cases):
    got = _of(cases, "zeros")
    assert len(got) == 4 and {c["shared"] for c in got} == {0, 1}
    for c in got:  # NaN, -0 and -inf pre-activations give +0
        pre, hid, z = _pre(c)
        hi = c["hi"][0]
        assert np.isnan(pre[:3]).all() and pre[3] == 0 and np.signbit(pre[3]) and pre[4] == -np.inf
        assert pre[5] == np.float32(0.75)
        assert c["h"].view(np.uint32)[:5].tolist() == [0] * 5 and c["h"][5] == np.float32(0.75)
        assert z.tolist() == [0.125, 0.5] and c["a"].tolist() == [min(np.float32(0.125), hi), min(np.float32(0.5), hi)]
    got = _of(cases, "infs")
    assert len(got) == 4 and {c["shared"] for c in got} == {0, 1}
    for c in got:  # +inf hidden units: z inf, -inf or NaN; a NaN z gives lo
        pre, hid, z = _pre(c)
        lo, hi = c["lo"][0], c["hi"][0]
        assert c["h"][0] == np.inf and c["h"][1] == np.inf and c["h"][2] == np.float32(0.5)
        assert z[0] == np.inf and z[1] == -np.inf and np.isnan(z[2:]).all()
        assert c["a"].tolist() == [hi, lo, lo, lo, lo]


def test_parameter_word_index_of_both_layouts(cases):
    got = _of(cases, "index")
    A, O, H = 3, 4, 2
    want = {(s, n, 0, r, k) for s in (0, 1) for n in range(3) for r in range(H) for k in range(O + 1)} | \
           {(s, n, 1, r, k) for s in (0, 1) for n in range(3) for r in range(A) for k in range(H + 1)}
    assert {(c["shared"], c["n"], c["layer"], c["r"], c["k"]) for c in got} == want
    for c in got:
        assert (c["A"], c["O"], c["H"]) == (A, O, H)
        word = c["r"] * (O + 1) + c["k"] if c["layer"] == 0 else H * (O + 1) + c["r"] * (H + 1) + c["k"]
        assert c["word"] == word
        assert c["at"] == (word if c["shared"] else word * c["N"] + c["n"])
    assert sorted({c["word"] for c in got}) == list(range(H * (O + 1) + A * (H + 1)))


def test_argument_check(cases):
    assert _of(cases, "valid") == [{"ok": 1, "words": 16 * 28 + 14 * 17, "fused_max": 40}]
