"""The BeerGame float32 MLP policy (csrc/scg_bg_mlp.h) on the host: a stand-alone program with its
own main (tests/native/bg_mlp_main.cpp), which includes that header alone, is built with
-ffp-contract=off and prints, for L = 1, 4 and 8, a table of cases with every float as its bit
pattern: ties at k + 0.5 on both parities, u on each bound and one ulp inside it, +-inf and NaN, a
-0 pre-activation, features above 2^24, a sample whose product must be rounded before the add,
H = 1, 3, 16 and 64 with general parameters, and every word index at H = 3. The test restates the
table in NumPy float32 (tests/bg_mlp_ref.py) and compares bits; it also checks on the expected
side that each case shows what it is there for. No sanitizer: a plain program."""
import os
import subprocess

import numpy as np
import pytest

import bg_mlp_ref
from conftest import PKG_ROOT, REPO

SRC = os.path.join(REPO, "tests", "native", "bg_mlp_main.cpp")
OUT = os.path.join(REPO, "tests", "native", "_build", "bg_mlp")
CSRC = os.path.join(PKG_ROOT, "csrc")
LEVELS = (1, 4, 8)
KINDS = {"tie": 8, "bound": 8, "special": 4, "negzero": 1, "big": 4, "product": 1, "h1": 1, "h64": 1, "h3": 1,
         "order": 1, "sampled": 1}
F32 = np.float32


def build():
    deps = [SRC, os.path.join(REPO, "include", "scgpu.h")] + \
        [os.path.join(CSRC, h) for h in ("scg_bg_mlp.h", "scg_bg_local.h", "scg_bg_policy.h", "scg_bg_plan.h")]
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    tmp = f"{OUT}.{os.getpid()}.tmp"  # concurrent test workers: build aside, rename into place
    subprocess.run(["hipcc", "-std=c++17", "-O1", "-ffp-contract=off", "--offload-host-only", "-Wall", "-I",
                    os.path.join(REPO, "include"), "-I", CSRC, "-o", tmp, SRC], check=True)
    os.replace(tmp, OUT)
    return OUT


def _floats(v):
    return np.array([int(x, 16) for x in v.split(",")], dtype=np.uint32).view(F32)


def _value(k, v):
    if k in ("p", "std", "eps", "u"):
        return _floats(v)
    if k in ("f", "a"):
        return np.array([int(x) for x in v.split(",")], dtype=np.int64)
    return int(v)


@pytest.fixture(scope="module")
def cases():
    r = subprocess.run([build()], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for line in r.stdout.strip().splitlines():
        kind, *kv = line.split()
        out.append((kind, {k: _value(k, v) for k, v in (x.split("=") for x in kv)}))
    return out


def _of(cases, kind, L=None):
    return [c for k, c in cases if k == kind and (L is None or c["L"] == L)]


def _unpack(c):
    """(w1 [H, 4L], b1 [H], w2 [L, H], b2 [L]) out of the case's words, by the reference's word()."""
    L, H, p = c["L"], c["H"], c["p"]
    assert len(p) == bg_mlp_ref.n_words(L, H)
    w1 = np.array([[p[bg_mlp_ref.word(L, H, 0, i, j)] for j in range(4 * L)] for i in range(H)], dtype=F32)
    b1 = np.array([p[bg_mlp_ref.word(L, H, 0, i, 4 * L)] for i in range(H)], dtype=F32)
    w2 = np.array([[p[bg_mlp_ref.word(L, H, 1, a, i)] for i in range(H)] for a in range(L)], dtype=F32)
    b2 = np.array([p[bg_mlp_ref.word(L, H, 1, a, H)] for a in range(L)], dtype=F32)
    return w1, b1, w2, b2


def _z(c):
    return bg_mlp_ref.z_values(*_unpack(c), bg_mlp_ref.inputs(c["f"].reshape(c["L"], 4)))


def _want(c):
    z = _z(c)
    u = bg_mlp_ref.sample(z, c["std"], c["eps"]) if c["sampled"] else z
    return u, bg_mlp_ref.finish(u, c["lo"], c["hi"])


def _bits(x):
    return np.asarray(x, dtype=F32).view(np.uint32)


def test_every_case_equals_the_restatement(cases):
    for L in LEVELS:
        assert {k: len(_of(cases, k, L)) for k in KINDS} == KINDS
    for kind in KINDS:
        for c in _of(cases, kind):
            u, a = _want(c)
            assert np.array_equal(_bits(c["u"]), _bits(u)), (kind, c)
            assert np.array_equal(c["a"], a), (kind, c)


@pytest.mark.parametrize("L", LEVELS)
def test_ties_round_to_even_on_both_parities(cases, L):
    seen = [set() for _ in range(L)]
    for c in _of(cases, "tie", L):
        u = c["u"].astype(np.float64)
        assert (np.abs(u - np.floor(u) - 0.5) == 0).all() and (c["lo"] < u).all() and (u < c["hi"]).all()
        assert (c["a"] % 2 == 0).all() and (np.abs(c["a"] - u) == 0.5).all()
        for a in range(L):
            seen[a].add(int(np.floor(u[a])) % 2)
    assert all(s == {0, 1} for s in seen)


@pytest.mark.parametrize("L", LEVELS)
def test_bounds_and_one_ulp_inside(cases, L):
    got = _of(cases, "bound", L)
    assert {(c["lo"], c["hi"]) for c in got} == {(-5, 7), (-2 ** 24, 2 ** 24)}
    for lo, hi in ((-5, 7), (-2 ** 24, 2 ** 24)):
        seen = [set() for _ in range(L)]
        inside = (np.nextafter(F32(lo), F32(np.inf)), np.nextafter(F32(hi), F32(-np.inf)))
        for c in (c for c in got if c["lo"] == lo):
            for a in range(L):
                u = c["u"][a]
                seen[a].add(float(u))
                want = lo if u == F32(lo) else hi if u == F32(hi) else int(np.rint(u))
                assert c["a"][a] == want
        assert all(s == {float(lo), float(hi), float(inside[0]), float(inside[1])} for s in seen), seen
    wide = [c for c in got if c["hi"] == 2 ** 24]
    assert {int(a) for c in wide for a in c["a"]} == {-2 ** 24, -2 ** 24 + 1, 2 ** 24 - 1, 2 ** 24}


@pytest.mark.parametrize("L", LEVELS)
def test_infinities_and_nan(cases, L):
    seen = set()
    for c in _of(cases, "special", L):
        for u, a in zip(c["u"], c["a"]):
            seen.add("nan" if np.isnan(u) else float(u))
            assert a == (c["hi"] if u > 0 else c["lo"])   # NaN > 0 is false: lo
    assert seen == {"nan", float("inf"), float("-inf"), float(F32(3.0e38))}


@pytest.mark.parametrize("L", LEVELS)
def test_a_negative_zero_pre_activation_gives_positive_zero(cases, L):
    (c,) = _of(cases, "negzero", L)
    w1, b1, w2, b2 = _unpack(c)
    x = bg_mlp_ref.inputs(c["f"].reshape(L, 4))
    assert (x > 0).all() and (_bits(w1) == 0x80000000).all() and (_bits(b1) == 0x80000000).all()
    assert (_bits(bg_mlp_ref.hidden(w1, b1, x)) == 0).all()             # +0 after the ReLU
    assert (_bits(c["u"]) == 0x80000000).all() and (c["a"] == 0).all()   # -0 + (-1 * +0) = -0; kept -0 would give +0


@pytest.mark.parametrize("L", LEVELS)
def test_features_above_2_pow_24_round_to_even(cases, L):
    big = set()
    for c in _of(cases, "big", L):
        f = c["f"]
        (q,) = np.nonzero(np.abs(f) > 2 ** 24)[0]
        big.add(int(f[q]))
        x = abs(float(F32(np.int32(f[q]))))   # the case's weight on it is its sign
        assert np.array_equal(c["u"].astype(np.float64), [(-1) ** a * x / 256 for a in range(L)])
    assert big == {2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 1, -2 ** 31}
    assert float(F32(np.int32(2 ** 24 + 1))) == 2 ** 24 and float(F32(np.int32(2 ** 24 + 3))) == 2 ** 24 + 4


@pytest.mark.parametrize("L", LEVELS)
def test_the_samples_product_is_rounded_before_the_add(cases, L):
    (c,) = _of(cases, "product", L)
    assert c["sampled"] == 1
    z, s, e = _z(c).astype(np.float64), c["std"].astype(np.float64), c["eps"].astype(np.float64)
    assert ((z + s * e) != 0).all()            # the exact sum, what a fused multiply-add rounds: 2^-24
    assert (_bits(c["u"]) == 0).all()           # the rounded product cancels z exactly


@pytest.mark.parametrize("L", LEVELS)
def test_hidden_widths_and_the_summation_order(cases, L):
    for kind, H in (("h1", 1), ("h64", 64), ("h3", 3), ("order", 16), ("sampled", 16)):
        (c,) = _of(cases, kind, L)
        assert c["H"] == H and len(set(_bits(c["p"]).tolist())) > len(c["p"]) // 2   # general words, not a pattern
        hid = bg_mlp_ref.hidden(*_unpack(c)[:2], bg_mlp_ref.inputs(c["f"].reshape(L, 4)))
        if H >= 16:
            assert (hid == 0).any() and (hid > 0).any()
    (c,) = _of(cases, "order", L)
    once = bg_mlp_ref.one_expression(*_unpack(c), bg_mlp_ref.inputs(c["f"].reshape(L, 4)))
    if L > 1:   # (one level may agree by chance)
        assert (_bits(once) != _bits(c["u"])).any()   # float32 step by step differs from float64 rounded once
    (c,) = _of(cases, "sampled", L)
    assert c["sampled"] == 1 and (c["std"] > 0).all() and (c["eps"] != 0).all()
    assert (_bits(c["u"]) != _bits(_z(c))).all()


@pytest.mark.parametrize("L", LEVELS)
def test_every_word_index_at_h3(cases, L):
    got = [c for c in _of(cases, "index", L)]
    H, I = 3, 4 * L
    want = {(0, i, j) for i in range(H) for j in range(I + 1)} | {(1, a, i) for a in range(L) for i in range(H + 1)}
    assert {(c["layer"], c["r"], c["k"]) for c in got} == want
    for c in got:
        assert c["H"] == 3
        assert c["word"] == bg_mlp_ref.word(L, H, c["layer"], c["r"], c["k"])
        assert c["word"] == (c["r"] * (I + 1) + c["k"] if c["layer"] == 0 else H * (I + 1) + c["r"] * (H + 1) + c["k"])
    assert sorted(c["word"] for c in got) == list(range(bg_mlp_ref.n_words(L, H)))   # a bijection onto 0..Q-1
    (w,) = _of(cases, "words", L)
    assert (w["q"], w["q64"]) == (bg_mlp_ref.n_words(L, 3), bg_mlp_ref.n_words(L, 64))


def test_argument_check(cases):
    assert _of(cases, "valid") == [{"ok": 1}]
