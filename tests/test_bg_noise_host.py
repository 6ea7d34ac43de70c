"""The noise row a BeerGame lane computes for itself (csrc/scg_normal.h bg_noise_row<L>) on the
host, against the NumPy statement of the noise (tests/noise_ref.py rows).

A stand-alone program with its own main (tests/native/bg_noise_main.cpp) includes the header alone
and prints the bits of bg_noise_row<L> for L = 1..8, rows {0, 1, 2^32 - 1}, env ids {0, 63, 64,
2^32 - 1} and seeds {0, 1, 2^64 - 1}. It is built with -fsanitize=address,undefined and
-ffp-contract=off as tests/test_noise_host.py builds its own (a plain executable; nothing here is
loaded into Python). Every word is compared, which pins the block and pair selection for every L:
L = 1 half a pair, 2 a pair, 3 a pair and a half, 4 a block, 5 a block and half a pair, 8 two
blocks."""
import os
import subprocess

import numpy as np
import pytest

import noise_ref
from conftest import PKG_ROOT, REPO

SRC = os.path.join(REPO, "tests", "native", "bg_noise_main.cpp")
OUT = os.path.join(REPO, "tests", "native", "_build", "bg_noise")
CSRC = os.path.join(PKG_ROOT, "csrc")

LEVELS = tuple(range(1, 9))
SEEDS = (0, 1, 2 ** 64 - 1)
ROWS = (0, 1, 2 ** 32 - 1)
ENVS = (0, 63, 64, 2 ** 32 - 1)


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
def printed():
    """{(L, seed, row, env): the L words the program printed}."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([build()], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    out = {}
    for line in r.stdout.strip().splitlines():
        kind, *kv = line.split()
        assert kind == "row", line
        d = dict(x.split("=") for x in kv)
        key = (int(d["L"]), int(d["seed"]), int(d["k"]), int(d["e"]))
        assert key not in out
        out[key] = [int(x, 16) for x in d["x"].split(",")]
    return out


def test_every_case_is_printed(printed):
    assert set(printed) == {(L, s, k, e) for L in LEVELS for s in SEEDS for k in ROWS for e in ENVS}
    assert all(len(v) == key[0] for key, v in printed.items())


@pytest.mark.parametrize("L", LEVELS)
def test_the_row_equals_the_numpy_rows(printed, L):
    for s in SEEDS:
        for k in ROWS:
            for e in ENVS:
                want = noise_ref.rows(s, 1, 1, L, row0=k, env_offset=e).view(np.uint32).reshape(L)
                assert printed[(L, s, k, e)] == [int(x) for x in want], (L, s, k, e)


def test_a_shorter_row_is_a_prefix_of_a_longer_one(printed):
    """Element a does not depend on L: the half pair of an odd L is its pair's cosine, and a row
    that ends inside a block uses that block's first words."""
    for s in SEEDS:
        for k in ROWS:
            for e in ENVS:
                full = printed[(8, s, k, e)]
                for L in LEVELS:
                    assert printed[(L, s, k, e)] == full[:L], (L, s, k, e)
