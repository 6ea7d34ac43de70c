"""The BeerGame week plan (csrc/scg_bg_plan.h) on the host: a stand-alone program with its own
main (tests/native/bg_plan_main.cpp), which includes that header alone, packs and unpacks a
week with both packings at the limits of their fields (read slot: nothing due, 0, the largest;
write slot: the largest; ring slots 1 and 127; every mode; every flag and option combination),
and reads the delay back out of plan words for 0, 255, 256 and SCG_BG_MAX_DELAY weeks. It
prints one line per case."""
import os
import subprocess

import pytest

from conftest import PKG_ROOT, REPO

SRC = os.path.join(REPO, "tests", "native", "bg_plan_main.cpp")
OUT = os.path.join(REPO, "tests", "native", "_build", "bg_plan")
CSRC = os.path.join(PKG_ROOT, "csrc")
MAX_WEEKS = MAX_DELAY = 4096  # SCG_BG_MAX_WEEKS, SCG_BG_MAX_DELAY (include/scgpu.h)


def build():
    deps = [SRC, os.path.join(REPO, "include", "scgpu.h"), os.path.join(CSRC, "scg_bg_plan.h")]
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    tmp = f"{OUT}.{os.getpid()}.tmp"  # concurrent test workers: build aside, rename into place
    subprocess.run(["hipcc", "-std=c++17", "-O1", "--offload-host-only", "-Wall", "-I", os.path.join(REPO, "include"),
                    "-I", CSRC, "-o", tmp, SRC], check=True)
    os.replace(tmp, OUT)
    return OUT


@pytest.fixture(scope="module")
def cases():
    r = subprocess.run([build()], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for line in r.stdout.strip().splitlines():
        kind, *kv = line.split()
        out.append((kind, {k: int(v) for k, v in (x.split("=") for x in kv)}))
    return out


def _of(cases, kind):
    return [c for k, c in cases if k == kind]


def test_step_packing_round_trips(cases):
    top = MAX_WEEKS + MAX_DELAY + 1
    got = _of(cases, "step")
    assert {(c["read"], c["write"], c["mode"], c["flags"]) for c in got} == \
        {(r, top, m, f) for r in (-1, 0, top) for m in range(4) for f in range(4)}
    assert all(c["ok"] == 1 for c in got), [c for c in got if c["ok"] != 1]
    assert _of(cases, "step_low_write") == [{"ok": 1}]


def test_slab_packing_round_trips(cases):
    got = _of(cases, "slab")
    assert {(c["read"], c["write"], c["R"], c["mode"], c["opt"]) for c in got} == \
        {(r, 126, R, m, o) for r in (-1, 0, 126) for R in (1, 127) for m in range(4) for o in range(32)}
    assert all(c["ok"] == 1 for c in got), [c for c in got if c["ok"] != 1]


def test_plan_word_keeps_whole_delays(cases):
    got = _of(cases, "plan")
    assert {(c["delay"], c["mode"], c["arrive"]) for c in got} == \
        {(d, m, a) for d in (0, 255, 256, MAX_DELAY) for m in range(4) for a in range(2)}
    assert all(c["ok"] == 1 for c in got), [c for c in got if c["ok"] != 1]
