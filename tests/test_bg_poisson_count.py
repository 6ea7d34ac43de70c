"""poisson_count_padded (scg_beergame_kernels.h) on the host: a stand-alone program with its own
main (tests/native/bg_poisson_count_main.cpp) compares it with the plain loop for table lengths
1, 7, 8, 9, 39, 40, 41 and 64 at u in {0, 1, 0xfffffffe, 0xffffffff} and thr[k] - 1, thr[k],
thr[k] + 1 for every k. On the GPU u == 0xffffffff, the one draw at which the block's
0xffffffff pads count, cannot be produced on demand; here it is an input."""
import os
import subprocess

from conftest import PKG_ROOT, REPO

SRC = os.path.join(REPO, "tests", "native", "bg_poisson_count_main.cpp")
OUT = os.path.join(REPO, "tests", "native", "_build", "bg_poisson_count")
CSRC = os.path.join(PKG_ROOT, "csrc")


def build():
    deps = [SRC, os.path.join(REPO, "include", "scgpu.h")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    tmp = f"{OUT}.{os.getpid()}.tmp"  # concurrent test workers: build aside, rename into place
    subprocess.run(["hipcc", "-std=c++17", "-O1", "--offload-host-only", "-Wno-unused-function", "-I",
                    os.path.join(REPO, "include"), "-I", CSRC, "-o", tmp, SRC], check=True)
    os.replace(tmp, OUT)
    return OUT


def test_padded_count_equals_the_plain_loop():
    r = subprocess.run([build()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "checked" and int(last[1]) > 8 * 3 * 4 and last[2:] == ["mismatches", "0"], r.stdout
