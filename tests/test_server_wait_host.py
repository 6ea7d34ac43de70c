"""The step servers' host lifecycle (csrc/scg_server_host.h) on the CPU: a stand-alone program
with its own main (tests/native/server_wait_main.cpp) drives the wait loop that
scg_bg_server_wait and scg_sc_server_wait share with fake stream-query and launch callables,
so the branches no GPU test may provoke (a stream error, a wave gone twice, a failing launch)
run here; and the publish, stale, retire and launch helpers. It prints one line per case."""
import os
import subprocess

import pytest

from conftest import PKG_ROOT, REPO

SRC = os.path.join(REPO, "tests", "native", "server_wait_main.cpp")
OUT = os.path.join(REPO, "tests", "native", "_build", "server_wait")
CSRC = os.path.join(PKG_ROOT, "csrc")


def build():
    deps = [SRC, os.path.join(REPO, "include", "scgpu.h")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    tmp = f"{OUT}.{os.getpid()}.tmp"  # concurrent test workers: build aside, rename into place
    subprocess.run(["hipcc", "-std=c++17", "-O1", "--offload-host-only", "-Wall", "-Wno-unused-function", "-pthread",
                    "-I", os.path.join(REPO, "include"), "-I", CSRC, "-o", tmp, SRC], check=True)
    os.replace(tmp, OUT)
    return OUT


@pytest.fixture(scope="module")
def lines():
    r = subprocess.run([build()], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for line in r.stdout.strip().splitlines():
        name, rest = line.split(" ", 1)
        head, _, msg = rest.partition(" msg=")
        out[name] = dict(kv.split("=") for kv in head.split())
        out[name]["msg"] = msg
    return out


def _case(lines, name, rc, queries=None, launches=0):
    c = lines[name]
    assert c["rc"] == rc, (name, c)
    assert int(c["launches"]) == int(c["relaunches"]) == launches, (name, c)
    assert c["locks"] == c["queries"], (name, c)  # the lock is taken for every check, and only then
    if queries is not None:
        assert int(c["queries"]) == queries, (name, c)
    return c


def test_answer_already_present(lines):
    c = _case(lines, "present", "OK", queries=0)
    assert c["stamped"] == "1"  # last_ns: the time of the request last served


def test_pending_after_spin_us(lines):
    c = _case(lines, "pending", "PENDING", queries=0)
    assert c["stamped"] == "0" and c["running"] == "1"


def test_busy_stream_is_waited_for(lines):
    c = _case(lines, "busy_then_answered", "OK")
    assert int(c["queries"]) >= 1 and c["running"] == "1"


def test_gone_once_is_launched_again(lines):
    c = _case(lines, "gone_once", "OK", queries=1, launches=1)
    assert c["running"] == "1" and c["stamped"] == "1"


def test_gone_twice_is_an_error(lines):
    c = _case(lines, "gone_twice", "ERR_HIP", queries=2, launches=1)
    assert c["msg"] == "test server: the block exits without answering (step 7)"


def test_stream_error_fails_at_once(lines):
    c = _case(lines, "stream_error", "ERR_HIP", queries=1)
    assert c["msg"] == "test server: the stream reports a made-up stream error (step 7)"
    assert c["running"] == "1"


def test_answer_between_query_and_recheck(lines):
    c = _case(lines, "answer_during_query", "OK", queries=1)
    assert c["running"] == "1"  # an idle stream with the answer in place is not a gone wave


def test_failing_relaunch_returns_its_code(lines):
    c = _case(lines, "relaunch_fails", "ERR_INVALID", queries=1, launches=1)
    assert c["running"] == "0" and c["msg"] == "test server: a made-up launch failure"


def test_publish_stale_retire_launch(lines):
    assert lines["publish"] == {"words16": "1", "words32": "1", "msg": ""}
    assert lines["stale"] == {"at_half": "0", "past_half": "1", "stopped": "0", "msg": ""}
    r = lines["retire"]
    assert r == {"idle": "OK", "exit0": "0", "ran": "OK", "exit1": "1", "syncs": "1", "running": "0",
                 "failed": "ERR_HIP", "exit2": "2", "msg": "test server: hipStreamSynchronize failed"}
    assert lines["launch"] == {"rc": "OK", "exit_seen": "2", "idle_ticks": "2000000", "running": "1", "launches": "1",
                               "failed": "ERR_HIP", "running_after": "0", "launches_after": "1", "msg": ""}
