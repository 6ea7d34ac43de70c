// The step servers' host lifecycle (include/scgpu.h scg_bg_server_*, scg_sc_server_*), one
// copy for the BeerGame wave and the SupplyChain block: retire, the stale rule, the launch
// bookkeeping, publishing a request line and the wait loop. Host only, and no HIP runtime
// call of its own: the stream query, the stream synchronise and the launch arrive as
// callables from the two .hip files, so tests/native/server_wait_main.cpp drives every branch
// of the wait loop on the CPU. The mailbox protocol itself (device + host) is scg_mailbox.h.
//
// The server structs (scg_bg_server, scg_sc_server) share the fields used here: box_host
// (with exit_req), running, idle_us, check_us, last_ns and launches.
//
// Restriction: servers of different kinds must not be stepped from concurrent threads. One
// thread's resident.claim (envs/resident.py) may retire a server between another thread's post
// and its wait; that wait then stalls for a check interval and launches again without claiming
// the device, so two servers may be resident at once.
#pragma once

#include <cstdint>

#include "scg_common.h"
#include "scg_mailbox.h"
#include "scgpu.h"

namespace scg {

// The wait loop's lock policy for a server whose host bookkeeping has one caller at a time.
struct NoLock {
  template <class Server>
  explicit NoLock(Server*) {}
};

// The words of a server's error messages: "<who>: <the stream> reports ... (<unit> %d)".
struct ServerNames {
  const char* who;     // "step server"
  const char* stream;  // "the wave's stream"
  const char* runner;  // "wave"
  const char* unit;    // "week"
};

// Ask the resident wave or block to exit and wait for it (`sync`: true once its stream is idle).
template <class Server, class Sync>
int server_retire(Server* sv, Sync&& sync, const char* who) {
  if (!sv->running) return SCG_OK;
  __atomic_store_n(&sv->box_host->exit_req, sv->box_host->exit_req + 1, __ATOMIC_RELEASE);
  sv->running = 0;
  if (!sync()) return fail(SCG_ERR_HIP, "%s: hipStreamSynchronize failed", who);
  return SCG_OK;
}

// Idle for more than half its time-out, it may be exiting: retire it before posting.
template <class Server>
bool server_stale(const Server* sv, int64_t now_ns) {
  return sv->running && now_ns - sv->last_ns > static_cast<int64_t>(sv->idle_us) * 500;
}

// Launch through `launch(exit_seen, idle_ticks)`: the exit word the wave starts from and its
// idle time-out in ticks of the 100 MHz real-time clock; then the bookkeeping.
template <class Server, class Launch>
int server_launch(Server* sv, Launch&& launch) {
  const uint32_t exit_seen = __atomic_load_n(&sv->box_host->exit_req, __ATOMIC_ACQUIRE);
  if (int rc = launch(exit_seen, static_cast<uint32_t>(sv->idle_us) * 100u)) return rc;
  sv->running = 1;
  sv->launches += 1;
  sv->last_ns = mono_ns();
  return SCG_OK;
}

// Publish a request line: words 1..N-1 relaxed, then word 0 (the request number) with release.
template <int N>
void server_publish(uint32_t* dst, const uint32_t (&line)[N]) {
  for (int i = 1; i < N; ++i) __atomic_store_n(&dst[i], line[i], __ATOMIC_RELAXED);
  __atomic_store_n(&dst[0], line[0], __ATOMIC_RELEASE);
}

// Wait until *answer == seq: SCG_OK, SCG_PENDING after spin_us (< 0: no limit), or an error.
// Every check interval (sv->check_us, 0: 2 s), under `Lock`: a stream error fails at once; a
// wave that has exited without serving the request (its stream idle: a host stall past its
// time-out, an exit another thread asked for) is launched again, once per wait (it serves
// pending requests first), and a second time is an error; a wave still queued or running is
// waited for, up to 60 s in all. `query(&text)` gives the stream's StreamState (and the error's
// text), `relaunch()` launches and returns an scg code; `when` is the week or step.
template <class Lock, class Server, class Query, class Relaunch>
int server_await(Server* sv, const uint32_t* answer, uint32_t seq, int64_t spin_us, int32_t* relaunches,
                 Query&& query, Relaunch&& relaunch, const ServerNames& nm, int when) {
  const int64_t start = mono_ns();
  const int64_t check_ns = (sv->check_us > 0 ? sv->check_us : 2000000) * int64_t(1000);
  int64_t check = start + check_ns;
  int gone = 0;
  for (uint32_t spins = 0;; ++spins) {
    if (__atomic_load_n(answer, __ATOMIC_ACQUIRE) == seq) break;
    cpu_relax();
    if ((spins & 255u) != 255u) continue;
    const int64_t now = mono_ns();
    if (spin_us >= 0 && now - start > spin_us * 1000) return SCG_PENDING;
    if (now < check) continue;
    check = now + check_ns;
    Lock lk(sv);
    const char* text = "";
    const StreamState q = query(&text);
    if (q == kStreamError) return fail(SCG_ERR_HIP, "%s: %s reports %s (%s %d)", nm.who, nm.stream, text, nm.unit, when);
    if (__atomic_load_n(answer, __ATOMIC_ACQUIRE) == seq) break;
    if (q == kStreamIdle) {
      if (gone++ > 0)
        return fail(SCG_ERR_HIP, "%s: the %s exits without answering (%s %d)", nm.who, nm.runner, nm.unit, when);
      sv->running = 0;
      *relaunches += 1;
      if (int rc = relaunch()) return rc;
    }
    if (now - start > 60000000000LL) return fail(SCG_ERR_HIP, "%s: no answer for 60 s (%s %d)", nm.who, nm.unit, when);
  }
  sv->last_ns = mono_ns();
  return SCG_OK;
}

}  // namespace scg
