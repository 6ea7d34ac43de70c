// The step servers' host lifecycle (csrc/scg_server_host.h) on the CPU: the wait loop driven
// with fake "query the stream" and "launch again" callables (and a thread that writes the answer
// word), the request-line publish, the stale rule, retire and launch. One line per case,
// which tests/test_server_wait_host.py asserts. Built with --offload-host-only; no GPU.
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <thread>

#include "scg_server_host.h"

namespace scg {
static char g_msg[512] = "";
int fail(int code, const char* fmt, ...) {  // libscgpu's is in scg_common.hip
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace scg

using namespace scg;

static int g_locks = 0;
struct CountLock {
  explicit CountLock(scg_sc_server*) { ++g_locks; }
};

static const ServerNames kNames{"test server", "the stream", "block", "step"};
static const char* code_name(int rc) {
  return rc == SCG_OK ? "OK" : rc == SCG_PENDING ? "PENDING" : rc == SCG_ERR_HIP ? "ERR_HIP"
       : rc == SCG_ERR_INVALID ? "ERR_INVALID" : "OTHER";
}

// One wait on a fresh SupplyChain server struct (the real one: the header is a template over
// its field names); query(n, answer) is the n-th stream query, relaunch(answer) the launch.
template <class Query, class Relaunch>
static void run(const char* name, int64_t spin_us, bool answered, int answer_after_us, Query&& query,
                Relaunch&& relaunch) {
  scg_sc_server_box box{};
  scg_sc_server sv{};
  sv.box_host = &box;
  sv.running = 1;
  sv.check_us = 1000;
  const uint32_t seq = 41;
  box.done_seq = answered ? seq : seq - 1;
  int queries = 0, launches = 0;
  g_locks = 0;
  g_msg[0] = 0;
  std::thread writer;
  if (answer_after_us > 0)
    writer = std::thread([&] {
      std::this_thread::sleep_for(std::chrono::microseconds(answer_after_us));
      __atomic_store_n(&box.done_seq, seq, __ATOMIC_RELEASE);
    });
  const int rc = server_await<CountLock>(
      &sv, &box.done_seq, seq, spin_us, &sv.relaunches,
      [&](const char** text) { return query(++queries, &box.done_seq, text); },
      [&] {
        ++launches;
        return relaunch(&sv, &box.done_seq);
      },
      kNames, 7);
  if (writer.joinable()) writer.join();
  std::printf("%s rc=%s queries=%d locks=%d launches=%d relaunches=%d running=%d stamped=%d msg=%s\n", name,
              code_name(rc), queries, g_locks, launches, sv.relaunches, sv.running, sv.last_ns != 0, g_msg);
}

int main() {
  const uint32_t seq = 41;
  auto busy = [](int, uint32_t*, const char**) { return kStreamBusy; };
  auto idle = [](int, uint32_t*, const char**) { return kStreamIdle; };
  auto launch_ok = [](scg_sc_server* sv, uint32_t*) {
    return server_launch(sv, [](uint32_t, uint32_t) { return int(SCG_OK); });
  };
  run("present", -1, true, 0, busy, launch_ok);
  run("pending", 0, false, 0, busy, launch_ok);
  run("busy_then_answered", -1, false, 3000, busy, launch_ok);
  run("gone_once", -1, false, 0, idle, [&](scg_sc_server* sv, uint32_t* answer) {
    __atomic_store_n(answer, seq, __ATOMIC_RELEASE);  // the new block serves the pending request
    return launch_ok(sv, answer);
  });
  run("gone_twice", -1, false, 0, idle, launch_ok);
  run("stream_error", -1, false, 0,
      [](int, uint32_t*, const char** text) {
        *text = "a made-up stream error";
        return kStreamError;
      },
      launch_ok);
  run("answer_during_query", -1, false, 0,
      [&](int, uint32_t* answer, const char**) {
        __atomic_store_n(answer, seq, __ATOMIC_RELEASE);  // lands between the query and the re-check
        return kStreamIdle;
      },
      launch_ok);
  run("relaunch_fails", -1, false, 0, idle,
      [](scg_sc_server*, uint32_t*) { return fail(SCG_ERR_INVALID, "test server: a made-up launch failure"); });

  // server_publish: 16- and 32-word lines land whole, word 0 included
  uint32_t l16[16], d16[16] = {0}, l32[32], d32[32] = {0};
  for (uint32_t i = 0; i < 16; ++i) l16[i] = 0x1000u + i;
  for (uint32_t i = 0; i < 32; ++i) l32[i] = 0x2000u + i;
  server_publish(d16, l16);
  server_publish(d32, l32);
  std::printf("publish words16=%d words32=%d\n", !std::memcmp(d16, l16, sizeof(l16)), !std::memcmp(d32, l32, sizeof(l32)));

  // server_stale: idle for more than idle_us / 2, and only while running
  scg_bg_server_box bbox{};
  scg_bg_server bsv{};
  bsv.box_host = &bbox;
  bsv.idle_us = 20000;
  bsv.last_ns = 5000;
  bsv.running = 1;
  const int64_t half = 10000000;  // idle_us / 2 in ns
  const bool at = server_stale(&bsv, bsv.last_ns + half), past = server_stale(&bsv, bsv.last_ns + half + 1);
  bsv.running = 0;
  std::printf("stale at_half=%d past_half=%d stopped=%d\n", at, past, server_stale(&bsv, bsv.last_ns + half + 1));

  // server_retire: a no-op when not running; else the exit word moves, then the synchronise
  int syncs = 0;
  const int rc0 = server_retire(&bsv, [&] { return ++syncs > 0; }, "test server");
  const uint32_t exit0 = bbox.exit_req;
  bsv.running = 1;
  const int rc1 = server_retire(&bsv, [&] { return ++syncs > 0; }, "test server");
  const uint32_t exit1 = bbox.exit_req;
  const int running1 = bsv.running;
  bsv.running = 1;
  const int rc2 = server_retire(&bsv, [&] { return false; }, "test server");
  std::printf("retire idle=%s exit0=%u ran=%s exit1=%u syncs=%d running=%d failed=%s exit2=%u msg=%s\n", code_name(rc0), exit0,
              code_name(rc1), exit1, syncs, running1, code_name(rc2), bbox.exit_req, g_msg);
  // server_launch: the launcher gets the exit word and the time-out in 100 MHz ticks; a failing
  // one's code comes back with the books untouched
  bsv.running = 0;
  uint32_t seen = 0, ticks = 0;
  const int rc3 = server_launch(&bsv, [&](uint32_t e, uint32_t t) { return seen = e, ticks = t, int(SCG_OK); });
  const int running3 = bsv.running;
  const long long launches3 = bsv.launches;
  bsv.running = 0;
  const int rc4 = server_launch(&bsv, [](uint32_t, uint32_t) { return int(SCG_ERR_HIP); });
  std::printf("launch rc=%s exit_seen=%u idle_ticks=%u running=%d launches=%lld failed=%s running_after=%d launches_after=%lld\n",
              code_name(rc3), seen, ticks, running3, launches3, code_name(rc4), bsv.running, (long long)bsv.launches);
  return 0;
}
