// Round trips of the BeerGame week plan (csrc/scg_bg_plan.h) on the host: every packer against
// its unpacker at the limits of its fields, and the plan word's delay. One line per case;
// tests/test_bg_plan_host.py asserts on them. Includes nothing but the header under test.
#include "scg_bg_plan.h"

#include <cstdio>

using namespace scg;

static WeekInfo week(int32_t read_slot, int32_t write_slot, int32_t mode, int32_t flags) {
  WeekInfo wk{};
  wk.week = 1;
  wk.read_slot = read_slot;
  wk.write_slot = write_slot;
  wk.mode = mode;
  wk.flags = flags;
  return wk;
}

int main() {
  const int32_t modes[] = {MODE_DIRECT, MODE_STORE, MODE_ADD, MODE_DROP};
  // step packing: slots up to the longest full table's last row
  const int32_t top = SCG_BG_MAX_WEEKS + SCG_BG_MAX_DELAY + 1;
  const int32_t reads[] = {-1, 0, top};
  for (int32_t rs : reads)
    for (int32_t mode : modes)
      for (int32_t flags = 0; flags < 4; ++flags) {
        const WeekInfo wk = week(rs, top, mode, flags);
        const WeekPlan p = unpack_week(pack_week(wk));
        const bool ok = p.read_slot == rs && p.write_slot == top && p.mode == mode &&
                        (p.terminal != 0) == ((flags & WEEK_TERMINAL) != 0) &&
                        (p.autoreset != 0) == ((flags & WEEK_AUTORESET) != 0);
        std::printf("step read=%d write=%d mode=%d flags=%d ok=%d\n", rs, top, mode, flags, ok ? 1 : 0);
      }
  // a write slot of 0 beside the largest read slot: neither field leaks into the other
  {
    const WeekPlan p = unpack_week(pack_week(week(top, 0, MODE_ADD, 0)));
    std::printf("step_low_write ok=%d\n", (p.read_slot == top && p.write_slot == 0 && p.mode == MODE_ADD) ? 1 : 0);
  }
  // slab packing: a ring of at most kSlabRingMax slots, so slots 0 .. kSlabRingMax - 1
  const int32_t stop = static_cast<int32_t>(kSlabRingMax) - 1;
  const int32_t sreads[] = {-1, 0, stop};
  const int32_t rings[] = {1, static_cast<int32_t>(kSlabRingMax)};
  for (int32_t rs : sreads)
    for (int32_t R : rings)
      for (int32_t mode : modes)
        for (int32_t opt = 0; opt < 32; ++opt) {  // bit 0 terminal, 1 autoreset, 2 ledgers, 3 returns, 4 history
          const int32_t flags = ((opt & 1) ? WEEK_TERMINAL : 0) | ((opt & 2) ? WEEK_AUTORESET : 0);
          const bool ledgers = opt & 4, returns = opt & 8, history = opt & 16;
          const WeekPlan p = unpack_week_slab(pack_week_slab(week(rs, stop, mode, flags), R, ledgers, returns, history));
          const bool ok = p.read_slot == rs && p.write_slot == stop && p.mode == mode && p.R == R &&
                          (p.terminal != 0) == ((opt & 1) != 0) && (p.autoreset != 0) == ((opt & 2) != 0) &&
                          (p.ledgers != 0) == ledgers && (p.returns != 0) == returns && (p.history != 0) == history;
          std::printf("slab read=%d write=%d R=%d mode=%d opt=%d ok=%d\n", rs, stop, R, mode, opt, ok ? 1 : 0);
        }
  // the plan word keeps a week's whole delay beside its mode and arrival bit
  const int32_t delays[] = {0, 255, 256, SCG_BG_MAX_DELAY};
  for (int32_t d : delays)
    for (int32_t mode : modes)
      for (int arrive = 0; arrive < 2; ++arrive) {
        const int32_t w = plan_word(mode, arrive != 0, d);
        const bool ok = w >= 0 && plan_delay(w) == d && plan_mode(w) == mode && plan_arrive(w) == (arrive != 0);
        std::printf("plan delay=%d mode=%d arrive=%d ok=%d\n", d, mode, arrive, ok ? 1 : 0);
      }
  return 0;
}
