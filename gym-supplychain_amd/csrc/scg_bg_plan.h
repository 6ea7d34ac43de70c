// The BeerGame week plan, host and device (no HIP runtime header: a host program can include
// this alone). scg_bg_prepare writes one plan word per week into cfg->plan; per step the host
// turns week w's word into a WeekInfo and packs it into the one dword a kernel gets; the
// kernel unpacks it into a WeekPlan. Each packing has its packer and its unpacker side by
// side, built from the same constants.
#pragma once

#include <cstdint>

#include "scgpu.h"

#if defined(__HIPCC__)
#define SCG_PLAN_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define SCG_PLAN_HD inline
#endif

namespace scg {

// ---- per-week plan word (host computed, uniform per launch) -------------------------
enum : int32_t { MODE_DIRECT = 0, MODE_STORE = 1, MODE_ADD = 2, MODE_DROP = 3 };
constexpr int32_t PLAN_ARRIVE = 4;
inline int32_t plan_mode(int32_t p) { return p & 3; }
inline bool plan_arrive(int32_t p) { return (p & PLAN_ARRIVE) != 0; }
// bits 8 and up hold the week's whole delay (the word is non-negative)
constexpr int kPlanDelayShift = 8;
static_assert(static_cast<int64_t>(SCG_BG_MAX_DELAY) << kPlanDelayShift <= INT32_MAX, "plan delay field too narrow");
inline int32_t plan_word(int32_t mode, bool arrive, int32_t delay) {
  return mode | (arrive ? PLAN_ARRIVE : 0) | (delay << kPlanDelayShift);
}
inline int32_t plan_delay(int32_t p) { return p >> kPlanDelayShift; }

// Per-week launch info as the host computes it from the plan word.
constexpr int32_t WEEK_TERMINAL = 1, WEEK_AUTORESET = 2;
struct WeekInfo {
  int32_t week;        // 1..T
  int32_t read_slot;   // -1: nothing due
  int32_t write_slot;
  int32_t mode;        // MODE_*
  int32_t demand_fixed;
  int32_t flags;       // WEEK_TERMINAL, WEEK_AUTORESET
};

// What a kernel reads out of its packed week. A flag or option is non-zero when set: it is
// the word's own masked bit, so testing it compiles to the bit test on the word.
struct WeekPlan {
  int32_t read_slot;   // -1: nothing due
  int32_t write_slot;
  int32_t mode;        // MODE_*
  uint32_t terminal, autoreset;
  // slab packing only
  int32_t R;           // ring slots
  uint32_t ledgers, returns, history;
};

// ---- step packing (bg_step_kernel's preloaded arguments, the step server's request line) ----
// bits 0-13 read_slot + 1 (0: nothing due), 14-27 write_slot, 28-29 mode, 30-31 flags
// (slots < 2^14 > SCG_BG_MAX_WEEKS + SCG_BG_MAX_DELAY + 2, the longest full table).
constexpr uint32_t kWeekSlotBits = 14, kWeekSlotMask = (1u << kWeekSlotBits) - 1;
constexpr uint32_t kWeekModeShift = 2 * kWeekSlotBits, kWeekFlagsShift = kWeekModeShift + 2;
static_assert(SCG_BG_MAX_WEEKS + SCG_BG_MAX_DELAY + 2 < (1 << kWeekSlotBits), "ring slot field too narrow");
static_assert(kWeekFlagsShift + 2 == 32 && MODE_DROP <= 3 && (WEEK_TERMINAL | WEEK_AUTORESET) <= 3, "week word fields");
SCG_PLAN_HD uint32_t pack_week(const WeekInfo& wk) {
  return static_cast<uint32_t>(wk.read_slot + 1) | (static_cast<uint32_t>(wk.write_slot) << kWeekSlotBits) |
         (static_cast<uint32_t>(wk.mode) << kWeekModeShift) | (static_cast<uint32_t>(wk.flags) << kWeekFlagsShift);
}
SCG_PLAN_HD WeekPlan unpack_week(uint32_t w) {
  WeekPlan p{};
  p.read_slot = static_cast<int32_t>(w & kWeekSlotMask) - 1;
  p.write_slot = static_cast<int32_t>((w >> kWeekSlotBits) & kWeekSlotMask);
  p.mode = static_cast<int32_t>((w >> kWeekModeShift) & 3u);
  p.terminal = w & (static_cast<uint32_t>(WEEK_TERMINAL) << kWeekFlagsShift);
  p.autoreset = w & (static_cast<uint32_t>(WEEK_AUTORESET) << kWeekFlagsShift);
  return p;
}

// ---- slab packing (bg_step_slab_kernel) -------------------------------------------------
// The slab's ring has at most kSlabRingMax slots (scg_bg_slab_layout): bits 0-7 read_slot + 1,
// 8-15 write_slot, 16-17 mode, 18-22 the SW_* bits (the week's flags and which optional rows
// the slab keeps), 24-30 R.
constexpr uint32_t kSlabSlotBits = 8, kSlabSlotMask = (1u << kSlabSlotBits) - 1;
constexpr uint32_t kSlabModeShift = 2 * kSlabSlotBits, kSlabRingShift = 24, kSlabRingMax = 127;
constexpr uint32_t SW_TERMINAL = 1u << 18, SW_AUTORESET = 1u << 19, SW_LEDGERS = 1u << 20, SW_RETURNS = 1u << 21,
                   SW_HISTORY = 1u << 22;
static_assert(kSlabRingMax <= kSlabSlotMask && (3u << kSlabModeShift) < SW_TERMINAL &&
                  SW_HISTORY < (1u << kSlabRingShift) && (kSlabRingMax << kSlabRingShift) >> kSlabRingShift == kSlabRingMax,
              "slab week word fields");
SCG_PLAN_HD uint32_t pack_week_slab(const WeekInfo& wk, int32_t R, bool ledgers, bool returns, bool history) {
  return static_cast<uint32_t>(wk.read_slot + 1) | (static_cast<uint32_t>(wk.write_slot) << kSlabSlotBits) |
         (static_cast<uint32_t>(wk.mode) << kSlabModeShift) | ((wk.flags & WEEK_TERMINAL) ? SW_TERMINAL : 0u) |
         ((wk.flags & WEEK_AUTORESET) ? SW_AUTORESET : 0u) | (ledgers ? SW_LEDGERS : 0u) |
         (returns ? SW_RETURNS : 0u) | (history ? SW_HISTORY : 0u) | (static_cast<uint32_t>(R) << kSlabRingShift);
}
SCG_PLAN_HD WeekPlan unpack_week_slab(uint32_t w) {
  WeekPlan p{};
  p.read_slot = static_cast<int32_t>(w & kSlabSlotMask) - 1;
  p.write_slot = static_cast<int32_t>((w >> kSlabSlotBits) & kSlabSlotMask);
  p.mode = static_cast<int32_t>((w >> kSlabModeShift) & 3u);
  p.R = static_cast<int32_t>((w >> kSlabRingShift) & kSlabRingMax);
  p.terminal = w & SW_TERMINAL;
  p.autoreset = w & SW_AUTORESET;
  p.ledgers = w & SW_LEDGERS;
  p.returns = w & SW_RETURNS;
  p.history = w & SW_HISTORY;
  return p;
}

}  // namespace scg
