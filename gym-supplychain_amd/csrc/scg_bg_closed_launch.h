// bg_launch_closed: the closed-loop rollout kernels of one source for levels 1-8 behind the one
// level switch. A unit that includes this holds the explicit instantiation for its source.
#pragma once

#include "scg_beergame_kernels.h"

namespace scg {

template <class Source>
int bg_launch_closed(int L, int variant, dim3 grid, hipStream_t s, const BgArgs& a, int32_t K, const RolloutWeeks& weeks,
                     const Source& src) {
  switch (L) {
#define X(l) \
  case l: return bg_launch_rollout<l>(variant, grid, s, a, K, weeks, src);
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#undef X
    default: return fail(SCG_ERR_INVALID, "policy rollout: levels=%d outside 1..%d", L, SCG_BG_POLICY_MAX_LEVELS);
  }
}

}  // namespace scg
