// The fused closed-loop launch (scg_sc_nodes.hip), as its caller sees it (scg_sc_policy.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "scg_supplychain_args.h"
#include "scg_normal.h"
#include "scg_sc_policy.h"
#include "scg_sc_mlp.h"

namespace scg {

// K closed-loop steps of every env in one launch, for Launch one of ScClosedLaunch<ScPolicyView>,
// ScClosedLaunch<ScMlpView>, ScSampledLaunch<ScPolicyView>, ScSampledLaunch<ScMlpView>,
// ScDrawnLaunch<ScPolicyView> and ScDrawnLaunch<ScMlpView> (the six instantiated). a.t / a.episode /
// a.flags describe the launch's first step. Refuses an MLP whose hidden width exceeds
// sc_mlp_fused_hidden_max(E, nodes), a sampled launch without std or noise, a drawn launch
// without std, and ledgers.
template <class Launch>
int sc_launch_nodes_closed(const ScArgs& a, const Launch& p, int maxd_bucket, int W, int E, int K, hipStream_t s);

}  // namespace scg
