"""The order of the closed-loop entry points' checks (no GPU needed): every row is a call of
scg_bg_rollout_policy, scg_bg_rollout_local or scg_bg_rollout_mlp that is wrong in two ways at
once, with the return code and the start of the message of the check that comes first. The
expectations were recorded from the library as it stood before the three entry points shared
one host path; the linear entry point checks the level count after its policy, the other two
check the config after the policy and before n_weeks."""
import ctypes

import pytest

from test_bg2_rollout_abi import T
from test_bg_local_abi import _policy as local_policy
from test_bg_mlp_abi import _policy as mlp_policy
from test_bg_policy_abi import FAKE, _policy as linear_policy, _prepared_v1

ENTRY = {"linear": ("scg_bg_rollout_policy", linear_policy), "local": ("scg_bg_rollout_local", local_policy),
         "mlp": ("scg_bg_rollout_mlp", mlp_policy)}

# (entry point, config edits, policy arguments (None: a null policy struct's params), n_weeks,
#  the state's week, return code, how the message starts)
ROWS = [
    # null params together with n_weeks = -1
    ("linear", {}, dict(params=None), -1, 0, "SCG_ERR_INVALID", "policy rollout needs a policy with params"),
    ("local", {}, dict(params=None), -1, 0, "SCG_ERR_INVALID", "local policy rollout needs a policy with params"),
    ("mlp", {}, dict(params=None), -1, 0, "SCG_ERR_INVALID", "MLP policy rollout needs a policy with params"),
    # a wrong kind together with 9 levels
    ("linear", dict(levels=9), dict(kind=2), 2, 0, "SCG_ERR_INVALID", "unknown policy kind 2"),
    ("local", dict(levels=9), dict(kind=1), 2, 0, "SCG_ERR_INVALID", "unknown local policy kind 1"),
    ("mlp", dict(levels=9), dict(kind=2), 2, 0, "SCG_ERR_INVALID", "unknown MLP policy kind 2"),
    # a valid policy with 9 levels together with n_weeks = -1
    ("linear", dict(levels=9), {}, -1, 0, "SCG_ERR_INVALID", "policy rollout: levels=9 above 8"),
    ("local", dict(levels=9), {}, -1, 0, "SCG_ERR_INVALID", "local policy: levels=9 above 8"),
    ("mlp", dict(levels=9), {}, -1, 0, "SCG_ERR_INVALID", "local policy: levels=9 above 8"),
    # a 65-week delay together with n_weeks = -1
    ("local", dict(delay=65), {}, -1, 0, "SCG_ERR_INVALID", "local policy: shipment_delays[5]=65 above SCG_BG_LOCAL_MAX_DELAY=64"),
    ("mlp", dict(delay=65), {}, -1, 0, "SCG_ERR_INVALID", "local policy: shipment_delays[5]=65 above SCG_BG_LOCAL_MAX_DELAY=64"),
    # a bad shift or hidden together with full_table
    ("linear", dict(full_table=1), dict(shift=31), 2, 0, "SCG_ERR_INVALID", "policy needs shift in 0..30"),
    ("local", dict(full_table=1), dict(shift=31), 2, 0, "SCG_ERR_INVALID", "local policy needs shift in 0..30"),
    ("mlp", dict(full_table=1), dict(hidden=65), 2, 0, "SCG_ERR_INVALID", "MLP policy needs hidden in 1..64"),
    # a valid call before reset() together with a rollout past the horizon
    ("linear", {}, {}, T + 5, -1, "SCG_ERR_NOT_RESET", "step() before reset()"),
    ("local", {}, {}, T + 5, -1, "SCG_ERR_NOT_RESET", "step() before reset()"),
    ("mlp", {}, {}, T + 5, -1, "SCG_ERR_NOT_RESET", "step() before reset()"),
    # noise without std together with a 65-week delay
    ("mlp", dict(delay=65), dict(noise=FAKE), 2, 0, "SCG_ERR_INVALID", "MLP policy: noise and std go together"),
]


@pytest.mark.parametrize("entry,edits,pol,k,week,code,text", ROWS,
                         ids=[f"{r[0]}-{i}" for i, r in enumerate(ROWS)])
def test_the_first_check_wins(entry, edits, pol, k, week, code, text):
    nat, c, st, keep = _prepared_v1(levels=edits.get("levels", 4))
    if "delay" in edits:
        keep["delays"][5] = edits["delay"]
    c.full_table = edits.get("full_table", 0)
    assert nat.lib.scg_bg_prepare(ctypes.byref(c)) == 0, nat.last_error()
    st.week = week
    name, make = ENTRY[entry]
    policy = make(nat, **pol)
    rc = getattr(nat.lib, name)(ctypes.byref(c), ctypes.byref(st), k, ctypes.byref(policy), FAKE, FAKE, FAKE, FAKE, 0, None)
    assert rc == getattr(nat, code)
    assert nat.last_error().startswith(text), nat.last_error()
    assert (st.week, st.episode) == (week, 3)
