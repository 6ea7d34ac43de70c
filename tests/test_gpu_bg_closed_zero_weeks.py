"""rollout_policy(..., n_weeks=0) with each of the three closed-loop policies (scg_bg_rollout_policy,
_local, _mlp: one host path, whose zero-week branch launches nothing), on BeerGameVecEnv and
BeerGame2VecEnv: reward_sum is zeros, and the env stays bit-equal to a twin that made no call, before
and after one more step(). N = 70 is one full wave and a partial one, L = 2; three weeks of step()
first put live rows in the ring."""
import numpy as np
import pytest
import torch

from test_gpu_bg_local_policy import DEV, INVENTORY, LIST_DELAYS, _assert_same_state, _env1, _env2

pytestmark = pytest.mark.gpu
N, L, PRE, CLIP = 70, 2, 3, (0, 8)


def _make(variant):
    if variant == 1:
        return _env1(N, L)
    return _env2(N, levels=L, initial_inventory=INVENTORY[:L], shipment_delays=LIST_DELAYS)


def _packed(env, policy):
    rs = np.random.RandomState(11)
    if policy == "linear":
        return env.pack_policy(rs.randint(-64, 65, size=(N, L, L)), rs.randint(-2000, 2001, size=(N, L)))
    if policy == "local":
        return env.pack_local_policy(rs.randint(-64, 65, size=(N, L, 4)), rs.randint(-2000, 2001, size=(N, L)))
    H = 3
    return env.pack_local_mlp(*(torch.as_tensor(x.astype(np.float32)) for x in
                                (rs.randn(H, 4 * L) / 40, rs.randn(H), rs.randn(L, H), 4 + rs.randn(L))))


@pytest.mark.parametrize("policy", ["linear", "local", "mlp"])
@pytest.mark.parametrize("variant", [1, 2])
def test_no_weeks_leaves_the_env_as_its_twin(variant, policy):
    env, twin = _make(variant), _make(variant)
    acts = torch.as_tensor(np.random.RandomState(3).randint(CLIP[0], CLIP[1] + 1, size=(PRE + 1, N, L)), dtype=torch.int32,
                           device=DEV)
    for e in (env, twin):
        e.reset()
        for k in range(PRE):
            e.step(acts[k])
    assert env._ring.any()
    res = env.rollout_policy(_packed(env, policy), None, 0, shift=0 if policy == "mlp" else 4, clip=CLIP,
                             return_actions=True, return_obs=True, return_rewards=True)
    assert res.reward_sum.dtype == torch.int64 and tuple(res.reward_sum.shape) == (N,) and not res.reward_sum.any()
    assert tuple(res.actions.shape) == tuple(res.obs.shape) == (0, N, L) and tuple(res.rewards.shape) == (0, N)
    assert (env.week, env.episode) == (PRE, 0)
    _assert_same_state(env, twin)
    obs, rew, done, _ = env.step(acts[PRE])
    tobs, trew, tdone, _ = twin.step(acts[PRE])
    assert torch.equal(obs, tobs) and torch.equal(rew, trew) and torch.equal(done, tdone)
    _assert_same_state(env, twin)
    env.check_errors()
