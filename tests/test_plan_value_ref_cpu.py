"""The planner value's references (value_ref.py) against the C oracle, and
heist_amd.search.follow_value / value_targets / discounted_return on CPU tensors.  No GPU: the
witnesses, the brute force and the replays run the C oracle only.  Every float64 comparison is
equality of the bits (through int64)."""
import numpy as np
import pytest
import torch

import field_ref as fr
import plan_ref as pr
import value_ref as vr
from heist_amd import _native
from heist_amd.obs_compact import record_words
from heist_amd.search import discounted_return, follow_value, value_targets

# the six fixtures whose layout passes the BFS check
VALID = [n for n in pr.CASES if n != "full_wallrow"]
GAMMAS = (1.0, 0.99)


def _dist(cell):
    return abs(cell[0] - pr.VAULT[0]) + abs(cell[1] - pr.VAULT[1])


# ---- 1. the restatement against the brute force over all 5^5 action sequences

@pytest.mark.parametrize("start", [(6, 6), (5, 4), (7, 8), (3, 5)])
def test_restatement_equals_brute_force(start):
    """max_steps 40: the horizon cuts the return; 5: the timeout falls on the last of the five
    ticks; 3: inside them.  The starts put detection ((5, 4) on the guard's row, (6, 6) beside the
    camera) and the vault ((7, 8), D0 = 1: no proximity bonus) inside the five ticks."""
    depth, G = 5, pr.GRID
    layout = pr.CASES["wallrow_both"][0]
    decided = set()
    for max_steps in (40, 5, 3):
        planes, walls, _ = fr.witness_planes(G, G, max_steps, start, pr.VAULT, layout, pr.BUDGET, horizon=depth)
        rewards = vr.oracle_returns(G, G, max_steps, start, pr.VAULT, layout, pr.BUDGET, depth)
        # what ended the sequences: a negative jump (detection), the vault's 10, trailing zeros (timeout)
        decided.add("detect" if (rewards < -0.5).any() else "none")
        decided.add("vault" if (rewards > 5).any() else "none")
        for gamma in GAMMAS:
            value = vr.value_from_planes(walls, pr.VAULT, planes, _dist(start), 0, max_steps, gamma)[0]
            best = vr.horner(rewards, gamma).max()
            print(start, max_steps, gamma, float(value[start]), float(best))
            assert vr.bits(value[start]) == vr.bits(best), (start, max_steps, gamma, value[start], best)
    if start == (7, 8):
        assert "vault" in decided
    if start in ((5, 4), (6, 6)):
        assert "detect" in decided


# ---- 2. the recurrence's own plan, replayed in the oracle

@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("name", VALID)
def test_greedy_plan_replayed_in_oracle(name, gamma):
    layout, start, T, _ = pr.CASES[name]
    planes, walls = fr.case_reference(name)[:2]
    value, action, vt, at = vr.case_value(name, gamma, _dist(start))
    assert vt.shape == at.shape == (pr.MAX_STEPS, pr.GRID, pr.GRID)
    assert vr.bits(vt[0]).tolist() == vr.bits(value).tolist() and (at[0] == action).all()
    assert (value[walls] == 0.0).all() and (action[walls] == -1).all() and (action[~walls] >= 0).all()
    plan = vr.greedy_plan(walls, pr.VAULT, planes, at, start)
    rewards, done = vr.oracle_replay(pr.GRID, pr.GRID, pr.MAX_STEPS, start, pr.VAULT, layout, pr.BUDGET, plan)
    assert done[-1] and not any(done[:-1]), name
    got = vr.horner(rewards, gamma)
    print(name, gamma, "optimal episode %d ticks (fastest %d), return %r" % (len(plan), T, float(got)))
    assert vr.bits(got) == vr.bits(value[start]), (name, gamma, float(got), float(value[start]))
    # the return-optimal episode is never shorter than the fastest clean one, and never pays less
    if T > 0:
        fast, _ = vr.oracle_replay(pr.GRID, pr.GRID, pr.MAX_STEPS, start, pr.VAULT, layout, pr.BUDGET, pr.CASES[name][3])
        assert vr.horner(fast, gamma) <= value[start]


def test_pinned_start_values():
    """V_0[start] at gamma 1: `empty` plays all 40 ticks beside the vault (the fastest plan, 14
    ticks, returns 11.56); wallrow_fixed_cam, which the planner calls unsolvable, still pays."""
    assert float(vr.case_value("empty", 1.0)[0][pr.START]) == 15.899999999999995
    assert float(vr.case_value("wallrow_fixed_cam", 1.0)[0][pr.START]) == 0.5714285714285716
    fast, _ = vr.oracle_replay(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, pr.CASES["empty"][0], pr.BUDGET,
                               pr.CASES["empty"][3])
    assert round(float(vr.horner(fast, 1.0)), 9) == 11.56


def test_done_env_and_gamma_zero():
    walls = np.zeros((7, 9), bool)
    walls[0, :] = walls[-1, :] = walls[:, 0] = walls[:, -1] = True
    planes = [np.zeros((7, 9), bool)] * 12
    value, action, vt, at = vr.value_from_planes(walls, (5, 7), planes, 10, 0, 200, 1.0, done=True)
    assert vt.shape[0] == 0 and (value == 0.0).all() and (action == -1).all()
    # gamma 0: the one-step reward; towards the vault pays 0.09 more than a wait
    value, action, _, _ = vr.value_from_planes(walls, (5, 7), planes, 10, 0, 200, 0.0)
    assert value[1, 1] == -0.01 + 1.0 * 0.1 and action[1, 1] == 2  # DOWN before RIGHT: the first maximum


# ---- 3. follow_value, value_targets and discounted_return on CPU tensors

@pytest.mark.parametrize("gamma", GAMMAS)
def test_helpers_cpu(gamma):
    H, N = pr.MAX_STEPS, len(VALID)
    pv = vr.cases_value(VALID, record_words(pr.GRID, pr.GRID), gamma)
    starts = np.array([pr.CASES[n][1] for n in VALID])
    sr, sc = torch.from_numpy(starts[:, 0]), torch.from_numpy(starts[:, 1])
    actions = follow_value(pv, sr, sc)
    assert actions.shape == (H, N) and actions.dtype == torch.int64
    assert torch.equal(pv.vis_mask(1)[0], torch.from_numpy(fr.case_reference(VALID[0])[0][0]))
    rewards, dones = np.zeros((H, N)), np.ones((H, N), bool)
    pos = np.zeros((H, N, 2), np.int64)
    pos[:] = starts
    for i, n in enumerate(VALID):
        layout, start = pr.CASES[n][:2]
        planes, walls = fr.case_reference(n)[:2]
        plan = vr.greedy_plan(walls, pr.VAULT, planes, pv.action_ticks[:, i].numpy(), start)
        assert actions[:len(plan), i].tolist() == plan and not actions[len(plan):, i].any(), n
        o, _ = fr.oracle_env(pr.GRID, pr.GRID, pr.MAX_STEPS, start, pr.VAULT, layout, pr.BUDGET)
        for k in range(H):  # the whole tensor, as step_multi(auto_reset=False) plays it
            rewards[k, i], dones[k, i], _ = o.step(int(actions[k, i]))
            inf = o.info()
            if k + 1 < H and k + 1 < len(plan):
                pos[k + 1:, i] = (inf["pos_r"], inf["pos_c"])
    ret = discounted_return(torch.from_numpy(rewards), torch.from_numpy(dones), gamma)
    assert ret.dtype == torch.float64 and ret.shape == (N,)
    v0 = pv.value[torch.arange(N), sr, sc]
    assert torch.equal(ret.view(torch.int64), v0.view(torch.int64)), (ret.tolist(), v0.tolist())
    val, act = value_targets(pv, torch.from_numpy(pos[..., 0]), torch.from_numpy(pos[..., 1]))
    assert val.shape == (H, N) and val.dtype == torch.float64 and act.dtype == torch.int8
    for i, n in enumerate(VALID):
        T = int(np.argmax(dones[:, i])) + 1
        for k in range(T):  # the Horner tail of the same rewards at every tick of the episode
            assert vr.bits(val[k, i].item()) == vr.bits(vr.horner(rewards[k:T, i], gamma)), (n, k)
        assert act[:T, i].tolist() == actions[:T, i].tolist(), n
    # no done row: the sum starts at row K - 1; K < H rows; the errors
    r = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], dtype=torch.float64)
    d = torch.tensor([[False, False], [False, True], [False, True]])
    assert discounted_return(r, d, 0.5).tolist() == [1.0 + 0.5 * (3.0 + 0.5 * 5.0), 2.0 + 0.5 * 4.0]
    v2, a2 = value_targets(pv, torch.from_numpy(pos[:5, :, 0]), torch.from_numpy(pos[:5, :, 1]))
    assert torch.equal(v2, val[:5]) and torch.equal(a2, act[:5])
    with pytest.raises(ValueError):
        discounted_return(r, d[:2], 1.0)
    pv.value_ticks = None
    follow_value(pv, sr, sc)  # needs the actions only
    with pytest.raises(ValueError):
        value_targets(pv, torch.from_numpy(pos[..., 0]), torch.from_numpy(pos[..., 1]))
    pv.action_ticks = None
    with pytest.raises(ValueError):
        follow_value(pv, sr, sc)


# ---- 4. registration

def test_plan_value_entry_points_exported():
    import heist_amd
    for name in ("heist_plan_value", "heist_plan_value_supported"):
        assert name in _native.SIGNATURES and name in _native.header_functions()
        assert hasattr(_native.lib(), name)
    assert _native.lib().heist_abi_version() == 5
    assert _native.lib().heist_plan_value_supported(None) == -1  # a bad handle
    assert _native.lib().heist_plan_value(None, 4, 1.0, None, None, None, None, None, None) == 100000
    assert hasattr(heist_amd, "PlanValue") and hasattr(heist_amd.HeistEnv, "plan_value")
    assert hasattr(heist_amd.HeistEnv, "plan_value_supported")
