"""The planner field's references (field_ref.py) against the planner's (plan_ref.py), and
heist_amd.search.follow_field / expert_labels on CPU tensors.  No GPU: the witnesses and the
replays run the C oracle only."""
import numpy as np
import pytest
import torch

import field_ref as fr
import plan_ref as pr
from heist_amd import _native
from heist_amd.obs_compact import record_words
from heist_amd.search import expert_labels, follow_field

NAMES = list(pr.CASES)


# ---- 1. the backward recurrence against the forward one, one run per start cell

@pytest.mark.parametrize("R,C", [(10, 10), (13, 17), (7, 9)])
def test_field_equals_plan_per_cell(R, C):
    rng = np.random.Generator(np.random.PCG64(1000 * R + C))
    H, mismatches, cut, forced = 26, 0, 0, 0
    for i in range(10):
        walls = rng.random((R, C)) < 0.2
        walls[0, :] = walls[-1, :] = walls[:, 0] = walls[:, -1] = True
        free = np.argwhere(~walls)
        vault = tuple(int(v) for v in free[rng.integers(len(free))])
        planes = [rng.random((R, C)) < rng.choice([0.1, 0.3]) for _ in range(H)]
        tick0, max_steps = int(rng.integers(0, 4)), (25 if i % 2 else 200)
        togo, action, ticks = fr.field_from_planes(walls, vault, planes, tick0, max_steps)
        HK = min(H, max_steps - tick0)
        assert ticks.shape == (HK, R, C) and (togo == ticks[0]).all()
        assert (togo[walls] == -1).all() and (action[walls] == -1).all()
        assert ((action == -1) == (togo == -1)).all()
        dist = fr.bfs_dist(walls, vault)
        for r, c in free:
            T, _ = pr.plan_from_planes(walls, (int(r), int(c)), vault, planes, tick0, max_steps)
            mismatches += int(T != togo[r, c])
            forced += int(T > max(1, dist[r, c]))
        cut += int(HK < H)
    assert mismatches == 0
    assert cut > 0 and forced > 0  # the max_steps cut and waits were both exercised


def test_done_env_and_short_horizon():
    walls = np.zeros((7, 9), bool)
    walls[0, :] = walls[-1, :] = walls[:, 0] = walls[:, -1] = True
    planes = [np.zeros((7, 9), bool)] * 12
    togo, action, ticks = fr.field_from_planes(walls, (5, 7), planes, 0, 200, done=True)
    assert ticks.shape[0] == 0 and (togo == -1).all() and (action == -1).all()
    togo, action, ticks = fr.field_from_planes(walls, (5, 7), planes[:3], 0, 200)
    dist = fr.bfs_dist(walls, (5, 7))
    want = np.where((dist >= 1) & (dist <= 3), dist, -1)
    want[5, 7] = 1  # on the vault: a WAIT arrives
    np.testing.assert_array_equal(togo, want)
    assert action[5, 7] == 0 and action[5, 6] == 4 and action[4, 7] == 2
    # one tick before the timeout only direct arrivals have a value, and that value is 1
    togo, _, _ = fr.field_from_planes(walls, (5, 7), planes, 199, 200)
    np.testing.assert_array_equal(togo, np.where((dist >= 0) & (dist <= 1), 1, -1))


# ---- 2. the fixtures on the oracle's witness planes

@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_fixture_table_on_witness_planes(name):
    _, start, T, plan = pr.CASES[name]
    planes, walls, counts, togo, action, ticks = fr.case_reference(name)
    print(name, "witnesses per tick: min", min(counts), "max", max(counts))
    assert len(planes) == pr.MAX_STEPS and min(counts) >= 1
    assert togo[start] == T
    assert ticks.shape == (pr.MAX_STEPS, pr.GRID, pr.GRID)
    # every cell against the forward recurrence on the same planes
    for r, c in np.argwhere(~walls):
        t, _ = pr.plan_from_planes(walls, (int(r), int(c)), pr.VAULT, planes, 0, pr.MAX_STEPS)
        assert t == togo[r, c], (r, c)


# ---- 3. follow_field and expert_labels on CPU tensors

def test_follow_field_and_expert_labels_cpu():
    H, N = pr.MAX_STEPS, len(NAMES)
    field = fr.cases_field(NAMES, record_words(pr.GRID, pr.GRID))
    starts = np.array([pr.CASES[n][1] for n in NAMES])
    actions, ticks = follow_field(field, torch.from_numpy(starts[:, 0]), torch.from_numpy(starts[:, 1]))
    assert actions.shape == (H, N) and actions.dtype == torch.int64 and ticks.dtype == torch.int32
    assert ticks.tolist() == [pr.CASES[n][2] for n in NAMES]
    actions = actions.numpy()
    pos = np.zeros((H, N, 2), np.int64)
    pos[:] = starts
    for i, n in enumerate(NAMES):
        layout, start, T, _ = pr.CASES[n]
        assert not actions[max(T, 0):, i].any(), n  # the plan's length equals togo
        o, _ = fr.oracle_env(pr.GRID, pr.GRID, pr.MAX_STEPS, start, pr.VAULT, layout, pr.BUDGET)
        for k in range(max(T, 0)):
            _, done, _ = o.step(int(actions[k, i]))
            inf = o.info()
            assert done == (k == T - 1), (n, k)
            if k + 1 < H:
                pos[k + 1:, i] = (inf["pos_r"], inf["pos_c"])
        inf = o.info()
        if T > 0:
            assert (inf["vault_reached"], inf["detected"], inf["tick"]) == (1, 0, T), n
    togo, act = expert_labels(field, torch.from_numpy(pos[..., 0]), torch.from_numpy(pos[..., 1]))
    assert togo.shape == (H, N) and togo.dtype == torch.int16 and act.dtype == torch.int8
    togo, act = togo.numpy(), act.numpy()
    for i, n in enumerate(NAMES):
        T = pr.CASES[n][2]
        if T > 0:
            assert list(togo[:T, i]) == list(range(T, 0, -1)), n  # down by 1 per tick
            assert list(act[:T, i]) == list(actions[:T, i]), n
        else:
            assert togo[0, i] == -1 and act[0, i] == -1, n
    # K < H rows, and the errors
    t2, a2 = expert_labels(field, torch.from_numpy(pos[:5, :, 0]), torch.from_numpy(pos[:5, :, 1]))
    assert np.array_equal(t2.numpy(), togo[:5]) and np.array_equal(a2.numpy(), act[:5])
    field.togo_ticks = None
    with pytest.raises(ValueError):
        follow_field(field, torch.from_numpy(starts[:, 0]), torch.from_numpy(starts[:, 1]))


def test_plan_field_entry_points_exported():
    for name in ("heist_plan_field", "heist_plan_field_supported"):
        assert name in _native.SIGNATURES and name in _native.header_functions()
        assert hasattr(_native.lib(), name)
    assert _native.lib().heist_abi_version() == 5
    assert _native.lib().heist_plan_field_supported(None) == -1  # a bad handle
    assert _native.lib().heist_plan_field(None, 4, None, None, None, None, None) == 100000
