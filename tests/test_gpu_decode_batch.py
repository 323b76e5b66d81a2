"""heist_architect_decode on whole batches against tests/decode_ref.py (pinned to the reference's
recordings by tests/test_decode_ref_cpu.py): the per-env indexing (cam + e * cam_stride,
budget[e], the e * max_* output strides), truncation to the capacities, the curriculum filter,
the 64-lane block edge, and "too poor for this asset, keep scanning"."""
import functools

import numpy as np
import pytest
import torch

import decode_ref
from heist_amd import EnvironmentConfig, HeistEnv
from heist_amd.architect_decode import capacities, decode_layouts
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

BUDGETS = (0, 1, 2, 4, 5, 15, 40)
GRIDS = [(3, 3), (20, 20), (13, 17), (64, 64)]


def _maps(n, R, C, seed):
    """Per-env maps and budgets, the env's kind cycling through:
      0 dense random classes (the budget runs out mid-row);
      1 sparse (the budget never runs out, unless it is 0);
      2 the first interior cells are a guard and a camera, walls after them, budget 2 or 4
        (too poor for the guard at both, for the camera at 2: the scan goes on);
      3 assets on every border cell, which must be ignored, around a sparse interior."""
    rng = np.random.default_rng(seed)
    amap = np.zeros((n, R, C), np.int64)
    bud = rng.choice(BUDGETS, n).astype(np.int32)
    for e in range(n):
        kind = e % 4
        if kind == 0:
            amap[e] = rng.integers(0, 4, (R, C))
        elif kind in (1, 3):
            cells = rng.random((R, C)) < 2.0 / max(R * C, 1)
            amap[e] = np.where(cells, rng.integers(1, 4, (R, C)), 0)
            if kind == 3:
                border = np.ones((R, C), bool)
                border[1:-1, 1:-1] = False
                amap[e][border] = rng.integers(1, 4, int(border.sum()))
        else:
            inner = np.zeros((R - 2) * (C - 2), np.int64)
            inner[:6] = (3, 2, 1, 3, 1, 2)[:len(inner)]
            amap[e, 1:-1, 1:-1] = inner.reshape(R - 2, C - 2)
            bud[e] = (2, 4)[(e // 4) % 2]
    return amap, bud


@functools.lru_cache(maxsize=None)
def _case(n, R, C, per_env_cam):
    """The batch and the reference's full scan of every env, made once per (n, grid, camera
    form) and shared by the filter / capacity cases (which only read them)."""
    amap, bud = _maps(n, R, C, seed=1000 * n + 64 * R + C)
    rng = np.random.default_rng(7 * n + R)
    rows = n if per_env_cam else 1
    cam = np.stack([30 + 90 * rng.random(rows), 5 + 30 * rng.random(rows), 360 * rng.random(rows)], 1)
    cam = cam.astype(np.float32)  # distinct per env: a wrong stride reads another env's values
    scans = [decode_ref.scan(amap[e], cam[e if per_env_cam else 0], bud[e]) for e in range(n)]
    return amap, bud, cam, scans


def _expected(scans, n, R, C, allow_cams, allow_guards, mw, mc, mg, max_path):
    """decode_ref's lists as the dense arrays decode_layouts returns: the used prefix filled,
    everything past each env's count the zeros it was allocated with."""
    W, nw = np.zeros((n, mw, 2), np.int32), np.zeros(n, np.int32)
    CP, nc = np.zeros((n, mc, 6), np.float64), np.zeros(n, np.int32)
    GP, GM = np.zeros((n, mg, max_path, 2), np.int32), np.zeros((n, mg, 3), np.int32)
    GF, ng = np.zeros((n, mg), np.float64), np.zeros(n, np.int32)
    lists = []
    for e in range(n):
        walls, cams, guards = decode_ref.finish(scans[e], allow_cams, allow_guards, mw, mc, mg)
        lists.append((walls, cams, guards))
        nw[e], nc[e], ng[e] = len(walls), len(cams), len(guards)
        for i, rc in enumerate(walls):
            W[e, i] = rc
        for i, c in enumerate(cams):
            CP[e, i] = (c["row"], c["col"], c["fov_angle"], c["heading"], c["rotation_speed"], c["vision_range"])
        for i, g in enumerate(guards):
            assert len(g["patrol_path"]) == 8
            GP[e, i, :8] = g["patrol_path"]
            GM[e, i] = (8, g["speed"], g["vision_range"])
            GF[e, i] = g["fov_angle"]
    return dict(wall_rc=W, n_walls=nw, cam_params=CP, n_cams=nc, guard_paths=GP, guard_meta=GM, guard_fov=GF,
                n_guards=ng), lists


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("max_path", [8, 12])
@pytest.mark.parametrize("small_caps", [False, True], ids=["default_caps", "caps_3_1_1"])
@pytest.mark.parametrize("allow_cams,allow_guards", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("per_env_cam", [False, True], ids=["cam_stride0", "cam_stride3"])
@pytest.mark.parametrize("R,C", GRIDS)
@pytest.mark.parametrize("n", [1, 65, 130])
def test_decode_batch_matches_reference(gpu_device, n, R, C, per_env_cam, allow_cams, allow_guards, small_caps,
                                        max_path):
    """Counts, the used prefix of every array (ints and float64 bit-equal), guard_meta (8, 1, 4)
    and fov 90.0, and zeros past each env's count, for every env of the batch."""
    amap, bud, cam, scans = _case(n, R, C, per_env_cam)
    kw = dict(max_walls=3, max_cams=1, max_guards=1) if small_caps else {}
    cp = torch.from_numpy(cam if per_env_cam else cam[0]).to(gpu_device)
    assert cp.shape == ((n, 3) if per_env_cam else (3,))
    lb = decode_layouts(torch.from_numpy(amap).to(gpu_device), cp, torch.from_numpy(bud).to(gpu_device),
                        allow_cams, allow_guards, max_path=max_path, **kw)
    mw, mc, mg = (3, 1, 1) if small_caps else capacities(int(bud.max()))
    want, lists = _expected(scans, n, R, C, allow_cams, allow_guards, mw, mc, mg, max_path)
    if small_caps and n >= 65 and (R, C) != (3, 3):  # the capacities are really below what was bought
        assert max(len(s[0]) for s in scans) > 3 and max(len(s[1]) for s in scans) > 1
        assert max(len(s[2]) for s in scans) > 1
    for k, w in want.items():
        got = getattr(lb, k).cpu().numpy()
        assert got.shape == w.shape and got.dtype == w.dtype, k
        bad = np.argwhere(_bits(got) != _bits(w))
        assert len(bad) == 0, "%s: %d entries differ, first at %s: got %r, want %r" % (
            k, len(bad), tuple(bad[0]), got[tuple(bad[0])], w[tuple(bad[0])])
    assert np.array_equal(lb.budget.cpu().numpy(), bud)
    used = want["guard_meta"][np.arange(mg)[None, :] < want["n_guards"][:, None]]
    assert (used == (8, 1, 4)).all()
    assert (want["guard_fov"][np.arange(mg)[None, :] < want["n_guards"][:, None]] == 90.0).all()
    # LayoutBatch.to_lists reads the same arrays back into the reference's form
    if n <= 65:
        assert lb.to_lists() == lists


def test_decoded_batch_sets_the_same_layouts_as_the_reference_lists(gpu_device):
    """End to end at 20 x 20: HeistEnv.set_layout_batch on the decoded batch against
    HeistEnv.set_layouts on decode_ref's lists: the exported grids are equal, and `valid` is the
    oracle's BFS on those grids."""
    n, R, C = 130, 20, 20
    amap, bud, cam, scans = _case(n, R, C, True)
    cfg = EnvironmentConfig()
    assert (cfg.grid_rows, cfg.grid_cols) == (R, C)
    mc, mg, mp = 13, 8, 8
    envs = [HeistEnv(n, cfg, max_cams=mc, max_guards=mg, max_path=mp, device=gpu_device) for _ in range(2)]
    lb = decode_layouts(torch.from_numpy(amap).to(gpu_device), torch.from_numpy(cam).to(gpu_device),
                        torch.from_numpy(bud).to(gpu_device), max_cams=mc, max_guards=mg, max_path=mp)
    lists = [decode_ref.finish(s, max_cams=mc, max_guards=mg) for s in scans]
    assert max(len(s[1]) for s in scans) <= mc and max(len(s[2]) for s in scans) <= mg  # nothing truncated
    va = envs[0].set_layout_batch(lb).cpu().numpy()
    vb = envs[1].set_layouts(lists, budget=[int(b) for b in bud]).cpu().numpy()
    ga, gb = (e.export(grid=True)["grid"].cpu().numpy() for e in envs)
    assert np.array_equal(ga, gb)
    assert np.array_equal(va, vb)
    want = np.array([po.bfs(ga[e], cfg.start_pos, cfg.vault_pos) for e in range(n)])
    assert np.array_equal(va.astype(bool), want)
    assert want.any() and (ga != 0).any()
    for e in envs:
        e.close()
