"""heist_plan_place_guard without a GPU: the premise the kernel rests on, checked with the C oracle
alone (the visibility of a layout plus a guard whose patrol starts on an EMPTY tile is the layout's
own OR the guard's alone against the same walls -- and not when it starts on a wall), the validity
predicate restated, the pure-torch candidate builders and greedy_pick on hand-made tables, the
wrapper's argument checks that need no device, and the library's symbols."""
import ctypes

import numpy as np
import pytest
import torch

import guard_place_ref as gr
import plan_ref as pr
from heist_amd import _build, _native
from heist_amd.search import (CAMERA_COST, GUARD_COST, PlacementScan, architect_patrol, greedy_pick, guard_candidates)
from heist_amd.vec_env import HeistEnv


# ---- the union premise

@pytest.mark.parametrize("name", sorted(gr.PREMISE))
def test_union_premise(name):
    c = gr.PREMISE[name]
    assert gr.expect_valid(c)
    base, walls = gr.planes_of("base")
    plus, walls_plus = gr.planes_of(("plus", c))
    own, walls_own = gr.planes_of(("alone", c))
    assert (walls == walls_plus).all() and (walls == walls_own).all(), "a guard on an EMPTY start changes no wall"
    assert len(base) == len(own) == pr.MAX_STEPS
    print(name, "plus-layout witnessed for", len(plus), "ticks")
    if name in gr.SHORT_WITNESS:
        assert len(plus) == 10
    elif name in gr.FULL_WITNESS:
        assert len(plus) == pr.MAX_STEPS
    assert len(plus) >= 10
    for k in range(len(plus)):
        assert ((base[k] | own[k]) == plus[k]).all(), "tick %d of %s" % (k + 1, name)
    # the guard's own cell is marked on every tick, whatever its range
    path, speed, rng, _ = c
    idx = 0
    for k in range(pr.MAX_STEPS):
        if len(path) >= 2:
            idx = (idx + speed % len(path)) % len(path)
        assert own[k][path[idx]], "tick %d of %s: own cell" % (k + 1, name)
        if rng == 0:
            assert own[k].sum() == 1
    # the recurrence on base | alone, at the start cell, is the oracle search's answer
    T = gr.search(c)[0]
    ref = gr.reference(c, 1.0)
    print(name, "ticks", T)
    assert ref["ticks"] == T
    assert gr.reference(None, 1.0)["ticks"] == 22 and (T < 0 or T >= 22)


def test_never_moving_candidates():
    own = gr.planes_of(("alone", gr.PREMISE["speed_multiple_of_len"]))[0]
    assert all((own[k] == own[0]).all() for k in range(pr.MAX_STEPS)), "step 0: the same cone every tick"
    fwd = gr.planes_of(("alone", gr.PREMISE["rectangle"]))[0]
    back = gr.planes_of(("alone", gr.PREMISE["negative_speed"]))[0]
    assert any((a != b).any() for a, b in zip(fwd, back)), "a negative speed walks the other way round"


def test_start_on_wall_breaks_the_premise():
    c = gr.START_ON_WALL
    assert not gr.expect_valid(c)
    assert gr.bought(gr.with_cand(gr.BASE, c)) == (1, 2), "the oracle's purchase takes it: no placement check"
    base, walls = gr.planes_of("base")
    plus, walls_plus = gr.planes_of(("plus", c))
    own, walls_own = gr.planes_of(("alone", c))
    assert walls[c[0][0]] and not walls_plus[c[0][0]] and not walls_own[c[0][0]], "the wall under it is replaced"
    assert any(((base[k] | own[k]) != plus[k]).any() for k in range(len(plus))), "and the union no longer holds"


# ---- validity

def test_validity_table():
    assert all(gr.expect_valid(c) for c in gr.PREMISE.values())
    assert not any(gr.expect_valid(c) for c in gr.INVALID.values())
    _, walls = gr.planes_of("base")
    for name, c in sorted(gr.PREMISE.items()):  # every in-contract row: bought, and no wall changed
        assert gr.bought(gr.with_cand(gr.BASE, c)) == (1, 2), name
        assert (gr.planes_of(("alone", c))[1] == walls).all(), name
    # the patrol index and the heading
    c = gr.PREMISE["rectangle"]
    assert gr.expect_valid(c, idx=5) and not gr.expect_valid(c, idx=6) and not gr.expect_valid(c, idx=-1)
    assert gr.expect_valid(c, heading=-1e300) and not gr.expect_valid(c, heading=float("inf"))
    assert not gr.expect_valid(c, heading=float("nan")) and gr.expect_valid(c, heading=-0.0)
    assert not gr.expect_valid(c, p=5), "len = P + 1"
    # an invalid candidate's reference is the baseline's
    ref, base = gr.reference(gr.INVALID["start_on_wall"], 0.99), gr.reference(None, 0.99)
    assert not ref["valid"] and ref["ticks"] == base["ticks"] and (ref["togo"] == base["togo"]).all()


def test_arrays_helper():
    cands = list(gr.PREMISE.values())
    paths, meta, fov = gr.arrays(cands)
    assert paths.shape == (len(cands), gr.P, 2) and meta.shape == (len(cands), 4) and fov.shape == (len(cands), 2)
    for m, c in enumerate(cands):
        n = len(c[0])
        assert [tuple(v) for v in paths[m, :n].tolist()] == list(c[0]) and n < gr.P
        assert ((paths[m, n:] < 0) | (paths[m, n:] >= pr.GRID)).any(1).all(), "garbage past len lies outside the grid"
        assert meta[m].tolist() == [n, c[1], c[2], 0] and fov[m].tolist() == [c[3], 0.0]


# ---- architect_patrol, guard_candidates

def test_architect_patrol():
    assert architect_patrol(5, 5, 10, 10) == [(4, 4), (4, 5), (4, 6), (5, 6), (6, 6), (6, 5), (6, 4), (5, 4)]
    # corners: the ring is clamped to the interior
    assert architect_patrol(1, 1, 10, 10) == [(1, 1), (1, 1), (1, 2), (1, 2), (2, 2), (2, 1), (2, 1), (1, 1)]
    assert architect_patrol(8, 8, 10, 10) == [(7, 7), (7, 8), (7, 8), (8, 8), (8, 8), (8, 8), (8, 7), (8, 7)]
    assert architect_patrol(1, 11, 10, 13) == [(1, 10), (1, 11), (1, 11), (1, 11), (2, 11), (2, 11), (2, 10), (1, 10)]
    for r in range(1, 9):
        for c in range(1, 12):
            pts = architect_patrol(r, c, 10, 13)
            assert len(pts) == 8 and all(1 <= a <= 8 and 1 <= b <= 11 for a, b in pts)


def test_guard_candidates():
    R, C = 6, 7
    grid = torch.zeros((2, R, C), dtype=torch.int8)
    grid[:, 0, :] = grid[:, -1, :] = grid[:, :, 0] = grid[:, :, -1] = 1
    grid[1, 2, 3] = 1   # a wall
    grid[1, 1, 1] = 2   # the start tile
    grid[1, 3, 4] = 4   # a camera
    paths, meta, fov = guard_candidates(grid)
    M = (R - 2) * (C - 2)
    assert paths.shape == (2, M, 8, 2) and paths.dtype == torch.int32 and paths.is_contiguous()
    assert meta.shape == (2, M, 4) and meta.dtype == torch.int32 and fov.shape == (2, M, 2) and fov.dtype == torch.float64
    tiles = [(r, c) for r in range(1, R - 1) for c in range(1, C - 1)]
    for m, (r, c) in enumerate(tiles):
        want = architect_patrol(r, c, R, C)
        for e in range(2):
            assert [tuple(v) for v in paths[e, m].tolist()] == want
            empty = int(grid[e, want[0][0], want[0][1]]) == 0
            assert meta[e, m].tolist() == [8 if empty else 0, 1, 4, 0], (e, r, c)
            assert fov[e, m].tolist() == [90.0, 0.0]
    assert bool((meta[0, :, 0] == 8).all())
    # env 1: the tiles whose patrol starts on the wall (2, 3), the start (1, 1) or the camera (3, 4) carry no candidate;
    # (1, 1) is the start of the patrols of (1, 1), (1, 2), (2, 1) and (2, 2): corner clamping
    off = [m for m, (r, c) in enumerate(tiles) if architect_patrol(r, c, R, C)[0] in ((2, 3), (1, 1), (3, 4))]
    assert [tiles[m] for m in off] == [(1, 1), (1, 2), (2, 1), (2, 2), (3, 4), (4, 5)]
    assert torch.nonzero(meta[1, :, 0] == 0).reshape(-1).tolist() == off
    p2, m2, f2 = guard_candidates(grid.numpy(), speed=2, vision_range=7, fov=120.0)
    assert torch.equal(p2, paths) and m2[0, 0].tolist() == [8, 2, 7, 0] and f2[0, 0].tolist() == [120.0, 0.0]
    with pytest.raises(ValueError):
        guard_candidates(torch.zeros((5, 6), dtype=torch.int8))


# ---- greedy_pick

def _scan(valid, ticks, value, ticks0, value0):
    valid, ticks = torch.tensor(valid, dtype=torch.bool), torch.tensor(ticks, dtype=torch.int16)
    value = torch.tensor(value, dtype=torch.float64)
    return PlacementScan(valid, ticks, value, torch.zeros_like(ticks, dtype=torch.int8),
                         torch.tensor(ticks0, dtype=torch.int16), torch.tensor(value0, dtype=torch.float64))


def test_greedy_pick_rule():
    assert (CAMERA_COST, GUARD_COST) == (3, 5)
    v0 = [9.0] * 6
    t0 = [20] * 6
    # env 0: camera takes 3.0 (1.0 per point), guard takes 6.0 (1.2 per point): the guard
    # env 1: camera takes 3.0, guard takes 5.0 (1.0 each): the tie goes to the camera
    # env 2: the better guard blocks (ticks -1): the other guard, 0.8 per point, loses to the camera's 0.9
    # env 3: nothing lowers the value: none
    # env 4: as env 0 with 4 points left: the guard is not affordable
    # env 5: two cameras tie: the lowest index; the invalid candidate of lower value is not looked at
    cam = _scan([[1, 1, 1]] * 5 + [[0, 1, 1]], [[20, 20, 20]] * 6,
                [[8.0, 6.0, 7.0], [8.0, 6.0, 7.0], [8.0, 6.3, 7.0], [9.0, 9.5, 9.0], [8.0, 6.0, 7.0], [1.0, 6.0, 6.0]], t0, v0)
    grd = _scan([[1, 1]] * 6, [[20, 20], [20, 20], [-1, 20], [20, 20], [20, 20], [20, 20]],
                [[3.0, 8.0], [4.0, 8.0], [0.0, 5.0], [9.0, 9.25], [3.0, 8.0], [8.9, 8.9]], t0, v0)
    kind, index, gain = greedy_pick(cam, grd, [15, 15, 15, 15, 4, 15])
    assert kind.tolist() == [1, 0, 0, -1, 0, 0] and index.tolist() == [0, 1, 1, -1, 1, 1]
    assert gain.tolist() == [6.0 / 5, 3.0 / 3, (9.0 - 6.3) / 3, 0.0, 3.0 / 3, 3.0 / 3]
    assert kind.dtype == torch.int64 and index.dtype == torch.int64 and gain.dtype == torch.float64
    # nothing affordable; one kind alone; a mask that takes the winner out
    assert greedy_pick(cam, grd, 2)[0].tolist() == [-1] * 6
    assert greedy_pick(None, grd, 15)[0].tolist() == [1, 1, 1, -1, 1, 1]
    assert greedy_pick(cam, None, 3)[1].tolist() == [1, 1, 1, -1, 1, 1]
    g_ok = torch.ones((6, 2), dtype=torch.bool)
    g_ok[0, 0] = False
    kind, index, _ = greedy_pick(cam, grd, 15, guard_ok=g_ok)
    assert (int(kind[0]), int(index[0])) == (0, 1)
    # an unsolvable baseline has no eligible candidate
    dead = _scan([[1, 1]], [[-1, -1]], [[0.0, 0.0]], [-1], [0.5])
    assert greedy_pick(dead, None, 15)[0].tolist() == [-1]


# ---- the wrapper's argument checks that need no device

class _NoDevice:
    n_envs = 3
    _guard_candidates_arg = HeistEnv._guard_candidates_arg


def test_plan_place_guard_argument_checks():
    chk = _NoDevice()._guard_candidates_arg
    pa, me, fv = (torch.from_numpy(x) for x in gr.arrays(list(gr.PREMISE.values())))
    M = pa.shape[0]
    a, b, c = chk(pa, me, fv)                                  # [M, ...]: the same candidates on every env
    assert a.shape == (3, M, gr.P, 2) and b.shape == (3, M, 4) and c.shape == (3, M, 2)
    assert torch.equal(a[2], pa) and torch.equal(b[1], me) and torch.equal(c[0], fv)
    a, b, c = chk(pa.expand(3, -1, -1, -1), me.expand(3, -1, -1), fv.expand(3, -1, -1))
    assert a.shape == (3, M, gr.P, 2)
    a, _, _ = chk(np.zeros((M, 64, 2), np.int32), me, fv)      # P = 64
    assert a.shape == (3, M, 64, 2)
    bad = [(pa.long(), me, fv), (pa, me.long(), fv), (pa, me, fv.float()),               # dtypes
           (pa[:, :, :1], me, fv), (pa.reshape(M, gr.P * 2), me, fv),                    # paths' shape
           (torch.zeros((M, 65, 2), dtype=torch.int32), me, fv), (torch.zeros((M, 0, 2), dtype=torch.int32), me, fv),
           (pa, me[:, :3], fv), (pa, me[:-1], fv), (pa, me, fv[:, :1]), (pa, me, fv[1:]),
           (pa.expand(2, -1, -1, -1), me.expand(2, -1, -1), fv.expand(2, -1, -1)),       # N = 2 on a 3-env handle
           (pa.expand(3, -1, -1, -1), me, fv)]                                           # mixed ranks
    for args in bad:
        with pytest.raises(ValueError):
            chk(*args)


# ---- the library

def test_library_exports_plan_place_guard():
    if _build.needs_build():
        _build.build()
    lib = ctypes.CDLL(_build.LIB_PATH)
    names = {"heist_plan_place_guard", "heist_plan_place_guard_supported"}
    assert all(hasattr(lib, n) for n in names)
    assert names <= set(_native.header_functions()) and names <= set(_native.SIGNATURES)
    res, args = _native.SIGNATURES["heist_plan_place_guard"]
    assert res is ctypes.c_int and len(args) == 17
    assert args[:5] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int]
    assert all(a is ctypes.c_void_p for a in args[5:])
    assert _native.lib().heist_abi_version() == 5
    assert _native.lib().heist_plan_place_guard_supported(None) == -1  # a bad handle, before any device work
