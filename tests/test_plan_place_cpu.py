"""heist_plan_place without a GPU: the premise the kernel rests on, checked with the C oracle alone
(the visibility of a layout plus a camera is the layout's own OR the camera's alone against the same
walls), the pure-torch candidate builder and PlacementScan's derived fields on hand-made tensors,
and the library's symbols."""
import ctypes

import numpy as np
import pytest
import torch

import place_ref as plr
import plan_ref as pr
from heist_amd import _build, _native
from heist_amd.search import PlacementScan, camera_candidates


# ---- the union premise

@pytest.mark.parametrize("i", range(len(plr.PREMISE)))
def test_union_premise(i):
    c = plr.PREMISE[i]
    assert plr.expect_valid(c)
    base, walls = plr.planes_of("base")
    plus, walls_plus = plr.planes_of(("plus", c))
    own, walls_own = plr.planes_of(("alone", c))
    assert (walls == walls_plus).all() and (walls == walls_own).all(), "a camera changes no wall"
    assert len(base) == len(plus) == len(own) == pr.MAX_STEPS
    for k in range(pr.MAX_STEPS):
        assert ((base[k] | own[k]) == plus[k]).all(), "tick %d of %r" % (k + 1, c)
    assert any((plus[k] != base[k]).any() for k in range(pr.MAX_STEPS)), "the candidate sees something new"
    # the recurrence on those planes, at the start cell, is the oracle search's answer
    T = plr.search(c)[0]
    print(c, "ticks", T)
    assert plr.reference(c, 1.0)["ticks"] == T
    base_ref = plr.reference(None, 1.0)
    assert base_ref["ticks"] == 22 and (T < 0 or T >= 22)


@pytest.mark.parametrize("name", ["camera_tile", "wall", "border"])
def test_rejected_candidate_is_the_base(name):
    c = plr.INVALID[name]
    assert plr.oracle_shown(c) and not plr.expect_valid(c)
    assert plr.bought(plr.with_cand(plr.BASE, c)) == (1, 1)
    base, walls = plr.planes_of("base")
    plus, walls_plus = plr.planes_of(("plus", c))
    assert (walls == walls_plus).all()
    for k in range(pr.MAX_STEPS):
        assert (base[k] == plus[k]).all(), "tick %d" % (k + 1)


def test_validity_table():
    assert all(plr.expect_valid(c) for c in plr.VALID)
    assert not any(plr.expect_valid(c) for c in plr.INVALID.values())
    # the one divergence: the oracle's purchase would take a camera on the guard's start tile
    assert plr.bought(plr.with_cand(plr.BASE, plr.INVALID["guard_start"])) == (2, 1)
    assert plr.bought(plr.with_cand(plr.BASE, plr.INVALID["start"])) == (1, 1)
    assert plr.bought(plr.with_cand(plr.BASE, plr.INVALID["vault"])) == (1, 1)
    # an invalid candidate's reference is the baseline's own object
    assert plr.reference(plr.INVALID["wall"], 0.99)["planes"] is plr.reference(None, 0.99)["planes"]
    blind = plr.reference(plr.BLIND, 0.99)
    base = plr.reference(None, 0.99)
    assert blind["valid"] and all((a == b).all() for a, b in zip(blind["planes"], base["planes"]))


# ---- camera_candidates

def test_camera_candidates_order_and_count():
    grid = torch.zeros((3, 5, 6), dtype=torch.int8)
    hd = [0.0, 90.0, 225.0]
    cd = camera_candidates(grid, hd, 60.0, 15.0, 6)
    assert cd.shape == (3, 3 * 4 * 3, 6) and cd.dtype == torch.float64 and cd.is_contiguous()
    want = [[float(r), float(c), 60.0, h, 15.0, 6.0] for r in range(1, 4) for c in range(1, 5) for h in hd]
    for e in range(3):
        assert cd[e].tolist() == want
    seen = {(int(v[0]), int(v[1]), v[3]) for v in cd[0].tolist()}
    assert seen == {(r, c, h) for r in range(1, 4) for c in range(1, 5) for h in hd}
    # what stands on a cell does not change the list: the kernel's valid flag tells
    grid[1, 2, 3] = 1
    assert torch.equal(camera_candidates(grid, hd, 60.0, 15.0, 6), cd)
    one = camera_candidates(np.zeros((1, 3, 3), np.int8), torch.tensor([45.0]), 30.0, -5.0, 4)
    assert one.tolist() == [[[1.0, 1.0, 30.0, 45.0, -5.0, 4.0]]]
    with pytest.raises(ValueError):
        camera_candidates(torch.zeros((5, 6), dtype=torch.int8), hd, 60.0, 15.0, 6)
    with pytest.raises(ValueError):
        camera_candidates(grid, [], 60.0, 15.0, 6)


# ---- PlacementScan's derived fields

def _hand_made():
    """Five envs, four candidates.  Row 0: a tie for the lowest value between candidates 1 and 3,
    candidate 2 lower still but blocking.  Row 1: nothing valid.  Row 2: an unsolvable baseline.
    Row 3: the only eligible candidate raises the value.  Row 4: every valid candidate blocks."""
    valid = torch.tensor([[1, 1, 1, 1], [0, 0, 0, 0], [1, 1, 0, 1], [0, 1, 0, 0], [1, 0, 1, 0]], dtype=torch.bool)
    ticks = torch.tensor([[22, 24, -1, 30], [18, 18, 18, 18], [-1, -1, -1, -1], [20, 21, 20, 20], [-1, 16, -1, 16]],
                         dtype=torch.int16)
    value = torch.tensor([[9.0, 8.5, 0.25, 8.5], [9.5, 9.5, 9.5, 9.5], [0.5, 0.5, 0.5, 0.5], [7.0, 7.5, 1.0, 1.0],
                          [0.5, 9.0, 0.25, 9.0]], dtype=torch.float64)
    action = torch.zeros((5, 4), dtype=torch.int8)
    ticks0 = torch.tensor([22, 18, -1, 20, 16], dtype=torch.int16)
    value0 = torch.tensor([9.75, 9.5, 0.5, 7.0, 9.0], dtype=torch.float64)
    return PlacementScan(valid, ticks, value, action, ticks0, value0)


def test_placement_scan_fields():
    sc = _hand_made()
    assert sc.best().tolist() == [1, -1, -1, 1, -1] and sc.best().dtype == torch.int64
    assert sc.headroom().tolist() == [9.75 - 8.5, 0.0, 0.0, 7.0 - 7.5, 0.0]
    assert sc.blocking().tolist() == [0.25, 0.0, 0.0, 0.0, 1.0]
    m = sc.metrics()
    assert set(m) == {"camera_headroom_mean", "camera_blocking_frac", "camera_headroom_envs"}
    assert m["camera_headroom_envs"] == 2
    assert m["camera_headroom_mean"] == (1.25 + -0.5) / 2
    assert m["camera_blocking_frac"] == (0.25 + 0.0 + 0.0 + 1.0) / 4   # rows 0, 1, 3, 4 have a solvable baseline
    none = PlacementScan(sc.valid[1:3], sc.ticks[1:3], sc.value[1:3], sc.action[1:3], sc.ticks0[2:3].expand(2),
                         sc.value0[1:3]).metrics()
    assert none == {"camera_headroom_mean": 0.0, "camera_blocking_frac": 0.0, "camera_headroom_envs": 0}


# ---- the library

def test_library_exports_plan_place():
    if _build.needs_build():
        _build.build()
    lib = ctypes.CDLL(_build.LIB_PATH)
    names = {"heist_plan_place", "heist_plan_place_supported"}
    assert all(hasattr(lib, n) for n in names)
    assert names <= set(_native.header_functions()) and names <= set(_native.SIGNATURES)
    assert len(_native.SIGNATURES["heist_plan_place"][1]) == 14
    assert _native.lib().heist_abi_version() == 5
    assert _native.lib().heist_plan_place_supported(None) == -1  # a bad handle, before any device work
