"""heist_plan_walls without a GPU: the reference's own pinned answers (walls_ref: the C oracle on
layouts with their wall lists edited), the pure-torch edit builders, the derived fields of
WallAblation and WallScan on hand-made tensors, and the library's symbols."""
import ctypes

import numpy as np
import pytest
import torch

import plan_ref as pr
import walls_ref as wr
from heist_amd import _build, _native
from heist_amd.search import WallAblation, WallScan, wall_ablation_edits, wall_candidates


# ---- the fixture table, from the oracle alone

@pytest.mark.parametrize("name", sorted(wr.FIXTURES))
def test_fixture_table(name):
    """Ticks from oracle_search, the value at the start cell from the witness planes, == on the floats."""
    for edits, T, V, level in wr.rows(name):
        ref = wr.reference(name, edits, 1.0)
        got = (wr.ticks(name, edits), float(ref["value"][pr.START]), ref["level"])
        print("%s %r: %r" % (name, edits, got))
        assert got[0] == T, (name, edits)
        assert got[1] == V, (name, edits)
        assert got[2] == level, (name, edits)
    assert wr.rows(name)[0][1:3] == wr.BUILT[name]


def test_fixed_cam_critical_walls_first_action():
    for c in (1, 2, 3):
        assert int(wr.reference("fixed_cam", wr.rem(4, c), 1.0)["action"][pr.START]) == 2


def test_what_the_emitter_what_ifs_cannot_show():
    """A wall whose addition raises the value, a wall whose removal lowers it, a critical wall and a wall
    that cuts the level off."""
    v = lambda name, edits: float(wr.reference(name, edits, 1.0)["value"][pr.START])  # noqa: E731
    assert v("cam_guard", wr.add(6, 6)) > v("cam_guard", ())
    assert v("fixed_cam", wr.rem(4, 4)) < v("fixed_cam", ())
    assert wr.ticks("fixed_cam", ()) < 0 < wr.ticks("fixed_cam", wr.rem(4, 2))
    cut = wr.reference("cam_guard", wr.add(5, 5), 1.0)
    assert cut["level"] == 0 and cut["ticks"] == -1
    assert wr.reference("cam_guard", (), 1.0)["level"] == 1


def test_fixtures_fit_the_budget():
    """Every asset of every edited layout is bought: at a budget that drops one, the table would
    describe another layout."""
    for name in wr.FIXTURES:
        for edits, _, _, level in wr.rows(name):
            walls, cams, guards = wr.edited(wr.FIXTURES[name], edits)
            o = pr.po.OracleEnv(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, wr.BUDGET)
            assert bool(o.set_layout(walls, cams, guards)) == bool(level), (name, edits)
            i = o.info()
            assert (i["n_cams"], i["n_guards"]) == (len(cams), len(guards)), (name, edits)
            g = o.grid()
            for w in walls:
                assert g[w] == 1, (name, edits, w)
            assert int((g[1:-1, 1:-1] == 1).sum()) == len(walls), (name, edits)


def test_reference_cell_tables():
    """An added wall cell holds -1 / 0.0, a removed one a real value."""
    a = wr.reference("cam_guard", wr.add(6, 6), 1.0)
    assert int(a["togo"][6, 6]) == -1 and float(a["value"][6, 6]) == 0.0
    r = wr.reference("fixed_cam", wr.rem(4, 2), 1.0)
    assert int(r["togo"][4, 2]) > 0 and float(r["value"][4, 2]) > 0.0
    assert int(wr.reference("fixed_cam", (), 1.0)["togo"][4, 2]) == -1


def test_flood():
    w = np.zeros((5, 5), bool)
    w[0, :] = w[-1, :] = w[:, 0] = w[:, -1] = True
    assert wr.flood(w, (1, 1), (3, 3)) == 1
    w[2, 1:4] = True
    assert wr.flood(w, (1, 1), (3, 3)) == 0
    assert wr.flood(w, (1, 1), (1, 1)) == 1


# ---- wall_ablation_edits / wall_candidates

def _grids():
    g = torch.zeros((3, 5, 6), dtype=torch.int8)
    g[:, 0, :] = g[:, -1, :] = g[:, :, 0] = g[:, :, -1] = 1
    g[:, 1, 1], g[:, 3, 4] = 2, 3
    g[0, 2, 3] = g[0, 1, 4] = g[0, 3, 1] = 1        # three walls, given out of row-major order
    g[1, 2, 2] = 1                                   # one wall
    g[1, 2, 3], g[1, 1, 2] = 4, 5                    # a camera and a guard's start tile: not walls
    return g                                         # env 2: no interior wall


def test_wall_ablation_edits_order_and_padding():
    ed, filled = wall_ablation_edits(_grids(), 4)
    assert ed.dtype == torch.int32 and ed.shape == (3, 5, 1, 3) and ed.is_contiguous()
    assert filled.dtype == torch.bool and filled.tolist() == [[True, True, True, False], [True, False, False, False],
                                                             [False] * 4]
    assert ed[0, :, 0].tolist() == [[0, 0, 0], [1, 4, 2], [2, 3, 2], [3, 1, 2], [0, 0, 0]]  # row-major
    assert ed[1, :, 0].tolist() == [[0, 0, 0], [2, 2, 2], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert ed[2, :, 0].tolist() == [[0, 0, 0]] * 5
    # fewer columns than walls: the first ones in order; none at all: variant 0 alone
    ed2, f2 = wall_ablation_edits(_grids(), 2)
    assert ed2[0, :, 0].tolist() == [[0, 0, 0], [1, 4, 2], [2, 3, 2]] and f2[0].tolist() == [True, True]
    ed0, f0 = wall_ablation_edits(_grids(), 0)
    assert ed0.shape == (3, 1, 1, 3) and f0.shape == (3, 0)
    # more columns than interior cells
    edx, fx = wall_ablation_edits(_grids(), 20)
    assert edx.shape == (3, 21, 1, 3) and int(fx.sum()) == 4 and int((edx[:, :, 0, 2] == 2).sum()) == 4


def test_wall_ablation_edits_input_types():
    g = _grids()
    want = wall_ablation_edits(g, 4)
    for other in (g.to(torch.int32), g.numpy(), g.numpy().astype(np.int32), g.to(torch.int64)):
        got = wall_ablation_edits(other, 4)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError):
        wall_ablation_edits(g[0], 4)
    with pytest.raises(ValueError):
        wall_ablation_edits(g, -1)


def test_wall_candidates():
    cd = wall_candidates(_grids())
    assert cd.dtype == torch.int32 and cd.shape == (3, 12, 1, 3) and cd.is_contiguous()
    assert cd[0, :, 0].tolist() == [[r, c, 1] for r in range(1, 4) for c in range(1, 5)]
    assert torch.equal(cd[0], cd[2])
    with pytest.raises(ValueError):
        wall_candidates(torch.zeros((2, 2, 5), dtype=torch.int8))


# ---- WallAblation's derived fields

def _hand_made():
    """Four layouts with up to three walls.  Row 0: the cam_guard fixture's removals (4, 1..3).  Row 1: the
    fixed_cam fixture's (4, 2) critical, (4, 4) shielding, (4, 6) redundant.  Row 2: no wall.  Row 3: a wall
    whose removal changes the value's last bit only, and one that makes the way longer and cheaper."""
    nx = float(np.nextafter(10.0, 11.0))
    ticks = torch.tensor([[22, 22, 20, 19], [-1, 14, -1, -1], [16, 16, 16, 16], [20, 20, 22, 20]], dtype=torch.int16)
    value = torch.tensor([[11.940000000000001, 11.940000000000001, 12.09, 12.19],
                          [0.5714285714285716, 15.899999999999995, 0.3285714285714293, 0.5714285714285716],
                          [13.0, 13.0, 13.0, 13.0], [10.0, nx, 9.5, 10.0]], dtype=torch.float64)
    filled = torch.tensor([[1, 1, 1], [1, 1, 1], [0, 0, 0], [1, 1, 0]], dtype=torch.bool)
    return ticks, value, filled


def test_wall_ablation_fields():
    ticks, value, filled = _hand_made()
    ab = WallAblation.from_tables(ticks, value, filled)
    assert ab.ticks is ticks and ab.value is value and torch.equal(ab.filled, filled)
    assert ab.ticks_saved.tolist() == [[0, 2, 3], [0, 0, 0], [0, 0, 0], [0, -2, 0]]
    want = torch.where(filled, value[:, 1:] - value[:, :1], torch.zeros(4, 3, dtype=torch.float64))
    assert torch.equal(ab.credit, want) and ab.credit.dtype == torch.float64
    assert float(ab.credit[1, 1]) == 0.3285714285714293 - 0.5714285714285716 < 0  # signed
    assert ab.critical.tolist() == [[False] * 3, [True, False, False], [False] * 3, [False] * 3]
    assert ab.redundant.tolist() == [[True, False, False], [False, False, True], [False] * 3, [False] * 3]
    assert ab.shielding.tolist() == [[False] * 3, [False, True, False], [False] * 3, [False, True, False]]
    with pytest.raises(ValueError):
        WallAblation.from_tables(ticks[:, :3], value, filled)


def test_wall_ablation_metrics():
    ticks, value, filled = _hand_made()
    ab = WallAblation.from_tables(ticks, value, filled)
    m = ab.metrics()
    assert set(m) == {"critical_wall_layout_frac", "redundant_wall_frac", "shielding_wall_frac", "wall_credit_mean"}
    assert m["critical_wall_layout_frac"] == 1.0      # row 1 alone is unsolvable, and it has a critical wall
    assert m["redundant_wall_frac"] == 2 / 8
    assert m["shielding_wall_frac"] == 2 / 8
    assert m["wall_credit_mean"] == pytest.approx(float(ab.credit.sum()) / 8, rel=1e-15)
    # nothing to average: zeros, not NaN
    none = WallAblation.from_tables(ticks[2:3], value[2:3], filled[2:3]).metrics()
    assert list(none.values()) == [0.0] * 4
    empty = WallAblation.from_tables(ticks[:, :1], value[:, :1], filled[:, :0]).metrics()
    assert list(empty.values()) == [0.0] * 4


# ---- WallScan's eligibility rules

def _scan():
    """Three envs x five candidates.  Env 0 (solvable, value 10): c0 invalid with the lowest value, c1 cuts the
    level off, c2 helps, c3 blocks (level valid, ticks -1), c4 hurts a little.  Env 1 (unsolvable baseline):
    two eligible walls of one value.  Env 2: no valid candidate."""
    t, f = True, False
    valid = torch.tensor([[f, t, t, t, t], [t, t, f, f, f], [f] * 5])
    level = torch.tensor([[t, f, t, t, t], [t, t, t, t, t], [t] * 5])
    ticks = torch.tensor([[20, -1, 20, -1, 22], [-1, -1, -1, -1, -1], [20] * 5], dtype=torch.int16)
    value = torch.tensor([[1.0, 0.5, 11.0, 2.0, 9.0], [0.25, 0.25, 0.5, 0.5, 0.5], [10.0] * 5], dtype=torch.float64)
    action = torch.zeros((3, 5), dtype=torch.int8)
    return WallScan(valid, level, ticks, value, action, torch.tensor([20, -1, 20], dtype=torch.int16),
                    torch.tensor([10.0, 0.5, 10.0], dtype=torch.float64))


def test_wall_scan_eligibility():
    sc = _scan()
    assert sc.eligible().tolist() == [[False, False, True, True, True], [True, True, False, False, False], [False] * 5]
    # neither the invalid candidate nor the one that invalidates the level is a buy; ties go to the lowest index
    assert sc.best().tolist() == [3, 0, -1]
    assert sc.headroom().tolist() == [8.0, 0.25, 0.0]
    assert sc.helps().tolist() == [1 / 3, 0.0, 0.0]
    assert sc.blocking().tolist() == [1 / 3, 0.0, 0.0]          # env 1's baseline is unsolvable already
    assert sc.invalidating().tolist() == [1 / 4, 0.0, 0.0]
    m = sc.metrics()
    assert m["wall_headroom_envs"] == 2 and m["wall_headroom_mean"] == 8.25 / 2
    assert m["wall_blocking_frac"] == (1 / 3) / 2               # over the two envs whose baseline is solvable
    assert m["wall_helps_frac"] == (1 / 3) / 3 and m["wall_invalidating_frac"] == (1 / 4) / 3


def test_wall_scan_nothing_to_average():
    sc = _scan()
    none = WallScan(torch.zeros_like(sc.valid), sc.level, sc.ticks, sc.value, sc.action,
                    torch.full_like(sc.ticks0, -1), sc.value0)
    m = none.metrics()
    assert m == {"wall_headroom_mean": 0.0, "wall_blocking_frac": 0.0, "wall_helps_frac": 0.0,
                 "wall_invalidating_frac": 0.0, "wall_headroom_envs": 0}


# ---- the library

def test_library_exports_plan_walls():
    if _build.needs_build():
        _build.build()
    lib = ctypes.CDLL(_build.LIB_PATH)
    assert hasattr(lib, "heist_plan_walls") and hasattr(lib, "heist_plan_walls_supported")
    assert {"heist_plan_walls", "heist_plan_walls_supported"} <= set(_native.header_functions())
    assert {"heist_plan_walls", "heist_plan_walls_supported"} <= set(_native.SIGNATURES)
    assert len(_native.SIGNATURES["heist_plan_walls"][1]) == 16
    assert _native.lib().heist_abi_version() == 5
    assert _native.lib().heist_plan_walls_supported(None) == -1  # a bad handle, before any device work
