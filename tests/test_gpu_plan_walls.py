"""heist_plan_walls (HeistEnv.plan_walls / plan_wall_ablate): every env planned with walls added or
removed, M variants in one launch -- whether the edits hold, whether the level is still valid, the
fewest ticks, the optimal return and first action from the Solver's cell, every variant's visibility
planes and the whole tick-0 tables.  Every comparison is equality, float64 through its bits (int64).

Yardsticks, none of which uses the kernel under test: walls_ref (the C oracle on layouts with their
wall lists edited, and the NumPy recurrences on its witness planes); heist_plan_field /
heist_plan_value on twin handles built from the edited layouts; heist_plan_masked on the same handle
for the variants without an edit.
"""
import numpy as np
import pytest
import torch

import masked_ref as mr
import plan_ref as pr
import value_ref as vr
import walls_ref as wr
from heist_amd import (EnvironmentConfig, HeistEnv, PlanWalls, WallAblation, WallScan, _native as nat, greedy_walls,
                       wall_ablation_edits, wall_candidates, wall_placement_scan)
from heist_amd.layouts import synthetic_layouts
from heist_amd.obs_compact import record_words

pytestmark = pytest.mark.gpu

HEIST_EINVAL = 100000
MC, MG, MP = 5, 3, 16
NAMES = sorted(wr.FIXTURES)
G, H = pr.GRID, pr.MAX_STEPS
SR, SC = pr.START
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def _cfg(R, C, max_steps, start=(1, 1)):
    return EnvironmentConfig(grid_rows=R, grid_cols=C, max_steps=max_steps, start_pos=start, architect_budget=C + 10)


def _make(n, cfg, dev, cones=True, mc=MC, mg=MG):
    env = HeistEnv(n, cfg, max_cams=mc, max_guards=mg, max_path=MP, device=dev, auto_reset=False)
    env.set_guard_cones(cones)
    return env


def _set(env, lays, budget, level=None):
    """Layouts set and reset, every emitter of every layout bought; level: the expected BFS validity."""
    valid = env.set_layouts(lays, budget=budget)
    env.reset()
    x = env.export(grid=True)
    assert valid.tolist() == ([True] * len(lays) if level is None else [bool(v) for v in level])
    assert x["n_cams"].tolist() == [len(l[1]) for l in lays] and x["n_guards"].tolist() == [len(l[2]) for l in lays]
    return x


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _edits(rows, E):
    """[N][M] tuples of (row, col, op) -> int32 [N, M, E, 3], op 0 beyond a variant's own."""
    return torch.tensor([[wr.edit_rows(ed, E) for ed in row] for row in rows], dtype=torch.int64).to(torch.int32)


def _planes(pw, e, m):
    return torch.stack([pw.vis_mask(k, m)[e] for k in range(1, pw.vis.shape[0] + 1)]).cpu().numpy()


def _check_padding(pw, HK):
    """Bits past R C and words past ceil(R C / 32) are 0; rows >= HK[e] are 0."""
    RC = pw.rows * pw.cols
    words = pw.vis.cpu().numpy().view(np.uint32)  # [H, N, M, W]
    nvis = (RC + 31) // 32
    assert not words[..., nvis:].any(), "words past ceil(RC/32) must be 0"
    if RC % 32:
        assert not (words[..., nvis - 1] >> (RC % 32)).any(), "bits past RC must be 0"
    for e, hk in enumerate(HK):
        assert not words[hk:, e].any(), "env %d: vis rows >= HK must be 0" % e


def _assert_ref(pw, i, m, ref, what):
    assert int(pw.ticks[i, m]) == ref["ticks"], what
    assert vr.bits(float(pw.value[i, m])) == vr.bits(ref["value"][pr.START]), what
    assert int(pw.action[i, m]) == int(ref["action"][pr.START]), what
    assert int(pw.level[i, m]) == ref["level"], what
    np.testing.assert_array_equal(pw.togo[i, m].cpu().numpy(), ref["togo"], what)
    np.testing.assert_array_equal(vr.bits(pw.value_cells[i, m].cpu().numpy()), vr.bits(ref["value"]), what)
    got = _planes(pw, i, m)
    diff = [k + 1 for k in range(got.shape[0]) if (got[k] != ref["planes"][k]).any()]
    assert not diff, "%s: vis differs from the witnesses first at tick %d" % (what, diff[0])


def _assert_twin(pw, e, m, pf, pv, i, pos, what):
    """Variant (e, m) == plan_field / plan_value of env i of a twin handle, the Solver on pos."""
    r, c = pos
    assert torch.equal(pw.togo[e, m], pf.togo[i]), what
    assert _same(pw.value_cells[e, m], pv.value[i]), what
    assert int(pw.ticks[e, m]) == int(pf.togo[i, r, c]) and _same(pw.value[e, m], pv.value[i, r, c]), what
    assert int(pw.action[e, m]) == int(pv.action[i, r, c]), what
    assert torch.equal(pw.vis[:, e, m], pf.vis[:, i]) and torch.equal(pf.vis[:, i], pv.vis[:, i]), what


def _assert_masked(pw, pm, what, cols=None):
    """Every variant (or those of cols) == plan_masked's of the same index."""
    s = slice(None) if cols is None else cols
    assert torch.equal(pw.ticks[:, s], pm.ticks[:, s]) and _same(pw.value[:, s], pm.value[:, s]), what
    assert torch.equal(pw.action[:, s], pm.action[:, s]) and torch.equal(pw.vis[:, :, s], pm.vis[:, :, s]), what
    if pw.togo is not None:
        assert torch.equal(pw.togo[:, s], pm.togo_cells[:, s]) and _same(pw.value_cells[:, s], pm.value_cells[:, s]), what


def _fixture_env(dev, cones=True, mc=MC, mg=MG, names=NAMES):
    env = _make(len(names), _cfg(G, G, H), dev, cones, mc, mg)
    _set(env, [wr.FIXTURES[n] for n in names], wr.BUDGET)
    return env


def _table_rows():
    """[N][M] edits: every row of walls_ref.TABLE, padded with the layout as built."""
    M = max(len(wr.rows(n)) for n in NAMES)
    return [([r[0] for r in wr.rows(n)] + [()] * M)[:M] for n in NAMES]


# ---- 1. the fixture table against the oracle on the edited layouts, and against twin handles

@pytest.mark.parametrize("cones", [True, False], ids=["cached_guards", "live_guards"])
@pytest.mark.parametrize("waves", [1, 2, 4])
def test_fixture_table(gpu_device, monkeypatch, waves, cones):
    monkeypatch.setenv("HEIST_MULTI_WAVES", str(waves))
    env = _fixture_env(gpu_device, cones)
    kc = env.kernel_config()
    assert kc["multi_waves"] == waves and kc["guard_cones"] == (1 if cones else 0) and env.plan_walls_supported == 1
    rows = _table_rows()
    ed = _edits(rows, 1)
    N, M, W = len(NAMES), ed.shape[1], record_words(G, G)
    pw = env.plan_walls(ed, gamma=1.0, cells=True)
    assert isinstance(pw, PlanWalls) and pw.gamma == 1.0 and torch.equal(pw.edits.cpu(), ed) and pw.masks is None
    assert pw.valid.shape == (N, M) and pw.valid.dtype == torch.bool and pw.level.shape == (N, M)
    assert pw.level.dtype == torch.bool
    assert pw.ticks.shape == (N, M) and pw.ticks.dtype == torch.int16
    assert pw.value.shape == (N, M) and pw.value.dtype == torch.float64
    assert pw.action.shape == (N, M) and pw.action.dtype == torch.int8
    assert pw.vis.shape == (H, N, M, W) and pw.vis.dtype == torch.int32
    assert pw.togo.shape == (N, M, G, G) and pw.togo.dtype == torch.int16
    assert pw.value_cells.shape == (N, M, G, G) and pw.value_cells.dtype == torch.float64
    assert pw.tick.tolist() == [0] * N and bool(pw.valid.all())
    for i, n in enumerate(NAMES):
        for m, edits in enumerate(rows[i]):
            ref = wr.reference(n, edits, 1.0)
            print("%s %r: ticks %d value %r level %d" % (n, edits, int(pw.ticks[i, m]), float(pw.value[i, m]),
                                                        int(pw.level[i, m])))
            _assert_ref(pw, i, m, ref, "%s %r" % (n, edits))
            for r, c, op in edits:  # an added wall cell holds -1 / 0.0, a removed one a real value
                if op == wr.ADD:
                    assert int(pw.togo[i, m, r, c]) == -1 and float(pw.value_cells[i, m, r, c]) == 0.0
                elif int(pw.ticks[i, m]) > 0:
                    assert int(pw.togo[i, m, r, c]) > 0
        # the pinned table, on the GPU's own numbers
        for m, (edits, T, V, level) in enumerate(wr.rows(n)):
            assert (int(pw.ticks[i, m]), float(pw.value[i, m]), int(pw.level[i, m])) == (T, V, level), (n, edits)
    _check_padding(pw, [H] * N)
    # the level-valid variants against twin handles built from the edited layouts, at another gamma too
    for gamma in (1.0, 0.99):
        pg = pw if gamma == 1.0 else env.plan_walls(ed, gamma=gamma, cells=True)
        for i, n in enumerate(NAMES):
            ms = [m for m, edits in enumerate(rows[i]) if wr.reference(n, edits, 1.0)["level"]]
            twin = _make(len(ms), _cfg(G, G, H), gpu_device, cones)
            _set(twin, [wr.edited(wr.FIXTURES[n], rows[i][m]) for m in ms], wr.BUDGET)
            pf, pv = twin.plan_field(), twin.plan_value(gamma=gamma)
            for j, m in enumerate(ms):
                _assert_twin(pg, i, m, pf, pv, j, pr.START, "%s %r gamma %r" % (n, rows[i][m], gamma))
            twin.close()
    lean = env.plan_walls(ed, gamma=1.0)
    assert lean.togo is None and lean.value_cells is None
    assert torch.equal(lean.ticks, pw.ticks) and _same(lean.value, pw.value) and torch.equal(lean.vis, pw.vis)
    env.close()


# ---- 2. twin handles at other shapes: 1-, 2- and 8-edit variants, adds and removes mixed

@pytest.mark.parametrize("cones", [True, False], ids=["twin_cached", "twin_live"])
@pytest.mark.parametrize("name", sorted(wr.SHAPES))
def test_twin_handles(gpu_device, name, cones):
    R, C, max_steps, nc, ng, budget = wr.SHAPES[name]
    case = wr.shape_case(name)
    cfg, hz = _cfg(R, C, max_steps), min(max_steps, 60)
    env = _make(2, cfg, gpu_device)
    x = _set(env, case["layouts"], budget)
    assert env.kernel_config()["guard_cones"] == 1
    for e in range(2):  # the CPU grid the variants were drawn on is the handle's
        np.testing.assert_array_equal(x["grid"][e].cpu().numpy(), case["grids"][e])
    ed = _edits(case["edits"], case["E"])
    assert [[len(v) for v in row] for row in case["edits"]] == [[1, 2, 8, 1]] * 2
    twin = _make(8, cfg, gpu_device, cones)
    _set(twin, [wr.edited(case["layouts"][e], v) for e in range(2) for v in case["edits"][e]], budget + wr.SLACK)
    for gamma in (1.0, 0.99):
        pw = env.plan_walls(ed, horizon=hz, gamma=gamma, cells=True)
        assert bool(pw.valid.all()) and bool(pw.level.all())
        pf, pv = twin.plan_field(horizon=hz), twin.plan_value(horizon=hz, gamma=gamma)
        for e in range(2):
            for m in range(4):
                _assert_twin(pw, e, m, pf, pv, 4 * e + m, (1, 1), "%s env %d variant %d gamma %r" % (name, e, m, gamma))
        _check_padding(pw, [hz] * 2)
    base = env.plan_field(horizon=hz)
    changed = sum(int(not torch.equal(pw.vis[:, e, m], base.vis[:, e])) for e in range(2) for m in range(4))
    print(name, "variants whose planes differ from the layout's:", changed)
    assert changed >= 2  # the walls matter to the rays
    env.close()
    twin.close()


# ---- 3. variants without an edit, invalid variants, masks

@pytest.mark.parametrize("cones", [True, False], ids=["cached_guards", "live_guards"])
def test_no_edit_and_invalid_equal_plan_masked(gpu_device, cones):
    names = ["cam_guard", "two_cams_guard"]
    env = _make(2, _cfg(G, G, H), gpu_device, cones)
    _set(env, [mr.FIXTURES[n] for n in names], mr.BUDGET)
    ons = [mr.variants(n)[:4] for n in names]
    masks = torch.tensor([[mr.mask_word(on, MC) for on in row] for row in ons], dtype=torch.int64)
    pm = env.plan_masked(masks, gamma=0.99, cells=True)
    none = torch.zeros((2, 4, 2, 3), dtype=torch.int32)
    none[:, :, :, :2] = torch.tensor([I32_MAX, I32_MIN], dtype=torch.int64).to(torch.int32)  # op 0: row and col are ignored
    pw = env.plan_walls(none, masks=masks, gamma=0.99, cells=True)
    assert bool(pw.valid.all()) and bool(pw.level.all()) and torch.equal(pw.masks.cpu(), masks)
    _assert_masked(pw, pm, "no edit")
    bad = none.clone()
    bad[:, :, 0] = torch.tensor([0, 3, 1], dtype=torch.int32)  # a wall on the border
    bad[:, :, 1] = torch.tensor([6, 6, 1], dtype=torch.int32)  # with a good edit beside it: none is applied
    pb = env.plan_walls(bad, masks=masks, gamma=0.99, cells=True)
    assert not bool(pb.valid.any()) and bool(pb.level.all())
    _assert_masked(pb, pm, "invalid")
    # masks=None is every slot live
    pa = env.plan_walls(none[:, :1], gamma=0.99, cells=True)
    _assert_masked(pa, pm, "no mask", cols=slice(0, 1))
    # a camera switched off and a wall added, in one variant: the twin has neither the camera nor a gap there
    off = torch.tensor([[mr.mask_word(((0,), (1,)), MC)], [mr.mask_word(((0, 1), (1,)), MC)]], dtype=torch.int64)
    both = env.plan_walls(_edits([[wr.add(6, 6)]] * 2, 1), masks=off, gamma=0.99, cells=True)
    twin = _make(2, _cfg(G, G, H), gpu_device, cones)
    lays = [mr.reduced(mr.FIXTURES["cam_guard"], ((0,), (1,))), mr.reduced(mr.FIXTURES["two_cams_guard"], ((0, 1), (1,)))]
    _set(twin, [wr.edited(l, wr.add(6, 6)) for l in lays], mr.BUDGET)
    pf, pv = twin.plan_field(), twin.plan_value(gamma=0.99)
    for e in range(2):
        _assert_twin(both, e, 0, pf, pv, e, pr.START, "camera off + wall, env %d" % e)
    assert bool(both.valid.all()) and not torch.equal(both.vis[:, :, 0], pm.vis[:, :, 1])
    env.close()
    twin.close()


# ---- 4. mid-episode state, horizons, a done env, the Solver on the add tile

def test_mid_episode_and_horizons(gpu_device):
    layout, plan = wr.FIXTURES["cam_guard"], pr.CASES["wallrow_both"][3]  # the layout's canonical plan, 22 ticks
    seen_at_once = ([], [{"row": 1, "col": 4, "fov_angle": 60.0, "vision_range": 6, "heading": 180.0,
                          "rotation_speed": 0.0}], [])             # looks along row 1 at the start: done on tick 1
    # adds only: a wall takes rays away and leaves the patrol alone, so the prefix stays unseen in every twin; the
    # prefix (1, 1) -> (1, 3) -> (3, 3) touches none of the tiles
    variants = [wr.add(6, 6), wr.add(7, 5), wr.add(6, 6) + wr.add(6, 4), wr.add(3, 3), ()]
    k = 7
    env = _make(2, _cfg(G, G, H), gpu_device)
    _set(env, [layout, seen_at_once], wr.BUDGET)
    twin = _make(3, _cfg(G, G, H), gpu_device)
    _set(twin, [wr.edited(layout, v) for v in variants[:3]], wr.BUDGET)
    acts = torch.tensor(plan[:k], device=gpu_device).reshape(-1, 1)
    env.step_multi(acts.expand(k, 2).contiguous(), auto_reset=False)
    twin.step_multi(acts.expand(k, 3).contiguous(), auto_reset=False)
    x, tx = env.export(), twin.export()
    assert x["tick"].tolist()[0] == k and x["done"].tolist() == [0, 1] and tx["done"].tolist() == [0, 0, 0]
    pos = (int(x["pos_r"][0]), int(x["pos_c"][0]))
    assert pos == (3, 3) and tx["pos_r"].tolist() == [3] * 3 and tx["pos_c"].tolist() == [3] * 3
    ed = _edits([variants, variants], 2)
    before = env.save_state().blobs.clone()
    for hz in (5, H):  # shorter and longer than the 33 ticks left
        pw = env.plan_walls(ed, horizon=hz, gamma=0.99, cells=True)
        assert pw.tick.tolist() == [k, -1] and pw.vis.shape[0] == hz
        pf, pv = twin.plan_field(horizon=hz), twin.plan_value(horizon=hz, gamma=0.99)
        for m in range(3):
            _assert_twin(pw, 0, m, pf, pv, m, pos, "after %d ticks, horizon %d, variant %d" % (k, hz, m))
        # the Solver stands on (3, 3): not placeable, and the variant is the one without an edit
        assert pw.valid[0].tolist() == [True, True, True, False, True]
        pm = env.plan_masked(torch.full((2, 1), -1, dtype=torch.int64), horizon=hz, gamma=0.99, cells=True)
        for m in (3, 4):
            assert torch.equal(pw.togo[0, m], pm.togo_cells[0, 0]) and _same(pw.value_cells[0, m], pm.value_cells[0, 0])
            assert torch.equal(pw.vis[:, 0, m], pm.vis[:, 0, 0]) and int(pw.ticks[0, m]) == int(pm.ticks[0, 0])
        # the env already done: valid and level are answered all the same, no plan, nothing to collect, no rows
        assert pw.valid[1].tolist() == [True] * 5 and pw.level[1].tolist() == [True] * 5
        assert pw.ticks[1].tolist() == [-1] * 5 and not _bits(pw.value[1]).any() and pw.action[1].tolist() == [-1] * 5
        assert not pw.vis[:, 1].any() and bool((pw.togo[1] == -1).all()) and not _bits(pw.value_cells[1]).any()
        _check_padding(pw, [min(hz, H - k), 0])
    assert int(pw.ticks[0, 4]) == len(plan) - k
    assert torch.equal(env.save_state().blobs, before)
    env.close()
    twin.close()


# ---- 5. the validity table, with guard bands around every output

BAND = 64


def _banded(n, dtype, dev, fill):
    t = torch.full((n + 2 * BAND,), fill, dtype=dtype, device=dev)
    return t, t[BAND:BAND + n]


def test_validity_table(gpu_device):
    """Every row is invalid, leaves the unedited plan and writes nothing outside the outputs."""
    env = _make(1, _cfg(G, G, H), gpu_device)
    _set(env, [wr.FIXTURES["cam_guard"]], wr.BUDGET)
    big = (I32_MAX, I32_MIN, -I32_MAX, -1)
    rows = [[(0, 3, 1)], [(9, 9, 1)], [(3, 0, 1)], [(3, 9, 1)],           # the border
            [(1, 1, 1)], [(8, 8, 1)],                                     # start (the Solver's cell too), vault
            [(6, 5, 1)], [(6, 5, 2)],                                     # the camera's tile
            [(5, 2, 1)], [(5, 2, 2)],                                     # the guard's start tile: kGuard
            [(4, 1, 1)],                                                  # a wall on a wall
            [(2, 2, 2)],                                                  # an EMPTY tile removed
            [(0, 3, 2)], [(9, 0, 2)], [(4, 9, 2)],                        # a border tile removed
            [(6, 6, 3)], [(6, 6, -1)], [(6, 6, I32_MAX)], [(6, 6, I32_MIN)], [(4, 2, 3)]]  # ops outside 0..2
    rows += [[(v, 3, op)] for v in big for op in (1, 2)] + [[(3, v, op)] for v in big for op in (1, 2)]
    rows += [[(v, v, 1)] for v in big]
    rows += [[(6, 6, 1), (6, 6, 1)], [(6, 6, 1), (6, 6, 2)], [(4, 2, 2), (4, 2, 2)], [(4, 2, 2), (4, 2, 1)]]  # one tile twice
    rows += [[(6, 6, 1), (0, 0, 1)], [(0, 0, 2), (4, 2, 2)]]              # a good edit beside a bad one: none applied
    n_bad = len(rows)
    rows += [[(6, 6, 1), (I32_MAX, I32_MIN, 0)], [(I32_MIN, 6, 0), (4, 2, 2)], [(6, 6, 1), (4, 2, 2)]]  # controls: valid
    M, E, hz = len(rows), 2, 30
    ed = torch.tensor([wr.edit_rows(r, E) for r in rows], dtype=torch.int64).to(torch.int32).reshape(1, M, E, 3)
    W, RC = record_words(G, G), G * G
    dev = gpu_device
    edb, edv = _banded(M * E * 3, torch.int32, dev, 7)
    edv.copy_(ed.reshape(-1).to(dev))
    vb, valid = _banded(M, torch.uint8, dev, 0xA5)
    lb, level = _banded(M, torch.uint8, dev, 0xA5)
    tb, ticks = _banded(M, torch.int16, dev, 0x5A5A)
    ub, value = _banded(M, torch.float64, dev, -7.25)
    ab, action = _banded(M, torch.int8, dev, 0x5A)
    sb, vis = _banded(hz * M * W, torch.int32, dev, 0x5A5A5A5A)
    cb, tcells = _banded(M * RC, torch.int16, dev, 0x5A5A)
    db, vcells = _banded(M * RC, torch.float64, dev, -7.25)
    bands = [(edb, 7), (vb, 0xA5), (lb, 0xA5), (tb, 0x5A5A), (ub, -7.25), (ab, 0x5A), (sb, 0x5A5A5A5A), (cb, 0x5A5A),
             (db, -7.25)]
    assert vis.data_ptr() % 16 == 0 and value.data_ptr() % 8 == 0 and vcells.data_ptr() % 8 == 0
    before = env.save_state().blobs.clone()
    rc = nat.lib().heist_plan_walls(env._h, hz, 0.99, M, E, nat.ptr(edv), None, nat.ptr(valid), nat.ptr(level),
                                    nat.ptr(ticks), nat.ptr(value), nat.ptr(action), nat.ptr(vis), nat.ptr(tcells),
                                    nat.ptr(vcells), env._stream())
    assert rc == 0
    torch.cuda.synchronize(gpu_device)
    for t, fill in bands:  # nothing outside the outputs, and the edits as given
        assert bool((t[:BAND] == fill).all()) and bool((t[-BAND:] == fill).all())
    assert torch.equal(edv.cpu(), ed.reshape(-1))
    assert torch.equal(env.save_state().blobs, before)
    assert valid.tolist() == [0] * n_bad + [1] * 3
    assert level.tolist() == [1] * M
    pm = env.plan_masked(torch.full((1, 1), -1, dtype=torch.int64), horizon=hz, gamma=0.99, cells=True)
    vis4, tc, vc = vis.reshape(hz, 1, M, W), tcells.reshape(M, G, G), vcells.reshape(M, G, G)
    for m in range(n_bad):
        what = "row %r" % (rows[m],)
        assert int(ticks[m]) == int(pm.ticks[0, 0]) and _same(value[m], pm.value[0, 0]), what
        assert int(action[m]) == int(pm.action[0, 0]) and torch.equal(vis4[:, 0, m], pm.vis[:, 0, 0]), what
        assert torch.equal(tc[m], pm.togo_cells[0, 0]) and _same(vc[m], pm.value_cells[0, 0]), what
    assert not torch.equal(vis4[:, 0, n_bad], pm.vis[:, 0, 0])                    # the controls are applied
    assert int(tc[n_bad, 6, 6]) == -1 and int(tc[n_bad + 1, 4, 2]) != int(pm.togo_cells[0, 0, 4, 2]) == -1
    assert int(tc[n_bad + 2, 6, 6]) == -1 and int(tc[n_bad + 2, 4, 2]) != -1
    env.close()


# ---- 6. the launch only reads the env

def test_plan_walls_reads_only(gpu_device, monkeypatch):
    """64 lean-served 20 x 20 envs with the shared fan table in use: the saved state of all envs is
    byte-equal before and after plan_walls(), and the next 20-tick heist_step_multi_records launch
    is bit-identical to a twin's that never called it."""
    monkeypatch.setenv("HEIST_MULTI_WAVES", "1")
    n, R, budget, K = 64, 20, 15, 20
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=R, max_steps=200)
    lays = synthetic_layouts(n, R, R, budget, seed=43)
    gen = torch.Generator().manual_seed(5)
    acts = torch.randint(0, 5, (4 + K, n), generator=gen).to(gpu_device)
    envs = []
    for i in range(2):
        env = HeistEnv(n, cfg, max_cams=MC, max_guards=MG, max_path=MP, device=gpu_device, auto_reset=True)
        kc = env.kernel_config()
        assert kc["lean"] == 1 and kc["multi_waves"] == 1, kc
        env.set_layouts(lays, budget=budget)
        env.reset()
        env.step_multi(acts[:4])  # leaves the fan table's position mid-table
        envs.append(env)
    a, b = envs
    before = a.save_state().blobs.clone()
    ed = torch.cat([wall_candidates(a.grid_snapshot())[:, 100:104], wall_ablation_edits(a.grid_snapshot(), 4)[0][:, 1:]], 1)
    pw = a.plan_walls(ed, horizon=50, gamma=0.99)
    assert bool(pw.valid.any()) and bool(pw.vis.any()) and bool((pw.edits[:, :, 0, 2] == 2).any())
    assert torch.equal(a.save_state().blobs, before)
    out_a = a.step_multi_records(acts[4:], reward64=True)
    out_b = b.step_multi_records(acts[4:], reward64=True)
    for u, v in zip(out_a, out_b):
        assert torch.equal(u, v)
    assert torch.equal(a.save_state().blobs, b.save_state().blobs)
    a.close()
    b.close()


# ---- 7. arguments

def _einval(fn):
    with pytest.raises(nat.HeistError) as ei:
        fn()
    assert "code %d" % HEIST_EINVAL in str(ei.value)


def test_arguments(gpu_device, monkeypatch):
    R, C, N, M, E, Hh = 10, 13, 3, 2, 2, 4
    env = _make(N, _cfg(R, C, 50), gpu_device)
    env.set_layouts([([(4, 4)], [], [])] * N, budget=10)
    env.reset()
    assert env.plan_walls_supported == env.plan_masked_supported == 1
    two = _edits([[wr.add(5, 5), wr.rem(4, 4) + wr.add(0, 0)]] * N, E)
    assert env.plan_walls(two, horizon=1024).vis.shape[0] == 1024
    _einval(lambda: env.plan_walls(two, horizon=0))
    _einval(lambda: env.plan_walls(two, horizon=1025))
    for bad in (float("nan"), float("inf"), -float("inf"), -0.01, 1.01):
        _einval(lambda: env.plan_walls(two, gamma=bad))
    _einval(lambda: env.plan_walls(torch.zeros((N, 0, 1, 3), dtype=torch.int32)))
    _einval(lambda: env.plan_walls(torch.zeros((N, 1, 0, 3), dtype=torch.int32)))
    _einval(lambda: env.plan_walls(torch.zeros((N, 1, 9, 3), dtype=torch.int32)))
    assert env.plan_walls(torch.zeros((N, 1, 8, 3), dtype=torch.int32), horizon=Hh).valid.tolist() == [[True]] * N
    for wrong in (two.to(torch.int64), two[:2], two[..., :2]):
        with pytest.raises(ValueError):
            env.plan_walls(wrong)
    with pytest.raises(ValueError):
        env.plan_walls(two, masks=torch.zeros((N, M + 1), dtype=torch.int64))
    W, RC = record_words(R, C), R * C
    kw = dict(device=gpu_device)
    edits = torch.zeros(N * M * E * 3 + 1, dtype=torch.int32, **kw)
    edits[:-1] = two.reshape(-1).to(gpu_device)
    masks = torch.full((N * M + 1,), -1, dtype=torch.int64, **kw)
    valid = torch.zeros(N * M + 1, dtype=torch.uint8, **kw)
    level = torch.zeros(N * M + 1, dtype=torch.uint8, **kw)
    ticks = torch.empty(N * M + 1, dtype=torch.int16, **kw)
    value = torch.empty(N * M + 1, dtype=torch.float64, **kw)
    action = torch.empty(N * M + 1, dtype=torch.int8, **kw)
    vis = torch.empty(Hh * N * M * W + 4, dtype=torch.int32, **kw)
    tcells = torch.empty(N * M * RC + 1, dtype=torch.int16, **kw)
    vcells = torch.empty(N * M * RC + 1, dtype=torch.float64, **kw)
    lib, st = nat.lib(), env._stream()
    good = [nat.ptr(edits), nat.ptr(masks), nat.ptr(valid), nat.ptr(level), nat.ptr(ticks), nat.ptr(value),
            nat.ptr(action), nat.ptr(vis), nat.ptr(tcells), nat.ptr(vcells)]
    call = lambda *a, M_=M, E_=E: lib.heist_plan_walls(env._h, Hh, 0.99, M_, E_, *a, st)  # noqa: E731
    assert call(*good) == 0
    torch.cuda.synchronize(gpu_device)
    assert valid[:N * M].tolist() == [1, 0] * N and level[:N * M].tolist() == [1, 1] * N
    want_t, want_v = tcells[:N * M * RC].clone(), vcells[:N * M * RC].clone()
    want = (ticks[:N * M].clone(), value[:N * M].clone(), action[:N * M].clone(), vis[:Hh * N * M * W].clone())
    pf, pv = env.plan_field(horizon=Hh), env.plan_value(horizon=Hh, gamma=0.99)
    assert torch.equal(want_t.reshape(N, M, R, C)[:, 1], pf.togo) and _same(want_v.reshape(N, M, R, C)[:, 1], pv.value)
    assert torch.equal(want[3].reshape(Hh, N, M, W)[:, :, 1], pf.vis)
    # the optional arguments: a NULL mask is every slot live; the cell tables each alone and neither
    for mk, tc, vc in ((None, good[8], good[9]), (good[1], None, good[9]), (good[1], good[8], None), (None, None, None)):
        ticks.zero_(), value.zero_(), action.zero_(), tcells.zero_(), vcells.zero_()
        assert call(good[0], mk, *good[2:8], tc, vc) == 0
        torch.cuda.synchronize(gpu_device)
        assert torch.equal(ticks[:N * M], want[0]) and _same(value[:N * M], want[1]) and torch.equal(action[:N * M], want[2])
        assert torch.equal(vis[:Hh * N * M * W], want[3])
        assert tc is None or torch.equal(tcells[:N * M * RC], want_t)
        assert vc is None or _same(vcells[:N * M * RC], want_v)
        assert tc is not None or not tcells.any()
        assert vc is not None or not _bits(vcells).any()
    # 4-byte alignment is enough for the edits, 8-byte for the float64 arrays and the masks, 2-byte for the int16 ones
    edits[1:] = edits[:-1].clone()
    assert call(nat.ptr(edits[1:]), nat.ptr(masks[1:]), nat.ptr(valid[1:]), nat.ptr(level[1:]), nat.ptr(ticks[1:]),
                nat.ptr(value[1:]), nat.ptr(action[1:]), good[7], nat.ptr(tcells[1:]), nat.ptr(vcells[1:])) == 0
    torch.cuda.synchronize(gpu_device)
    assert torch.equal(ticks[1:], want[0]) and _same(value[1:], want[1]) and _same(vcells[1:], want_v)
    assert valid[1:].tolist() == [1, 0] * N and level[1:].tolist() == [1, 1] * N
    edits[:-1] = edits[1:].clone()
    for i in (0, 2, 3, 4, 5, 6, 7):  # every required pointer
        args = list(good)
        args[i] = None
        assert call(*args) == HEIST_EINVAL
    assert call(*good, M_=0) == HEIST_EINVAL and call(*good, M_=-1) == HEIST_EINVAL
    assert call(*good, E_=0) == HEIST_EINVAL and call(*good, E_=9) == HEIST_EINVAL and call(*good, E_=-1) == HEIST_EINVAL
    assert vis.data_ptr() % 16 == 0 and value.data_ptr() % 8 == 0 and masks.data_ptr() % 8 == 0
    for off in (1, 2):  # 16-byte alignment of the row array
        args = list(good)
        args[7] = nat.ptr(vis[off:])
        assert call(*args) == HEIST_EINVAL
    for i, t in ((1, masks), (5, value), (9, vcells)):
        args = list(good)
        args[i] = nat.ptr(t.view(torch.int32)[1:])  # 4 bytes past an 8-byte boundary
        assert call(*args) == HEIST_EINVAL
    args = list(good)
    args[0] = nat.ptr(edits.view(torch.int16)[1:])  # 2 bytes past a 4-byte boundary
    assert call(*args) == HEIST_EINVAL
    for i, t in ((4, ticks), (8, tcells)):
        args = list(good)
        args[i] = nat.ptr(t.view(torch.int8)[1:])   # an odd address
        assert call(*args) == HEIST_EINVAL
    assert lib.heist_plan_walls(None, Hh, 0.99, M, E, *good, st) == HEIST_EINVAL
    assert lib.heist_plan_walls_supported(None) == -1
    torch.cuda.synchronize(gpu_device)
    env.close()
    # 64 x 64: not supported, as for plan_masked
    big = _make(2, _cfg(64, 64, 50), gpu_device)
    assert big.plan_walls_supported == 0 and big.plan_masked_supported == 0
    _einval(lambda: big.plan_walls(torch.zeros((2, 1, 1, 3), dtype=torch.int32), horizon=4))
    big.close()
    monkeypatch.setenv("HEIST_PROBE_MODE", "1")
    probe = _make(3, _cfg(20, 20, 60), gpu_device)
    assert probe.kernel_config()["probe_mode"] == 1
    _einval(lambda: probe.plan_walls(torch.zeros((3, 1, 1, 3), dtype=torch.int32)))
    probe.close()


# ---- 8. other sizes: M = 1 and 5, E = 1 and 8, no guard slot

def test_other_sizes(gpu_device):
    env = _make(1, _cfg(G, G, H), gpu_device, mc=2, mg=0)
    _set(env, [wr.FIXTURES["fixed_cam"]], wr.BUDGET)
    assert env.max_guards == 0 and env.plan_walls_supported == 1
    rows = wr.rows("fixed_cam")
    one = env.plan_walls(_edits([[rows[2][0]]], 8), gamma=1.0, cells=True)          # M = 1, E = 8
    assert one.vis.shape[2] == 1 and one.edits.shape == (1, 1, 8, 3)
    _assert_ref(one, 0, 0, wr.reference("fixed_cam", rows[2][0], 1.0), "M = 1, E = 8")
    five = env.plan_walls(_edits([[r[0] for r in rows[:5]]], 1).reshape(1, 5, 3), gamma=1.0, cells=True)  # [N, M, 3]: E = 1
    assert five.edits.shape == (1, 5, 1, 3)
    for m in range(5):
        _assert_ref(five, 0, m, wr.reference("fixed_cam", rows[m][0], 1.0), "M = 5, E = 1, variant %d" % m)
    assert torch.equal(five.vis[:, :, 2], one.vis[:, :, 0])
    # three critical walls at once: still 14 ticks, the table's first action
    three = env.plan_walls(_edits([[wr.rem(4, 1) + wr.rem(4, 2) + wr.rem(4, 3)]], 8), gamma=1.0)
    assert (int(three.ticks[0, 0]), int(three.action[0, 0]), bool(three.valid[0, 0])) == (14, 2, True)
    ab = env.plan_wall_ablate(gamma=1.0)
    assert isinstance(ab, WallAblation) and ab.ticks.shape == (1, 8) and bool(ab.filled.all())
    assert ab.critical[0].tolist() == [True, True, True] + [False] * 4            # (4, 1), (4, 2), (4, 3)
    assert ab.shielding[0].tolist() == [False, False, False, True, False, False, False]   # (4, 4)
    assert ab.redundant[0].tolist() == [False] * 4 + [True] * 3                    # (4, 6), (4, 7), (4, 8)
    assert ab.ticks[0].tolist() == [r[1] for r in rows] and [float(v) for v in ab.value[0]] == [r[2] for r in rows]
    env.close()


# ---- 9. the search layer on the GPU

def _search_env(dev, n=8):
    R, budget = 12, 14
    cfg = _cfg(R, R, 40)
    env = _make(n, cfg, dev)
    lays = synthetic_layouts(n, R, R, budget, seed=11, n_cams=2, n_guards=1)
    valid = env.set_layouts(lays, budget=budget)
    env.reset()
    return env, cfg, valid


def test_wall_placement_scan_chunking(gpu_device):
    env, cfg, _ = _search_env(gpu_device)
    cd = wall_candidates(env.grid_snapshot())
    M, hz = cd.shape[1], 30
    assert M == 100
    whole = wall_placement_scan(env, cd, horizon=hz, gamma=0.99)
    per = 4 * hz * env.n_envs * record_words(12, 12)
    parts = wall_placement_scan(env, cd, horizon=hz, gamma=0.99, max_bytes=7 * per)  # chunks of 7, the last one of 2
    assert isinstance(whole, WallScan) and whole.valid.shape == (env.n_envs, M)
    for a, b in ((whole.valid, parts.valid), (whole.level, parts.level), (whole.ticks, parts.ticks),
                 (whole.action, parts.action), (whole.ticks0, parts.ticks0)):
        assert torch.equal(a, b)
    assert _same(whole.value, parts.value) and _same(whole.value0, parts.value0)
    direct = env.plan_walls(cd, horizon=hz, gamma=0.99)
    assert torch.equal(whole.ticks, direct.ticks) and _same(whole.value, direct.value)
    g = env.grid_snapshot()[:, 1:-1, 1:-1].reshape(env.n_envs, -1)
    assert torch.equal(whole.valid, (g == 0))          # every interior EMPTY tile, and only those (tick 0: the
    pf, pv = env.plan_field(horizon=hz), env.plan_value(horizon=hz, gamma=0.99)  # Solver stands on START)
    assert torch.equal(whole.ticks0, pf.togo[:, 1, 1]) and _same(whole.value0, pv.value[:, 1, 1])
    m = whole.metrics()
    assert set(m) == {"wall_headroom_mean", "wall_blocking_frac", "wall_helps_frac", "wall_invalidating_frac",
                      "wall_headroom_envs"}
    print(m)
    env.close()


def test_greedy_walls_two_rounds(gpu_device):
    """Both rounds re-derived: the round's choice from a scan of the env as a twin that holds the walls chosen so
    far, by the rule in NumPy; the round's value and ticks from that twin with the chosen wall built in."""
    env, cfg, valid = _search_env(gpu_device)
    hz, n = 30, env.n_envs
    before = env.save_state().blobs.clone()
    gw = greedy_walls(env, 2, horizon=hz, gamma=0.99, max_bytes=4 * hz * n * record_words(12, 12) * 40)
    assert torch.equal(env.save_state().blobs, before)
    assert len(gw.index) == 2 and gw.edits.shape == (n, 2, 3)
    lays, spent = env.layout_lists()
    chosen = [[] for _ in range(n)]
    value, ticks = gw.value0.cpu().numpy().copy(), gw.ticks0.cpu().numpy().copy()
    for r in range(2):
        twin = _make(n, cfg, gpu_device)
        twin.set_layouts([(list(l[0]) + chosen[e], l[1], l[2]) for e, l in enumerate(lays)],
                         budget=[int(s) + 2 for s in spent])
        twin.reset()
        sc = wall_placement_scan(twin, wall_candidates(twin.grid_snapshot()), horizon=hz, gamma=0.99)
        assert _same(sc.value0, torch.from_numpy(value).to(gpu_device)) and sc.ticks0.cpu().numpy().tolist() == ticks.tolist()
        ok = (sc.valid & sc.level & (sc.ticks >= 0)).cpu().numpy()
        v, t = sc.value.cpu().numpy(), sc.ticks.cpu().numpy()
        for e in range(n):
            gain = np.where(ok[e] & (value[e] - v[e] > 0), value[e] - v[e], -1.0)
            want = int(np.argmax(gain)) if gain.max() > 0 else -1
            assert int(gw.index[r][e]) == want, (r, e)
            if want >= 0:
                rr, cc = want // 10 + 1, want % 10 + 1
                assert gw.edits[e, r].tolist() == [rr, cc, 1]
                chosen[e].append((rr, cc))
                value[e], ticks[e] = v[e, want], t[e, want]
            else:
                assert gw.edits[e, r].tolist() == [0, 0, 0]
        assert vr.bits(gw.value[r].cpu().numpy()).tolist() == vr.bits(value).tolist()
        assert gw.ticks[r].cpu().numpy().tolist() == ticks.tolist()
        twin.close()
    assert sum(len(c) for c in chosen) >= n // 2  # the adversary finds walls to build
    # the final layouts, built: the predicted value is the rebuilt layout's
    twin = _make(n, cfg, gpu_device)
    twin.set_layouts([(list(l[0]) + chosen[e], l[1], l[2]) for e, l in enumerate(lays)], budget=[int(s) + 2 for s in spent])
    twin.reset()
    assert _same(twin.plan_value(horizon=hz, gamma=0.99).value[:, 1, 1], gw.value[1])
    twin.close()
    with pytest.raises(ValueError):
        greedy_walls(env, 9)
    env.close()


# ---- 10. trainer

def test_trainer_track_wall_credit(gpu_device, tmp_path):
    from heist_amd.training import AdversarialTrainer
    outs, seen = {}, []
    for track in (False, True):
        cfg = EnvironmentConfig(grid_rows=G, grid_cols=G, max_steps=H)
        d = tmp_path / str(track)
        tr = AdversarialTrainer(cfg, solver_episodes_per_layout=1, total_episodes=10 ** 6, save_dir=str(d / "ck"),
                                log_dir=str(d / "logs"), n_envs=32, rollout_len=16, device=gpu_device, seed=0,
                                minibatch=256, track_wall_credit=track, headroom_envs=8)
        inner = tr._wall_credit_layout_batch

        def spy(env_ids, tr=tr, inner=inner):  # the state of every ablated batch, as the trainer saw it
            seen.append(tr.env.save_state([int(i) for i in env_ids][:8]))
            inner(env_ids)
        tr._wall_credit_layout_batch = spy
        tr.global_episode = 200  # curriculum phase with cameras and guards
        tr._assign_layouts(np.arange(32))
        n_seen = len(seen)
        outs[track] = tr.train_iteration()
        if track:
            assert n_seen >= 1
            # the twin-handle scan: every interior wall of every saved env dropped from its layout in turn
            m = len(seen[-1])
            twin = HeistEnv(m, cfg, max_cams=tr.env.max_cams, max_guards=tr.env.max_guards, max_path=tr.env.max_path,
                            device=gpu_device, auto_reset=True)
            assert bool(twin.load_state(seen[-1]).all())
            grid = twin.grid_snapshot().cpu().numpy()
            pf, pv = twin.plan_field(), twin.plan_value(gamma=1.0)
            t0, v0 = pf.togo[:, 1, 1].cpu().numpy(), pv.value[:, 1, 1].cpu().numpy()
            lays, spent = twin.layout_lists()
            drops = [(e, w) for e in range(m) for w in sorted(map(tuple, np.argwhere(grid[e, 1:-1, 1:-1] == 1) + 1))]
            n_unsolv, n_crit_lay, n_red, n_shield, credit = int((t0 < 0).sum()), set(), 0, 0, []
            for j0 in range(0, len(drops), m):
                part = drops[j0:j0 + m]
                rebuilt = [(lays[e][0], lays[e][1], lays[e][2]) for e in range(m)]
                for j, (e, w) in enumerate(part):
                    walls = [tuple(x) for x in lays[e][0]]
                    assert (int(w[0]), int(w[1])) in walls
                    rebuilt[j] = ([x for x in walls if x != (int(w[0]), int(w[1]))], lays[e][1], lays[e][2])
                twin.set_layouts(rebuilt, budget=[int(spent[e]) for e, _ in part] + [int(s) for s in spent[len(part):]])
                twin.reset()
                t1, v1 = twin.plan_field().togo[:, 1, 1].cpu().numpy(), twin.plan_value(gamma=1.0).value[:, 1, 1].cpu().numpy()
                for j, (e, w) in enumerate(part):
                    c = v1[j] - v0[e]
                    credit.append(c)
                    n_shield += int(c < 0)
                    n_red += int(t1[j] == t0[e] and int(vr.bits(v1[j:j + 1])[0]) == int(vr.bits(v0[e:e + 1])[0]))
                    if t0[e] < 0 < t1[j]:
                        n_crit_lay.add(e)
            div = lambda a, b: a / b if b else 0.0  # noqa: E731
            want = {"critical_wall_layout_frac": div(len(n_crit_lay), n_unsolv), "redundant_wall_frac": div(n_red, len(drops)),
                    "shielding_wall_frac": div(n_shield, len(drops)), "wall_credit_mean": div(float(np.sum(credit)), len(drops))}
            twin.close()
            assert tr._headroom_env is not None and len(drops) >= 1
        else:
            assert not seen and tr._headroom_env is None
        tr.close()
    keys = {"critical_wall_layout_frac", "redundant_wall_frac", "shielding_wall_frac", "wall_credit_mean"}
    assert set(outs[True]) == set(outs[False]) | keys and not keys & set(outs[False])
    # the three shares are ratios of exact counts.  The mean is a float64 sum of a few dozen terms taken in another
    # order: a relative 1e-12 is a thousand times its rounding
    for k in sorted(keys):
        print(k, outs[True][k], want[k])
        if k == "wall_credit_mean":
            assert outs[True][k] == pytest.approx(want[k], rel=1e-12, abs=1e-15), k
        else:
            assert outs[True][k] == want[k], k
