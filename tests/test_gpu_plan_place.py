"""heist_plan_place (HeistEnv.plan_place) and the searches on it: every env planned with one more
camera, M candidates per env in one launch that casts the candidate alone -- validity, the fewest
ticks, the optimal return and first action from the Solver's cell, every variant's visibility planes
and the whole tick-0 tables.  Every comparison is equality, float64 through its bits (int64).

Yardsticks, none of which uses the kernel under test: place_ref (the C oracle on layouts with the
candidate appended to their camera lists, and the NumPy recurrences on its witness planes);
heist_plan_field / heist_plan_value on twin handles whose layouts hold the candidate as a camera of
their own.
"""
import numpy as np
import pytest
import torch

import masked_ref as mr
import place_ref as plr
import plan_ref as pr
import value_ref as vr
from heist_amd import (EnvironmentConfig, HeistEnv, PlacementScan, PlanPlace, RelocationScan, _native as nat,
                       ablation_masks, camera_candidates, greedy_cameras, placement_scan, relocation_scan)
from heist_amd.layouts import synthetic_layouts
from heist_amd.obs_compact import record_words

pytestmark = pytest.mark.gpu

HEIST_EINVAL = 100000
MC, MG, MP = 5, 3, 16
G, H = pr.GRID, pr.MAX_STEPS
SR, SC = pr.START
NAN_ROW = [float("nan")] * 6


def _cfg(R, C, max_steps, start=(1, 1)):
    return EnvironmentConfig(grid_rows=R, grid_cols=C, max_steps=max_steps, start_pos=start, architect_budget=C + 10)


def _make(n, cfg, dev, cones=True, mc=MC, mg=MG):
    env = HeistEnv(n, cfg, max_cams=mc, max_guards=mg, max_path=MP, device=dev, auto_reset=False)
    env.set_guard_cones(cones)
    return env


def _set(env, lays, budget):
    """Layouts set and reset, every emitter of every layout bought."""
    env.set_layouts(lays, budget=budget)
    env.reset()
    x = env.export()
    assert x["n_cams"].tolist() == [len(l[1]) for l in lays] and x["n_guards"].tolist() == [len(l[2]) for l in lays]
    return x


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _rows(cands):
    return torch.tensor([list(c) for c in cands], dtype=torch.float64)


def _planes(pp, e, m):
    """[H, R, C] bool: variant (e, m)'s visibility rows unpacked."""
    return torch.stack([pp.vis_mask(k, m)[e] for k in range(1, pp.vis.shape[0] + 1)]).cpu().numpy()


def _check_padding(pp, HK):
    """Bits past R C and words past ceil(R C / 32) are 0; rows >= HK[e] are 0."""
    RC = pp.rows * pp.cols
    words = pp.vis.cpu().numpy().view(np.uint32)  # [H, N, M, W]
    nvis = (RC + 31) // 32
    assert not words[..., nvis:].any(), "words past ceil(RC/32) must be 0"
    if RC % 32:
        assert not (words[..., nvis - 1] >> (RC % 32)).any(), "bits past RC must be 0"
    for e, hk in enumerate(HK):
        assert not words[hk:, e].any(), "env %d: vis rows >= HK must be 0" % e


def _assert_twin(pp, e, m, pf, pv, i, pos, what):
    """Variant (e, m) of pp equals plan_field / plan_value of twin env i, everywhere and at pos."""
    assert torch.equal(pp.togo_cells[e, m], pf.togo[i]), what
    assert _same(pp.value_cells[e, m], pv.value[i]), what
    assert int(pp.ticks[e, m]) == int(pf.togo[i, pos[0], pos[1]]), what
    assert _same(pp.value[e, m], pv.value[i, pos[0], pos[1]]), what
    assert int(pp.action[e, m]) == int(pv.action[i, pos[0], pos[1]]), what
    assert torch.equal(pp.vis[:, e, m], pf.vis[:, i]) and torch.equal(pf.vis, pv.vis), what


# ---- 1. the fixture table against the oracle on the layouts with the candidate appended

TABLE = plr.VALID + list(plr.INVALID.values())  # 18 candidates: 3 envs x 6


@pytest.mark.parametrize("cones", [True, False], ids=["cached_guards", "live_guards"])
@pytest.mark.parametrize("waves", [1, 2, 4])
def test_fixture_table(gpu_device, monkeypatch, waves, cones):
    monkeypatch.setenv("HEIST_MULTI_WAVES", str(waves))
    N, M, W = 3, 6, record_words(G, G)
    assert len(TABLE) == N * M
    env = _make(N, _cfg(G, G, H), gpu_device, cones)
    _set(env, [plr.BASE] * N, plr.BUDGET)
    kc = env.kernel_config()
    assert kc["multi_waves"] == waves and kc["guard_cones"] == (1 if cones else 0) and env.plan_place_supported == 1
    cands = _rows(TABLE).reshape(N, M, 6)
    for gamma in (1.0, 0.99):
        pp = env.plan_place(cands, gamma=gamma, cells=True)
        assert isinstance(pp, PlanPlace) and pp.gamma == gamma and pp.tick.tolist() == [0] * N
        assert pp.valid.shape == (N, M) and pp.valid.dtype == torch.bool
        assert pp.ticks.shape == (N, M) and pp.ticks.dtype == torch.int16
        assert pp.value.shape == (N, M) and pp.value.dtype == torch.float64
        assert pp.action.shape == (N, M) and pp.action.dtype == torch.int8
        assert pp.vis.shape == (H, N, M, W) and pp.vis.dtype == torch.int32
        assert pp.togo_cells.shape == (N, M, G, G) and pp.value_cells.shape == (N, M, G, G)
        assert pp.cands.shape == (N, M, 6) and torch.equal(_bits(pp.cands.cpu()), _bits(cands))
        pf, pv = env.plan_field(), env.plan_value(gamma=gamma)   # the baseline, on the handle itself
        base = plr.reference(None, gamma)
        np.testing.assert_array_equal(pf.togo[0].cpu().numpy(), base["togo"])
        for j, c in enumerate(TABLE):
            e, m = divmod(j, M)
            ref, what = plr.reference(c, gamma), "%r gamma %r" % (c, gamma)
            print("%s: valid %d ticks %d value %r" % (what, int(pp.valid[e, m]), int(pp.ticks[e, m]), float(pp.value[e, m])))
            assert bool(pp.valid[e, m]) == ref["valid"] == (j < len(plr.VALID)), what
            assert int(pp.ticks[e, m]) == ref["ticks"], what
            assert vr.bits(float(pp.value[e, m])) == vr.bits(ref["value"][pr.START]), what
            assert int(pp.action[e, m]) == int(ref["action"][pr.START]), what
            np.testing.assert_array_equal(pp.togo_cells[e, m].cpu().numpy(), ref["togo"], what)
            np.testing.assert_array_equal(vr.bits(pp.value_cells[e, m].cpu().numpy()), vr.bits(ref["value"]), what)
            got = _planes(pp, e, m)
            diff = [k + 1 for k in range(H) if (got[k] != ref["planes"][k]).any()]
            assert not diff, "%s: vis differs from the witnesses first at tick %d" % (what, diff[0])
            wm = torch.from_numpy(ref["walls"]).to(gpu_device)
            assert bool((pp.togo_cells[e, m][wm] == -1).all()) and not _bits(pp.value_cells[e, m][wm]).any()
            if not ref["valid"]:  # the baseline, bit for bit
                _assert_twin(pp, e, m, pf, pv, e, pr.START, what)
        _check_padding(pp, [H] * N)
    lean = env.plan_place(cands, gamma=0.99)
    assert lean.togo_cells is None and lean.value_cells is None
    assert torch.equal(lean.ticks, pp.ticks) and _same(lean.value, pp.value) and torch.equal(lean.vis, pp.vis)
    assert torch.equal(lean.valid, pp.valid) and torch.equal(lean.action, pp.action)
    env.close()


# ---- 2. twin handles: the candidate as a camera of the layout's own

# name -> (R, C, max_steps, budget)
SHAPES = {"10x10": (10, 10, 40, 15), "13x17": (13, 17, 50, 27), "20x20": (20, 20, 60, 30), "32x32": (32, 32, 80, 42)}
# (fov, heading, speed, range) of the three candidates every env gets; range 7 is cast on the exact path alone
PARAMS = [(60.0, 90.0, 15.0, 6.0), (95.5, 301.25, -10.0, 7.0), (30.0, 0.0, 0.0, 4.0)]


def _empty_cells(grid, e, rng, k):
    """k distinct EMPTY interior cells of env e's grid, drawn with rng."""
    rr, cc = np.nonzero(grid[e, 1:-1, 1:-1] == 0)
    pick = rng.permutation(len(rr))[:k]
    return [(int(rr[i]) + 1, int(cc[i]) + 1) for i in pick]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_twin_handles(gpu_device, name):
    R, C, max_steps, budget = SHAPES[name]
    N, M = 4, len(PARAMS)
    cfg = _cfg(R, C, max_steps)
    lays = synthetic_layouts(N, R, C, budget, seed=1000 * R + C, n_cams=2, n_guards=1)
    a = _make(N, cfg, gpu_device)
    _set(a, lays, budget)
    assert a.plan_place_supported == 1
    grid = a.grid_snapshot().cpu().numpy()
    rng = np.random.Generator(np.random.PCG64(7 * R + C))
    cands, twins = [], []
    for e, (walls, cams, guards) in enumerate(lays):
        cells = _empty_cells(grid, e, rng, M)
        for (r, c), (fov, hd, sp, rg) in zip(cells, PARAMS):
            cands.append((r, c, fov, hd, sp, rg))
            twins.append((walls, cams + [plr.cam_dict(cands[-1])], guards))
    b = _make(N * M, cfg, gpu_device, mc=MC + 1)
    _set(b, twins, budget + 3)
    wall, twall = grid == 1, b.grid_snapshot().cpu().numpy() == 1
    for gamma in (1.0, 0.99):
        pp = a.plan_place(_rows(cands).reshape(N, M, 6), gamma=gamma, cells=True)
        assert bool(pp.valid.all())
        pf, pv = b.plan_field(), b.plan_value(gamma=gamma)
        for e in range(N):
            for m in range(M):
                i = e * M + m
                assert (wall[e] == twall[i]).all()
                _assert_twin(pp, e, m, pf, pv, i, (SR, SC), "%s env %d candidate %d gamma %r" % (name, e, m, gamma))
        _check_padding(pp, [max_steps] * N)
    base = a.plan_field().vis
    assert sum(int(not torch.equal(pp.vis[:, e, m], base[:, e])) for e in range(N) for m in range(M)) >= N * M // 2
    a.close()
    b.close()


# ---- 3. mid-episode state, horizons, the timeout, done envs

def test_mid_episode_and_horizons(gpu_device):
    c = plr.PREMISE[1]                 # (7, 3), heading 90, speed 15: it rotates
    T, plan = plr.search(c)[:2]        # unseen under BASE plus c, hence under BASE
    assert T == 34
    seen_at_once = ([], [{"row": 1, "col": 4, "fov_angle": 60.0, "vision_range": 6, "heading": 180.0,
                          "rotation_speed": 0.0}], [])            # looks along row 1 at the start: done on tick 1
    cfg = _cfg(G, G, H)
    a, b = _make(3, cfg, gpu_device), _make(3, cfg, gpu_device, mc=MC + 1)
    _set(a, [plr.BASE, plr.BASE, seen_at_once], plr.BUDGET)
    _set(b, [plr.with_cand(l, c) for l in (plr.BASE, plr.BASE, seen_at_once)], plr.BUDGET)
    slot = [len(plr.BASE[1]), len(plr.BASE[1]), 1]  # the candidate's camera slot in b
    acts = torch.zeros((H, 3), dtype=torch.int64, device=gpu_device)
    acts[:T, :2] = torch.tensor(plan, device=gpu_device).reshape(-1, 1)
    played = 0
    for k in (3, 7):
        a.step_multi(acts[played:k], auto_reset=False)
        b.step_multi(acts[played:k], auto_reset=False)
        played = k
        xa, xb = a.export(), b.export()
        assert xa["tick"].tolist()[:2] == [k, k] and xa["done"].tolist() == [0, 0, 1] and xb["done"].tolist() == [0, 0, 1]
        pos = (int(xa["pos_r"][0]), int(xa["pos_c"][0]))
        assert pos == (int(xb["pos_r"][0]), int(xb["pos_c"][0]))
        rows = torch.tensor([list(c)] * 3, dtype=torch.float64)
        rows[:, 3] = torch.stack([xb["cam_heading"][e, slot[e]] for e in range(3)]).cpu()  # its heading now
        assert float(rows[0, 3]) == (90.0 + 15.0 * k) % 360.0
        # a horizon shorter than, equal to and longer than the H - k ticks left
        for hz in (5, H - k, H):
            pp = a.plan_place(rows.reshape(3, 1, 6), horizon=hz, gamma=0.99, cells=True)
            pf, pv = b.plan_field(horizon=hz), b.plan_value(horizon=hz, gamma=0.99)
            assert pp.tick.tolist() == [k, k, -1] and pp.vis.shape[0] == hz and bool(pp.valid[:2].all())
            for e in (0, 1):
                _assert_twin(pp, e, 0, pf, pv, e, pos, "after %d ticks, horizon %d, env %d" % (k, hz, e))
            assert int(pp.ticks[0, 0]) == (T - k if hz >= T - k else -1)
            # the env already done: no plan, nothing to collect, no visibility rows
            assert int(pp.ticks[2, 0]) == -1 and not _bits(pp.value[2]).any() and int(pp.action[2, 0]) == -1
            assert bool((pp.togo_cells[2] == -1).all()) and not _bits(pp.value_cells[2]).any()
            assert not pp.vis[:, 2].any()
            _check_padding(pp, [min(hz, H - k)] * 2 + [0])
    a.close()
    b.close()
    # one tick before the timeout: one step, the timeout's share of the reward included
    far = plr.cand(8, 6, 0, 0, rng=2)  # looks at the vault's row from (8, 6): the start is never seen
    a, b = _make(2, cfg, gpu_device), _make(2, cfg, gpu_device, mc=MC + 1)
    _set(a, [([], [], []), plr.BASE], plr.BUDGET)
    _set(b, [plr.with_cand(([], [], []), far), plr.with_cand(plr.BASE, far)], plr.BUDGET)
    waits = torch.zeros((H - 1, 2), dtype=torch.int64)
    a.step_multi(waits, auto_reset=False)
    b.step_multi(waits, auto_reset=False)
    x = b.export()
    assert int(x["tick"][0]) == H - 1 and int(x["done"][0]) == 0
    pl = a.plan_place(_rows([far]), cells=True)
    lf, lv = b.plan_field(), b.plan_value()
    for e in (0, 1):
        _assert_twin(pl, e, 0, lf, lv, e, (SR, SC), "last tick, env %d" % e)
    assert not pl.vis[1:].any() and bool(pl.vis[0].any()) and pl.ticks[:, 0].tolist() == [-1, -1]
    assert float(pl.value[0, 0]) == -0.01 + 1.0 * 0.1 + (1.0 - 13.0 / 14.0) * 2.0
    a.close()
    b.close()


# ---- 4. relocation: the rows of the layout without camera j, plus camera j elsewhere

def test_relocation(gpu_device):
    walls, cams, guards = mr.FIXTURES["two_cams_guard"]     # cameras at (6, 3) and (6, 5), heading 270, speed 30
    cfg = _cfg(G, G, H)
    a = _make(2, cfg, gpu_device)
    x = _set(a, [(walls, cams, guards)] * 2, mr.BUDGET)
    moved = [(7, 6), (2, 7)]                                # where camera 0 goes, per env
    b = _make(2, cfg, gpu_device)
    _set(b, [(walls, [dict(cams[0], row=r, col=c), cams[1]], guards) for r, c in moved], mr.BUDGET)
    masks = ablation_masks(x["n_cams"], x["n_guards"], MC, MG)[:, [1]].contiguous()   # all but camera 0
    for gamma in (1.0, 0.99):
        pm = a.plan_masked(masks, gamma=gamma)
        rows = _rows([(r, c, 60.0, 270.0, 30.0, 6.0) for r, c in moved]).reshape(2, 1, 6)
        pp = a.plan_place(rows, gamma=gamma, base=pm.vis[:, :, 0], cells=True)
        pf, pv = b.plan_field(), b.plan_value(gamma=gamma)
        assert bool(pp.valid.all())
        for e in range(2):
            _assert_twin(pp, e, 0, pf, pv, e, (SR, SC), "camera 0 moved to %r, gamma %r" % (moved[e], gamma))
    # relocation_scan: the same answers at the candidate of that tile, and the rank restated
    rs = relocation_scan(a, 0, gamma=0.99)
    assert isinstance(rs, RelocationScan) and isinstance(rs.scan, PlacementScan)
    full = a.plan_masked(torch.tensor([-1]), gamma=0.99)
    assert torch.equal(rs.ticks_built, full.ticks[:, 0]) and _same(rs.value_built, full.value[:, 0])
    assert torch.equal(rs.scan.ticks0, pm.ticks[:, 0]) and _same(rs.scan.value0, pm.value[:, 0])
    assert rs.scan.valid.shape == (2, (G - 2) * (G - 2))
    for e, (r, c) in enumerate(moved):
        j = (r - 1) * (G - 2) + (c - 1)
        assert rs.scan.cands[e, j].tolist() == [float(r), float(c), 60.0, 270.0, 30.0, 6.0]
        assert bool(rs.scan.valid[e, j]) and int(rs.scan.ticks[e, j]) == int(pp.ticks[e, 0])
        assert _same(rs.scan.value[e, j], pp.value[e, 0])
    grid = a.grid_snapshot()
    assert torch.equal(rs.scan.valid, (grid[:, 1:-1, 1:-1] == 0).reshape(2, -1))
    v, ok = rs.scan.value.cpu().numpy(), rs.scan.valid.cpu().numpy()
    want = [(ok[e] & (v[e] < float(full.value[e, 0]))).sum() for e in range(2)]
    assert rs.rank.tolist() == want
    print("relocation rank of camera 0:", rs.rank.tolist(), "of", ok.sum(1).tolist())
    two = relocation_scan(a, 1, headings=[0.0, 180.0], gamma=0.99)
    assert two.scan.valid.shape == (2, 2 * (G - 2) * (G - 2)) and two.scan.cands[0, 1].tolist() == [1.0, 1.0, 60.0, 180.0, 30.0, 6.0]
    a.close()
    b.close()


# ---- 5. M handling

def test_m_handling(gpu_device):
    env = _make(2, _cfg(G, G, H), gpu_device)
    _set(env, [plr.BASE, (pr.WALLROW, [pr.cam(90, 0)], [])], plr.BUDGET)
    nine = plr.VALID + [plr.INVALID["wall"]]
    rows = _rows(nine)
    p9 = env.plan_place(rows, gamma=0.99, cells=True)            # [M, 6]: the same candidates on every env
    assert p9.vis.shape == (H, 2, 9, record_words(G, G)) and p9.cands.shape == (2, 9, 6)
    assert p9.valid.tolist() == [[True] * 8 + [False]] * 2
    for m, c in enumerate(nine):                                 # env 0 is the fixture table's layout
        assert int(p9.ticks[0, m]) == plr.reference(c, 0.99)["ticks"]
    assert not torch.equal(p9.ticks[0], p9.ticks[1])
    for m in range(9):                                           # M = 1, one candidate at a time
        p1 = env.plan_place(rows[m:m + 1], gamma=0.99, cells=True)
        assert p1.vis.shape[2] == 1 and torch.equal(p1.vis[:, :, 0], p9.vis[:, :, m])
        assert torch.equal(p1.togo_cells[:, 0], p9.togo_cells[:, m]) and _same(p1.value_cells[:, 0], p9.value_cells[:, m])
        assert torch.equal(p1.ticks[:, 0], p9.ticks[:, m]) and _same(p1.value[:, 0], p9.value[:, m])
        assert torch.equal(p1.action[:, 0], p9.action[:, m]) and torch.equal(p1.valid[:, 0], p9.valid[:, m])
    # candidates that differ per env: env 1 gets them in reverse
    per = torch.stack([rows, rows.flip(0)])
    pd = env.plan_place(per, gamma=0.99, cells=True)
    assert torch.equal(pd.vis[:, 0], p9.vis[:, 0]) and torch.equal(pd.vis[:, 1], p9.vis[:, 1].flip(1))
    assert torch.equal(pd.ticks[1], p9.ticks[1].flip(0)) and _same(pd.value[1], p9.value[1].flip(0))
    assert torch.equal(pd.togo_cells[1], p9.togo_cells[1].flip(0)) and torch.equal(pd.valid[1], p9.valid[1].flip(0))
    # base given = the base the wrapper takes by itself
    pb = env.plan_place(rows, gamma=0.99, base=env.plan_value(gamma=0.5).vis)
    assert torch.equal(pb.vis, p9.vis) and _same(pb.value, p9.value)
    with pytest.raises(ValueError):
        env.plan_place(rows.float())
    with pytest.raises(ValueError):
        env.plan_place(torch.zeros((3, 9, 6), dtype=torch.float64))
    with pytest.raises(ValueError):
        env.plan_place(rows, base=env.plan_field(horizon=5).vis)
    env.close()


# ---- 6. the launch only reads the env

def test_plan_place_reads_only(gpu_device, monkeypatch):
    """64 lean-served 20 x 20 envs with the shared fan table in use: the saved state is byte-equal
    before and after plan_place(), and the next 20-tick heist_step_multi_records launch is
    bit-identical to a twin's that never called it."""
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
    cd = camera_candidates(a.grid_snapshot(), [0.0, 120.0], 60.0, 15.0, 6)[:, 100:108]
    pp = a.plan_place(cd, horizon=50, gamma=0.99)
    assert bool(pp.valid.any()) and bool(pp.vis.any())
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
    R, C, N, M, Hh = 13, 17, 3, 2, 4
    env = _make(N, _cfg(R, C, 50), gpu_device)
    env.set_layouts([([], [], [])] * N, budget=10)
    env.reset()
    assert env.plan_place_supported == env.plan_masked_supported == 1
    rows = _rows([(5, 5, 60, 0, 15, 6), NAN_ROW])
    assert env.plan_place(rows, horizon=1024).vis.shape[0] == 1024
    _einval(lambda: env.plan_place(rows, horizon=0))
    _einval(lambda: env.plan_place(rows, horizon=1025))
    for bad in (float("nan"), float("inf"), -float("inf"), -0.01, 1.01):
        _einval(lambda: env.plan_place(rows, gamma=bad))
    _einval(lambda: env.plan_place(torch.zeros((N, 0, 6), dtype=torch.float64)))
    W, RC = record_words(R, C), R * C
    kw = dict(device=gpu_device)
    cand = torch.zeros(N * M * 6 + 1, dtype=torch.float64, **kw)
    cand[:N * M * 6] = rows.reshape(1, -1).expand(N, -1).reshape(-1).to(gpu_device)
    base = torch.zeros(Hh * N * W + 4, dtype=torch.int32, **kw)
    base[:Hh * N * W] = env.plan_field(horizon=Hh).vis.reshape(-1)
    valid = torch.zeros(N * M + 1, dtype=torch.uint8, **kw)
    ticks = torch.empty(N * M + 1, dtype=torch.int16, **kw)
    value = torch.empty(N * M + 1, dtype=torch.float64, **kw)
    action = torch.empty(N * M + 1, dtype=torch.int8, **kw)
    vis = torch.empty(Hh * N * M * W + 4, dtype=torch.int32, **kw)
    tcells = torch.empty(N * M * RC + 1, dtype=torch.int16, **kw)
    vcells = torch.empty(N * M * RC + 1, dtype=torch.float64, **kw)
    lib, st = nat.lib(), env._stream()
    good = [nat.ptr(cand), nat.ptr(base), nat.ptr(valid), nat.ptr(ticks), nat.ptr(value), nat.ptr(action), nat.ptr(vis),
            nat.ptr(tcells), nat.ptr(vcells)]
    call = lambda *a, M_=M: lib.heist_plan_place(env._h, Hh, 0.99, M_, *a, st)  # noqa: E731
    assert call(*good) == 0
    torch.cuda.synchronize(gpu_device)
    assert valid[:N * M].tolist() == [1, 0] * N
    want_t, want_v = tcells[:N * M * RC].clone(), vcells[:N * M * RC].clone()
    want = (ticks[:N * M].clone(), value[:N * M].clone(), action[:N * M].clone(), vis[:Hh * N * M * W].clone())
    pf, pv = env.plan_field(horizon=Hh), env.plan_value(horizon=Hh, gamma=0.99)
    assert torch.equal(want_t.reshape(N, M, R, C)[:, 1], pf.togo) and _same(want_v.reshape(N, M, R, C)[:, 1], pv.value)
    assert torch.equal(want[3].reshape(Hh, N, M, W)[:, :, 1], pf.vis)
    # the optional outputs, each alone and neither
    for tc, vc in ((None, good[8]), (good[7], None), (None, None)):
        ticks.zero_(), value.zero_(), action.zero_(), tcells.zero_(), vcells.zero_()
        assert call(*good[:7], tc, vc) == 0
        torch.cuda.synchronize(gpu_device)
        assert torch.equal(ticks[:N * M], want[0]) and _same(value[:N * M], want[1]) and torch.equal(action[:N * M], want[2])
        assert tc is None or torch.equal(tcells[:N * M * RC], want_t)
        assert vc is None or _same(vcells[:N * M * RC], want_v)
        assert tc is not None or not tcells.any()
        assert vc is not None or not _bits(vcells).any()
    # 8-byte alignment is enough for the float64 arrays, 2-byte for the int16 ones, any for the int8 / uint8 ones
    cand[1:] = cand[:N * M * 6].clone()
    assert call(nat.ptr(cand[1:]), good[1], nat.ptr(valid[1:]), nat.ptr(ticks[1:]), nat.ptr(value[1:]), nat.ptr(action[1:]),
                good[6], nat.ptr(tcells[1:]), nat.ptr(vcells[1:])) == 0
    torch.cuda.synchronize(gpu_device)
    assert torch.equal(ticks[1:], want[0]) and _same(value[1:], want[1]) and _same(vcells[1:], want_v)
    assert valid[1:].tolist() == [1, 0] * N
    cand[:N * M * 6] = cand[1:].clone()
    for i in range(7):  # every required pointer
        args = list(good)
        args[i] = None
        assert call(*args) == HEIST_EINVAL
    assert call(*good, M_=0) == HEIST_EINVAL and call(*good, M_=-1) == HEIST_EINVAL
    assert vis.data_ptr() % 16 == 0 and base.data_ptr() % 16 == 0 and value.data_ptr() % 8 == 0
    for i, t in ((1, base), (6, vis)):  # 16-byte alignment of the two row arrays
        for off in (1, 2):
            args = list(good)
            args[i] = nat.ptr(t[off:])
            assert call(*args) == HEIST_EINVAL
    for i, t in ((0, cand), (4, value), (8, vcells)):
        args = list(good)
        args[i] = nat.ptr(t.view(torch.int32)[1:])  # 4 bytes past an 8-byte boundary
        assert call(*args) == HEIST_EINVAL
    assert lib.heist_plan_place(None, Hh, 0.99, M, *good, st) == HEIST_EINVAL
    assert lib.heist_plan_place_supported(None) == -1
    torch.cuda.synchronize(gpu_device)
    env.close()
    # 64 x 64: not supported, as for plan_masked
    big = _make(2, _cfg(64, 64, 50), gpu_device)
    assert big.plan_place_supported == 0 and big.plan_masked_supported == 0
    _einval(lambda: big.plan_place(rows, horizon=4, base=torch.zeros((4, 2, record_words(64, 64)), dtype=torch.int32,
                                                                       device=gpu_device)))
    big.close()
    monkeypatch.setenv("HEIST_PROBE_MODE", "1")
    probe = _make(3, _cfg(20, 20, 60), gpu_device)
    assert probe.kernel_config()["probe_mode"] == 1
    _einval(lambda: probe.plan_place(rows, base=torch.zeros((60, 3, record_words(20, 20)), dtype=torch.int32,
                                                            device=gpu_device)))
    probe.close()


def test_any_bit_pattern_is_safe(gpu_device):
    """Rows of extreme and non-finite doubles: every one is invalid and leaves the baseline; rows at
    the contract's bounds are valid.  (What the launch must never do with them is touch memory it does
    not own; here it is seen to finish and to answer as the contract says.)"""
    env = _make(1, _cfg(G, G, H), gpu_device)
    _set(env, [plr.BASE], plr.BUDGET)
    inf, big = float("inf"), 1.7e308
    ok = [2.0, 2.0, 60.0, 0.0, 0.0, 6.0]
    bad = []
    for f, vals in ((0, (inf, -inf, big, -big, 2.0 ** 31, float("nan"))), (1, (inf, -big, 2.0 ** 40, float("nan"))),
                    (2, (0.0, -60.0, inf, big, 16000.5, float("nan"))), (3, (inf, -inf, big, -big, float("nan"))),
                    (4, (inf, -inf, big, -big, float("nan"))), (5, (-1.0, inf, 32768.0, big, float("nan")))):
        for v in vals:
            row = list(ok)
            row[f] = v
            bad.append(row)
    edge = [[2.9, 2.9, 16000.0, -1e300, 1e300, 1.0], [2.0, 2.0, 1e-300, 1e300, -1e300, 3.0], [2.0, 2.0, 60.0, 0.0, 0.0, 32767.0]]
    pp = env.plan_place(_rows(bad + edge), gamma=0.99, horizon=8, cells=True)
    nb = len(bad)
    assert pp.valid[0].tolist() == [False] * nb + [True] * len(edge)
    pf, pv = env.plan_field(horizon=8), env.plan_value(horizon=8, gamma=0.99)
    for m in range(nb):
        _assert_twin(pp, 0, m, pf, pv, 0, pr.START, "row %r" % (bad[m],))
    base = pf.vis[:, 0]
    for m in range(nb, nb + len(edge)):
        assert torch.equal(pp.vis[:, 0, m] & base, base)
    # range 32767 from (2, 2), heading 0: the exact path runs east along row 2 up to the border wall
    assert bool(pp.vis_mask(1, nb + 2)[0, 2, 3:9].all()) and not bool(pp.vis_mask(1, nb + 2)[0, 2, 2])
    _check_padding(pp, [8])
    env.close()


# ---- 8. monotone where it must be

def test_monotone_ticks_and_rows(gpu_device):
    n, R, budget, max_steps = 32, 20, 15, 60
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=R, max_steps=max_steps)
    env = HeistEnv(n, cfg, max_cams=MC, max_guards=MG, max_path=MP, device=gpu_device, auto_reset=False)
    env.set_layouts(synthetic_layouts(n, R, R, budget, seed=77), budget=budget)
    env.reset()
    cd = camera_candidates(env.grid_snapshot(), [45.0], 60.0, 15.0, 6)
    pf = env.plan_field()
    pp = env.plan_place(cd, base=pf.vis)
    t0 = pf.togo[:, 1, 1].reshape(-1, 1)
    big = lambda t: torch.where(t < 0, torch.full_like(t, 30000), t)  # noqa: E731  -1 counts as largest
    assert bool((big(pp.ticks) >= big(t0)).all()), "one more camera never shortens the way"
    assert bool((big(pp.ticks) > big(t0)).any()), "some camera costs the Solver ticks"
    assert torch.equal(pp.ticks[~pp.valid], t0.expand_as(pp.ticks)[~pp.valid])
    base = pf.vis.unsqueeze(2)
    assert torch.equal(pp.vis & base, base.expand_as(pp.vis)), "every row holds its base row"
    grid = env.grid_snapshot()
    assert torch.equal(pp.valid, (grid[:, 1:-1, 1:-1] == 0).reshape(n, -1))
    print("valid %d of %d, blocking %d, slower %d" % (int(pp.valid.sum()), pp.valid.numel(),
                                                      int(((pp.ticks < 0) & (t0 > 0)).sum()), int((pp.ticks > t0).sum())))
    env.close()


# ---- 9. greedy_cameras: the scan's prediction is the rebuilt layout's value

def test_greedy_cameras(gpu_device):
    N, budget = 4, 15
    cfg = _cfg(G, G, H)
    env = _make(N, cfg, gpu_device, mc=3)
    # baselines 18, 14, -1 and 22 ticks (field_ref's witnesses): three envs have cameras to gain, one has none
    lays = synthetic_layouts(N, G, G, budget, seed=14, n_cams=1, n_guards=1)
    x = _set(env, lays, budget)
    got, spent = env.layout_lists()
    assert spent == x["spent"].tolist() and [len(l[1]) for l in got] == [1] * N and [len(l[2]) for l in got] == [1] * N
    for (w0, c0, g0), (w1, c1, g1) in zip(lays, got):
        assert sorted(w0) == sorted(w1) and [g["patrol_path"] for g in g0] == [g["patrol_path"] for g in g1]
        assert [(c["row"], c["col"], c["heading"]) for c in c0] == [(c["row"], c["col"], c["heading"]) for c in c1]
    assert env.plan_field().togo[:, SR, SC].tolist() == [18, 14, -1, 22]
    v0 = env.plan_value(gamma=0.99).value[:, SR, SC].clone()
    n_cams = x["n_cams"].clone()
    added = 0
    for rnd in range(3):  # the third round finds every env's camera slots full
        cams, pred = greedy_cameras(env, 1, [0.0, 90.0, 180.0, 270.0], 60.0, 15.0, 6, gamma=0.99)
        assert len(cams) == len(pred) == 1 and cams[0].shape == (N, 6) and pred[0].shape == (N,)
        chose = ~torch.isnan(cams[0][:, 0])
        xe = env.export()
        assert xe["tick"].tolist() == [0] * N and torch.equal(xe["n_cams"], n_cams + chose.int())
        n_cams = xe["n_cams"].clone()
        v = env.plan_value(gamma=0.99).value[:, SR, SC]
        print("round %d: chose %s, value %s -> %s" % (rnd, chose.tolist(), v0.tolist(), v.tolist()))
        assert _same(v, pred[0]), "round %d: the rebuilt layout's value is the scan's prediction" % rnd
        assert _same(v[~chose], v0[~chose])
        added += int(chose.sum())
        v0 = v.clone()
        if rnd == 2:
            assert not bool(chose.any())
        assert not bool(chose[2])  # the unsolvable layout: no candidate is eligible
    assert added >= 3
    env.close()


# ---- 10. placement_scan: chunks of M give one call's tables

def test_placement_scan_chunking(gpu_device):
    env = _make(2, _cfg(G, G, H), gpu_device)
    _set(env, [plr.BASE, (pr.WALLROW, [pr.cam(90, 0)], [])], plr.BUDGET)
    cd = camera_candidates(env.grid_snapshot(), [0.0, 200.0], 60.0, 0.0, 6)   # cameras that never turn: some block
    M = cd.shape[1]
    assert M == 2 * (G - 2) * (G - 2)
    one = env.plan_place(cd, gamma=0.99)
    per = 4 * H * 2 * record_words(G, G)
    calls = []
    inner = env.plan_place

    def spy(c, **kw):
        calls.append(int(torch.as_tensor(c).shape[-2]))
        return inner(c, **kw)
    env.plan_place = spy
    whole = placement_scan(env, cd, gamma=0.99)
    assert calls == [1, M]
    del calls[:]
    parts = placement_scan(env, cd, gamma=0.99, max_bytes=7 * per + 5)
    assert calls == [1] + [7] * (M // 7) + [M % 7]
    env.plan_place = inner
    pf, pv = env.plan_field(), env.plan_value(gamma=0.99)
    for sc in (whole, parts):
        assert isinstance(sc, PlacementScan)
        assert torch.equal(sc.valid, one.valid) and torch.equal(sc.ticks, one.ticks) and _same(sc.value, one.value)
        assert torch.equal(sc.action, one.action) and torch.equal(_bits(sc.cands), _bits(cd))
        assert torch.equal(sc.ticks0, pf.togo[:, SR, SC]) and _same(sc.value0, pv.value[:, SR, SC])
    assert whole.ticks0.tolist() == [22, -1]
    b = whole.best()
    assert int(b[1]) == -1 and int(b[0]) >= 0 and float(whole.headroom()[1]) == 0.0
    assert float(whole.headroom()[0]) == float(whole.value0[0]) - float(whole.value[0, int(b[0])])
    elig = (whole.valid[0] & (whole.ticks[0] >= 0)).cpu().numpy()
    v = whole.value[0].cpu().numpy()
    assert elig[int(b[0])] and int(b[0]) == int(np.nonzero(elig & (v == v[elig].min()))[0][0])
    assert 0.0 < float(whole.blocking()[0]) < 1.0 and float(whole.blocking()[1]) == 0.0
    env.close()


# ---- 11. trainer

def _metrics_restated(valid, ticks, value, ticks0, value0):
    """The trainer's three figures from a scan's tables, in NumPy, env by env."""
    va, t, v = valid.cpu().numpy().astype(bool), ticks.cpu().numpy().astype(np.int64), value.cpu().numpy()
    t0, v0 = ticks0.cpu().numpy().astype(np.int64), value0.cpu().numpy()
    head, block = [], []
    for e in range(len(t0)):
        ok = va[e] & (t[e] >= 0)
        if ok.any():
            head.append(v0[e] - v[e][ok].min())
        if t0[e] >= 0:
            block.append((va[e] & (t[e] < 0)).sum() / va[e].sum() if va[e].any() else 0.0)
    return {"camera_headroom_mean": float(np.sum(head) / len(head)) if head else 0.0,
            "camera_blocking_frac": float(np.sum(block) / len(block)) if block else 0.0,
            "camera_headroom_envs": len(head)}


def test_trainer_track_camera_headroom(gpu_device, tmp_path):
    from heist_amd.components.security import Camera
    from heist_amd.training import AdversarialTrainer
    outs, seen = {}, []
    for track in (False, True):
        cfg = EnvironmentConfig(grid_rows=G, grid_cols=G, max_steps=H)
        d = tmp_path / str(track)
        tr = AdversarialTrainer(cfg, solver_episodes_per_layout=1, total_episodes=10 ** 6, save_dir=str(d / "ck"),
                                log_dir=str(d / "logs"), n_envs=32, rollout_len=16, device=gpu_device, seed=0,
                                minibatch=256, track_camera_headroom=track, headroom_envs=8, headroom_headings=4)
        inner = tr._headroom_layout_batch

        def spy(env_ids, tr=tr, inner=inner):  # the state of every scanned batch, as the trainer saw it
            seen.append(tr.env.save_state([int(i) for i in env_ids][:8]))
            inner(env_ids)
        tr._headroom_layout_batch = spy
        tr.global_episode = 200  # curriculum phase with cameras and guards
        tr._assign_layouts(np.arange(32))
        n_seen = len(seen)
        outs[track] = tr.train_iteration()
        if track:
            assert n_seen >= 1
            twin = HeistEnv(len(seen[-1]), cfg, max_cams=tr.env.max_cams, max_guards=tr.env.max_guards,
                            max_path=tr.env.max_path, device=gpu_device, auto_reset=True)
            assert bool(twin.load_state(seen[-1]).all())
            ref = Camera(0, 0)
            assert (ref.fov_angle, ref.rotation_speed, ref.vision_range) == (60.0, 15.0, 6)
            cd = camera_candidates(twin.grid_snapshot(), [0.0, 90.0, 180.0, 270.0], 60.0, 15.0, 6)
            sc = placement_scan(twin, cd, gamma=1.0)
            want = _metrics_restated(sc.valid, sc.ticks, sc.value, sc.ticks0, sc.value0)
            assert sc.metrics() == pytest.approx(want, rel=1e-12, abs=0.0)
            twin.close()
            assert tr._headroom_env is not None and tr._headroom_env.kernel_config()["guard_cones"] == 1
        else:
            assert not seen and tr._headroom_env is None
        tr.close()
        assert tr._headroom_env is None
    keys = {"camera_headroom_mean", "camera_blocking_frac", "camera_headroom_envs"}
    assert set(outs[True]) == set(outs[False]) | keys and not keys & set(outs[False])
    # the count is exact.  The two means are float64 sums of at most 8 terms taken in another order:
    # a relative 1e-12 is a thousand times their rounding
    for k in sorted(keys):
        print(k, outs[True][k], want[k])
        if k.endswith("_envs"):
            assert outs[True][k] == want[k], k
        else:
            assert outs[True][k] == pytest.approx(want[k], rel=1e-12, abs=0.0), k
    assert outs[True]["camera_headroom_envs"] >= 1
