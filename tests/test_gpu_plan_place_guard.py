"""heist_plan_place_guard (HeistEnv.plan_place_guard) and the searches on it: every env planned with
one more guard, M candidates per env in one launch that casts the candidate alone -- validity, the
fewest ticks, the optimal return and first action from the Solver's cell, every variant's visibility
planes and the whole tick-0 tables.  Every comparison is equality, float64 through its bits (int64).

Yardsticks, none of which uses the kernel under test: guard_place_ref (the C oracle's witness planes
of the base layout ORed with the candidate's alone, and the NumPy recurrences on them);
heist_plan_field / heist_plan_value on twin handles whose layouts hold the candidate as a guard of
their own, served from the cone cache or cast live.
"""
import numpy as np
import pytest
import torch

import guard_place_ref as gr
import plan_ref as pr
import value_ref as vr
from heist_amd import (EnvironmentConfig, GreedyAdversary, HeistEnv, PlacementScan, PlanPlace, _native as nat,
                       architect_patrol, camera_candidates, greedy_adversary, greedy_pick, guard_candidates,
                       guard_placement_scan, placement_scan)
from heist_amd.layouts import synthetic_layouts
from heist_amd.obs_compact import record_words

pytestmark = pytest.mark.gpu

HEIST_EINVAL = 100000
MC, MG, MP = 5, 3, 16
G, H = pr.GRID, pr.MAX_STEPS
SR, SC = pr.START
I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1


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


def _arr(cands, p=gr.P, garbage=True):
    return tuple(torch.from_numpy(x) for x in gr.arrays(cands, p, garbage))


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
    assert torch.equal(pp.vis[:, e, m], pf.vis[:, i]) and torch.equal(pf.vis, pv.vis), what
    assert torch.equal(pp.togo_cells[e, m], pf.togo[i]), what
    assert _same(pp.value_cells[e, m], pv.value[i]), what
    assert int(pp.ticks[e, m]) == int(pf.togo[i, pos[0], pos[1]]), what
    assert _same(pp.value[e, m], pv.value[i, pos[0], pos[1]]), what
    assert int(pp.action[e, m]) == int(pv.action[i, pos[0], pos[1]]), what


# ---- 1. the fixture table against the oracle's planes, base | alone

TABLE = [(n, c) for n, c in sorted(gr.PREMISE.items())] + [(n, c) for n, c in sorted(gr.INVALID.items())]  # 9 + 13


@pytest.mark.parametrize("cones", [True, False], ids=["cached_guards", "live_guards"])
@pytest.mark.parametrize("waves", [1, 2, 4])
def test_fixture_table(gpu_device, monkeypatch, waves, cones):
    monkeypatch.setenv("HEIST_MULTI_WAVES", str(waves))
    N, M, W = 2, 11, record_words(G, G)
    assert len(TABLE) == N * M
    env = _make(N, _cfg(G, G, H), gpu_device, cones)
    _set(env, [gr.BASE] * N, gr.BUDGET)
    kc = env.kernel_config()
    assert kc["multi_waves"] == waves and kc["guard_cones"] == (1 if cones else 0) and env.plan_place_guard_supported == 1
    pa, me, fv = (x.reshape((N, M) + x.shape[1:]) for x in _arr([c for _, c in TABLE]))
    for gamma in (1.0, 0.99):
        pp = env.plan_place_guard(pa, me, fv, gamma=gamma, cells=True)
        assert isinstance(pp, PlanPlace) and pp.gamma == gamma and pp.tick.tolist() == [0] * N
        assert pp.valid.shape == (N, M) and pp.valid.dtype == torch.bool
        assert pp.ticks.shape == (N, M) and pp.ticks.dtype == torch.int16
        assert pp.value.shape == (N, M) and pp.value.dtype == torch.float64
        assert pp.action.shape == (N, M) and pp.action.dtype == torch.int8
        assert pp.vis.shape == (H, N, M, W) and pp.vis.dtype == torch.int32
        assert pp.togo_cells.shape == (N, M, G, G) and pp.value_cells.shape == (N, M, G, G)
        assert isinstance(pp.cands, tuple) and len(pp.cands) == 3
        assert all(torch.equal(a.cpu(), b) for a, b in zip(pp.cands, (pa, me, fv)) if a.dtype != torch.float64)
        pf, pv = env.plan_field(), env.plan_value(gamma=gamma)   # the baseline, on the handle itself
        base = gr.reference(None, gamma)
        np.testing.assert_array_equal(pf.togo[0].cpu().numpy(), base["togo"])
        for j, (name, c) in enumerate(TABLE):
            e, m = divmod(j, M)
            ref, what = gr.reference(c, gamma), "%s gamma %r" % (name, gamma)
            print("%s: valid %d ticks %d value %r" % (what, int(pp.valid[e, m]), int(pp.ticks[e, m]), float(pp.value[e, m])))
            assert bool(pp.valid[e, m]) == ref["valid"] == (name in gr.PREMISE), what
            got = _planes(pp, e, m)
            diff = [k + 1 for k in range(H) if (got[k] != ref["planes"][k]).any()]
            assert not diff, "%s: vis differs from the witnesses first at tick %d" % (what, diff[0])
            assert int(pp.ticks[e, m]) == ref["ticks"], what
            assert vr.bits(float(pp.value[e, m])) == vr.bits(ref["value"][pr.START]), what
            assert int(pp.action[e, m]) == int(ref["action"][pr.START]), what
            np.testing.assert_array_equal(pp.togo_cells[e, m].cpu().numpy(), ref["togo"], what)
            np.testing.assert_array_equal(vr.bits(pp.value_cells[e, m].cpu().numpy()), vr.bits(ref["value"]), what)
            wm = torch.from_numpy(ref["walls"]).to(gpu_device)
            assert bool((pp.togo_cells[e, m][wm] == -1).all()) and not _bits(pp.value_cells[e, m][wm]).any()
            if not ref["valid"]:  # the baseline, bit for bit
                _assert_twin(pp, e, m, pf, pv, e, pr.START, what)
        _check_padding(pp, [H] * N)
    lean = env.plan_place_guard(pa, me, fv, gamma=0.99)
    assert lean.togo_cells is None and lean.value_cells is None
    assert torch.equal(lean.ticks, pp.ticks) and _same(lean.value, pp.value) and torch.equal(lean.vis, pp.vis)
    assert torch.equal(lean.valid, pp.valid) and torch.equal(lean.action, pp.action)
    env.close()


# ---- 2. twin handles: the candidate as a guard of the layout's own

# name -> (R, C, max_steps, budget, envs)
SHAPES = {"10x13": (10, 13, 40, 20, 8), "20x20": (20, 20, 60, 30, 8), "32x32": (32, 32, 80, 42, 8)}


def _empty_cells(grid, e, rng, k):
    """k distinct EMPTY interior cells of env e's grid away from the last interior row and column, drawn with rng."""
    rr, cc = np.nonzero(grid[e, 1:-2, 1:-2] == 0)
    pick = rng.permutation(len(rr))[:k]
    assert len(pick) == k
    return [(int(rr[i]) + 1, int(cc[i]) + 1) for i in pick]


def _twin_candidates(R, C, cell, other, rng):
    """Three guards that start on the EMPTY tile `cell`: the Architect's 8-point patrol at range 4 (a twin can
    serve it from its cone cache), the same patrol at range 8 (past the cache's range: cast live), and a
    5-point jump patrol through `other` and random tiles, walls and border included, speed 2, fov 120.5, range 6."""
    ring = architect_patrol(cell[0] + 1, cell[1] + 1, R, C)
    assert ring[0] == cell
    jump = [cell, other] + [(int(rng.integers(0, R)), int(rng.integers(0, C))) for _ in range(3)]
    return [gr.cand(ring), gr.cand(ring, rng=8), gr.cand(jump, speed=2, rng=6, fov=120.5)]


@pytest.mark.parametrize("cones", [True, False], ids=["twin_cached", "twin_live"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_twin_handles(gpu_device, name, cones):
    R, C, max_steps, budget, N = SHAPES[name]
    M = 3
    cfg = _cfg(R, C, max_steps)
    lays = synthetic_layouts(N, R, C, budget, seed=1000 * R + C, n_cams=2, n_guards=1)
    a = _make(N, cfg, gpu_device)
    _set(a, lays, budget)
    assert a.plan_place_guard_supported == 1
    grid = a.grid_snapshot().cpu().numpy()
    rng = np.random.Generator(np.random.PCG64(7 * R + C))
    cands, twins = [], []
    for e, (walls, cams, guards) in enumerate(lays):
        cell, other = _empty_cells(grid, e, rng, 2)
        for c in _twin_candidates(R, C, cell, other, rng):
            cands.append(c)
            twins.append((walls, cams, guards + [gr.guard_dict(c)]))
    b = _make(N * M, cfg, gpu_device, cones=cones, mg=MG + 1)
    _set(b, twins, budget + 5)
    wall, twall = grid == 1, b.grid_snapshot().cpu().numpy() == 1
    pa, me, fv = (x.reshape((N, M) + x.shape[1:]) for x in _arr(cands))
    for gamma in (1.0, 0.99):
        pp = a.plan_place_guard(pa, me, fv, gamma=gamma, cells=True)
        assert int(pp.valid.sum()) == N * M, "every start tile was drawn from the EMPTY cells"
        pf, pv = b.plan_field(), b.plan_value(gamma=gamma)
        for e in range(N):
            for m in range(M):
                i = e * M + m
                assert (wall[e] == twall[i]).all()
                _assert_twin(pp, e, m, pf, pv, i, (SR, SC), "%s env %d candidate %d gamma %r" % (name, e, m, gamma))
        _check_padding(pp, [max_steps] * N)
    base = a.plan_field().vis
    assert all(not torch.equal(pp.vis[:, e, m], base[:, e]) for e in range(N) for m in range(M)), "a guard marks its cell"
    a.close()
    b.close()


# ---- 3. mid-episode state, horizons, done envs

@pytest.mark.parametrize("cones", [True, False], ids=["twin_cached", "twin_live"])
def test_mid_episode_and_horizons(gpu_device, cones):
    c = gr.CORNER
    T, plan = gr.search(c)[:2]         # unseen under BASE plus c, hence under BASE
    assert T == 22
    seen_at_once = ([], [{"row": 1, "col": 4, "fov_angle": 60.0, "vision_range": 6, "heading": 180.0,
                          "rotation_speed": 0.0}], [])            # looks along row 1 at the start: done on tick 1
    cfg = _cfg(G, G, H)
    a, b = _make(3, cfg, gpu_device), _make(3, cfg, gpu_device, cones=cones, mg=MG + 1)
    _set(a, [gr.BASE, gr.BASE, seen_at_once], gr.BUDGET)
    _set(b, [gr.with_cand(l, c) for l in (gr.BASE, gr.BASE, seen_at_once)], gr.BUDGET)
    slot = [1, 1, 0]  # the candidate's guard slot in b
    acts = torch.zeros((H, 3), dtype=torch.int64, device=gpu_device)
    acts[:T, :2] = torch.tensor(plan, device=gpu_device).reshape(-1, 1)
    k = 7
    a.step_multi(acts[:k], auto_reset=False)
    b.step_multi(acts[:k], auto_reset=False)
    xa, xb = a.export(), b.export()
    assert xa["tick"].tolist()[:2] == [k, k] and xa["done"].tolist() == [0, 0, 1] and xb["done"].tolist() == [0, 0, 1]
    pos = (int(xa["pos_r"][0]), int(xa["pos_c"][0]))
    assert pos == (int(xb["pos_r"][0]), int(xb["pos_c"][0]))
    pa, me, fv = (x.unsqueeze(0).expand((3,) + x.shape).clone() for x in _arr([c]))
    for e in range(3):  # its patrol index and heading now
        me[e, 0, 3] = int(xb["guard_idx"][e, slot[e]])
        fv[e, 0, 1] = float(xb["guard_heading"][e, slot[e]])
    assert me[0, 0].tolist() == [4, 1, 2, k % 4] and float(fv[0, 0, 1]) == 180.0   # on (2, 7), come from (2, 8)
    # a horizon shorter than and a horizon longer than the H - k ticks left
    for hz in (5, H):
        pp = a.plan_place_guard(pa, me, fv, horizon=hz, gamma=0.99, cells=True)
        pf, pv = b.plan_field(horizon=hz), b.plan_value(horizon=hz, gamma=0.99)
        assert pp.tick.tolist() == [k, k, -1] and pp.vis.shape[0] == hz and pp.valid[:, 0].tolist() == [True, True, True]
        for e in (0, 1):
            _assert_twin(pp, e, 0, pf, pv, e, pos, "after %d ticks, horizon %d, env %d" % (k, hz, e))
        assert int(pp.ticks[0, 0]) == (T - k if hz >= T - k else -1)
        # the env already done: HK = 0 and the fill
        assert int(pp.ticks[2, 0]) == -1 and not _bits(pp.value[2]).any() and int(pp.action[2, 0]) == -1
        assert bool((pp.togo_cells[2] == -1).all()) and not _bits(pp.value_cells[2]).any()
        assert not pp.vis[:, 2].any()
        _check_padding(pp, [min(hz, H - k)] * 2 + [0])
    a.close()
    b.close()


# ---- 4. relocation: the rows of the layout without its guard, plus that guard's own patrol

def test_relocation(gpu_device):
    """The env guard switched off with plan_masked, and put back as the candidate: plan_field / plan_value of
    the handle itself.  The guard's own start tile holds the guard in the grid and is not EMPTY, so the
    candidate carries the guard's patrol rotated by one point -- it starts on patrol point 1, an EMPTY tile,
    and stands on its last point, the guard's point 0, with the guard's heading: the same guard on every tick."""
    cfg = _cfg(G, G, H)
    a = _make(2, cfg, gpu_device)
    _set(a, [gr.BASE, (pr.WALLROW, [], [pr.GUARD])], gr.BUDGET)
    path = pr.GUARD["patrol_path"]
    own = gr.cand(path[1:] + path[:1], pr.GUARD["speed"], pr.GUARD["vision_range"], pr.GUARD["fov_angle"])
    pa, me, fv = _arr([own])
    me[0, 3] = len(path) - 1
    mask = torch.full((2, 1), ~(1 << MC), dtype=torch.int64)   # every slot but guard 0
    for gamma in (1.0, 0.99):
        pm = a.plan_masked(mask, gamma=gamma)
        pf, pv = a.plan_field(), a.plan_value(gamma=gamma)
        assert not torch.equal(pm.vis[:, :, 0], pf.vis)
        pp = a.plan_place_guard(pa, me, fv, gamma=gamma, base=pm.vis[:, :, 0], cells=True)
        assert pp.valid.tolist() == [[True], [True]]
        for e in range(2):
            _assert_twin(pp, e, 0, pf, pv, e, (SR, SC), "guard 0 put back, env %d gamma %r" % (e, gamma))
    # the guard's record as it stands is not a valid candidate: its start tile is its own
    pa, me, fv = _arr([gr.cand(path)])
    assert a.plan_place_guard(pa, me, fv, horizon=4).valid.tolist() == [[False], [False]]
    a.close()


# ---- 5. M, P and handles without emitter slots

def test_m_and_p_handling(gpu_device):
    env = _make(2, _cfg(G, G, H), gpu_device)
    _set(env, [gr.BASE, (pr.WALLROW, [pr.cam(90, 0)], [])], gr.BUDGET)
    names = ["through_wall", "jump", "range0", "still"]
    five = [gr.PREMISE[n] for n in names] + [gr.INVALID["start_on_wall"]]
    pa, me, fv = _arr(five)
    p5 = env.plan_place_guard(pa, me, fv, gamma=0.99, cells=True)       # [M, ...]: the same candidates on every env
    assert p5.vis.shape == (H, 2, 5, record_words(G, G)) and p5.cands[0].shape == (2, 5, gr.P, 2)
    assert p5.valid.tolist() == [[True] * 4 + [False]] * 2
    for m, c in enumerate(five):                                        # env 0 is the fixture table's layout
        assert int(p5.ticks[0, m]) == gr.reference(c, 0.99)["ticks"]
    for m in range(5):                                                  # M = 1, one candidate at a time
        p1 = env.plan_place_guard(pa[m:m + 1], me[m:m + 1], fv[m:m + 1], gamma=0.99, cells=True)
        assert p1.vis.shape[2] == 1 and torch.equal(p1.vis[:, :, 0], p5.vis[:, :, m])
        assert torch.equal(p1.togo_cells[:, 0], p5.togo_cells[:, m]) and _same(p1.value_cells[:, 0], p5.value_cells[:, m])
        assert torch.equal(p1.ticks[:, 0], p5.ticks[:, m]) and _same(p1.value[:, 0], p5.value[:, m])
        assert torch.equal(p1.action[:, 0], p5.action[:, m]) and torch.equal(p1.valid[:, 0], p5.valid[:, m])
    # P = 64: the same candidates in a wider array, garbage behind; a 64-point patrol that walks the still guard's tile
    q = _arr(five, p=64)
    p64 = env.plan_place_guard(*q, gamma=0.99)
    assert torch.equal(p64.vis, p5.vis) and _same(p64.value, p5.value) and torch.equal(p64.valid, p5.valid)
    long = gr.cand([(7, 2)] * 64)
    pl = env.plan_place_guard(*_arr([long], p=64), gamma=0.99)
    assert bool(pl.valid.all()) and torch.equal(pl.vis[:, :, 0], p5.vis[:, :, 3]), "64 equal points: the still guard"
    # P = 1
    p1 = env.plan_place_guard(*_arr([gr.PREMISE["still"], gr.INVALID["zero_fov"]], p=1), gamma=0.99)
    assert p1.valid.tolist() == [[True, False]] * 2 and torch.equal(p1.vis[:, :, 0], p5.vis[:, :, 3])
    # candidates that differ per env: env 1 gets them in reverse
    per = tuple(torch.stack([x, x.flip(0)]) for x in (pa, me, fv))
    pd = env.plan_place_guard(*per, gamma=0.99, cells=True)
    assert torch.equal(pd.vis[:, 0], p5.vis[:, 0]) and torch.equal(pd.vis[:, 1], p5.vis[:, 1].flip(1))
    assert torch.equal(pd.ticks[1], p5.ticks[1].flip(0)) and _same(pd.value[1], p5.value[1].flip(0))
    # base given = the base the wrapper takes by itself
    pb = env.plan_place_guard(pa, me, fv, gamma=0.99, base=env.plan_value(gamma=0.5).vis)
    assert torch.equal(pb.vis, p5.vis) and _same(pb.value, p5.value)
    with pytest.raises(ValueError):
        env.plan_place_guard(pa.long(), me, fv)
    with pytest.raises(ValueError):
        env.plan_place_guard(pa, me, fv, base=env.plan_field(horizon=5).vis)
    env.close()
    # a handle without any emitter slot: the candidate needs none
    bare = HeistEnv(2, _cfg(G, G, H), max_cams=0, max_guards=0, max_path=MP, device=gpu_device, auto_reset=False)
    bare.set_layouts([(pr.WALLROW, [], [])] * 2, budget=gr.BUDGET)
    bare.reset()
    twin = _make(2, _cfg(G, G, H), gpu_device)
    _set(twin, [(pr.WALLROW, [], [gr.guard_dict(gr.PREMISE["jump"])]), (pr.WALLROW, [], [gr.guard_dict(gr.PREMISE["rectangle"])])],
         gr.BUDGET)
    pa, me, fv = (x.unsqueeze(1) for x in _arr([gr.PREMISE["jump"], gr.PREMISE["rectangle"]]))
    assert bare.plan_place_guard_supported == 1
    pp = bare.plan_place_guard(pa, me, fv, gamma=0.99, cells=True)
    pf, pv = twin.plan_field(), twin.plan_value(gamma=0.99)
    assert bool(pp.valid.all())
    for e in range(2):
        _assert_twin(pp, e, 0, pf, pv, e, (SR, SC), "no emitter slots, env %d" % e)
    bare.close()
    twin.close()


# ---- 6. the launch only reads the env

def test_plan_place_guard_reads_only(gpu_device, monkeypatch):
    """64 lean-served 20 x 20 envs with the shared fan table in use: the saved state is byte-equal
    before and after plan_place_guard(), and the next 20-tick heist_step_multi_records launch is
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
    pa, me, fv = (x[:, 100:108] for x in guard_candidates(a.grid_snapshot()))
    pp = a.plan_place_guard(pa, me, fv, horizon=50, gamma=0.99)
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
    R, C, N, M, P, Hh = 10, 13, 3, 2, 4, 4
    env = _make(N, _cfg(R, C, 50), gpu_device)
    env.set_layouts([([], [], [])] * N, budget=10)
    env.reset()
    assert env.plan_place_guard_supported == env.plan_place_supported == 1
    two = [gr.cand([(5, 5), (5, 6)]), gr.cand([])]
    pa, me, fv = _arr(two, p=P)
    assert env.plan_place_guard(pa, me, fv, horizon=1024).vis.shape[0] == 1024
    _einval(lambda: env.plan_place_guard(pa, me, fv, horizon=0))
    _einval(lambda: env.plan_place_guard(pa, me, fv, horizon=1025))
    for bad in (float("nan"), float("inf"), -float("inf"), -0.01, 1.01):
        _einval(lambda: env.plan_place_guard(pa, me, fv, gamma=bad))
    _einval(lambda: env.plan_place_guard(torch.zeros((N, 0, P, 2), dtype=torch.int32), torch.zeros((N, 0, 4), dtype=torch.int32),
                                         torch.zeros((N, 0, 2), dtype=torch.float64)))
    W, RC = record_words(R, C), R * C
    kw = dict(device=gpu_device)
    path = torch.zeros(N * M * P * 2 + 1, dtype=torch.int32, **kw)
    path[:-1] = pa.reshape(1, -1).expand(N, -1).reshape(-1).to(gpu_device)
    meta = torch.zeros(N * M * 4 + 1, dtype=torch.int32, **kw)
    meta[:-1] = me.reshape(1, -1).expand(N, -1).reshape(-1).to(gpu_device)
    fov = torch.zeros(N * M * 2 + 1, dtype=torch.float64, **kw)
    fov[:-1] = fv.reshape(1, -1).expand(N, -1).reshape(-1).to(gpu_device)
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
    good = [nat.ptr(path), nat.ptr(meta), nat.ptr(fov), nat.ptr(base), nat.ptr(valid), nat.ptr(ticks), nat.ptr(value),
            nat.ptr(action), nat.ptr(vis), nat.ptr(tcells), nat.ptr(vcells)]
    call = lambda *a, M_=M, P_=P: lib.heist_plan_place_guard(env._h, Hh, 0.99, M_, P_, *a, st)  # noqa: E731
    assert call(*good) == 0
    torch.cuda.synchronize(gpu_device)
    assert valid[:N * M].tolist() == [1, 0] * N
    want_t, want_v = tcells[:N * M * RC].clone(), vcells[:N * M * RC].clone()
    want = (ticks[:N * M].clone(), value[:N * M].clone(), action[:N * M].clone(), vis[:Hh * N * M * W].clone())
    pf, pv = env.plan_field(horizon=Hh), env.plan_value(horizon=Hh, gamma=0.99)
    assert torch.equal(want_t.reshape(N, M, R, C)[:, 1], pf.togo) and _same(want_v.reshape(N, M, R, C)[:, 1], pv.value)
    assert torch.equal(want[3].reshape(Hh, N, M, W)[:, :, 1], pf.vis)
    # the optional outputs, each alone and neither
    for tc, vc in ((None, good[10]), (good[9], None), (None, None)):
        ticks.zero_(), value.zero_(), action.zero_(), tcells.zero_(), vcells.zero_()
        assert call(*good[:9], tc, vc) == 0
        torch.cuda.synchronize(gpu_device)
        assert torch.equal(ticks[:N * M], want[0]) and _same(value[:N * M], want[1]) and torch.equal(action[:N * M], want[2])
        assert tc is None or torch.equal(tcells[:N * M * RC], want_t)
        assert vc is None or _same(vcells[:N * M * RC], want_v)
        assert tc is not None or not tcells.any()
        assert vc is not None or not _bits(vcells).any()
    # 4-byte alignment is enough for the int32 arrays, 8-byte for the float64 ones, 2-byte for the int16 ones
    path[1:] = path[:-1].clone()
    meta[1:] = meta[:-1].clone()
    fov[1:] = fov[:-1].clone()
    assert call(nat.ptr(path[1:]), nat.ptr(meta[1:]), nat.ptr(fov[1:]), good[3], nat.ptr(valid[1:]), nat.ptr(ticks[1:]),
                nat.ptr(value[1:]), nat.ptr(action[1:]), good[8], nat.ptr(tcells[1:]), nat.ptr(vcells[1:])) == 0
    torch.cuda.synchronize(gpu_device)
    assert torch.equal(ticks[1:], want[0]) and _same(value[1:], want[1]) and _same(vcells[1:], want_v)
    assert valid[1:].tolist() == [1, 0] * N
    path[:-1], meta[:-1], fov[:-1] = path[1:].clone(), meta[1:].clone(), fov[1:].clone()
    for i in range(9):  # every required pointer
        args = list(good)
        args[i] = None
        assert call(*args) == HEIST_EINVAL
    assert call(*good, M_=0) == HEIST_EINVAL and call(*good, M_=-1) == HEIST_EINVAL
    assert call(*good, P_=0) == HEIST_EINVAL and call(*good, P_=65) == HEIST_EINVAL and call(*good, P_=-1) == HEIST_EINVAL
    assert vis.data_ptr() % 16 == 0 and base.data_ptr() % 16 == 0 and value.data_ptr() % 8 == 0
    for i, t in ((3, base), (8, vis)):  # 16-byte alignment of the two row arrays
        for off in (1, 2):
            args = list(good)
            args[i] = nat.ptr(t[off:])
            assert call(*args) == HEIST_EINVAL
    for i, t in ((2, fov), (6, value), (10, vcells)):
        args = list(good)
        args[i] = nat.ptr(t.view(torch.int32)[1:])  # 4 bytes past an 8-byte boundary
        assert call(*args) == HEIST_EINVAL
    for i, t in ((0, path), (1, meta)):
        args = list(good)
        args[i] = nat.ptr(t.view(torch.int16)[1:])  # 2 bytes past a 4-byte boundary
        assert call(*args) == HEIST_EINVAL
    for i, t in ((5, ticks), (9, tcells)):
        args = list(good)
        args[i] = nat.ptr(t.view(torch.int8)[1:])   # an odd address
        assert call(*args) == HEIST_EINVAL
    assert lib.heist_plan_place_guard(None, Hh, 0.99, M, P, *good, st) == HEIST_EINVAL
    assert lib.heist_plan_place_guard_supported(None) == -1
    torch.cuda.synchronize(gpu_device)
    env.close()
    # 64 x 64: not supported, as for plan_place
    big = _make(2, _cfg(64, 64, 50), gpu_device)
    assert big.plan_place_guard_supported == 0 and big.plan_place_supported == 0
    _einval(lambda: big.plan_place_guard(pa, me, fv, horizon=4, base=torch.zeros((4, 2, record_words(64, 64)),
                                                                                 dtype=torch.int32, device=gpu_device)))
    big.close()
    monkeypatch.setenv("HEIST_PROBE_MODE", "1")
    probe = _make(3, _cfg(20, 20, 60), gpu_device)
    assert probe.kernel_config()["probe_mode"] == 1
    _einval(lambda: probe.plan_place_guard(pa, me, fv, base=torch.zeros((60, 3, record_words(20, 20)), dtype=torch.int32,
                                                                        device=gpu_device)))
    probe.close()


def test_rows_outside_the_contract(gpu_device):
    """Ordinary rejected inputs: INT32_MIN / INT32_MAX in each meta and path word, NaN, +-inf and -0.0 in each
    fov word, len = P + 1, idx = len.  Each is invalid and leaves the base rows' plan, except the words the
    contract takes any value of (speed) or that value of (a heading of -0.0)."""
    env = _make(1, _cfg(G, G, H), gpu_device)
    _set(env, [gr.BASE], gr.BUDGET)
    P = 4
    ok_path, ok_meta, ok_fov = [(2, 2), (2, 3), (3, 3)], [3, 1, 4, 0], [90.0, 0.0]
    rows, expect = [], []

    def add(path=None, meta=None, fov=None, valid=False):
        pts = list(ok_path if path is None else path)
        pts = pts + [(I32_MIN, I32_MAX)] * (P - len(pts))
        rows.append((pts, list(ok_meta if meta is None else meta), list(ok_fov if fov is None else fov)))
        expect.append(valid)

    add(valid=True)
    for word in range(4):
        for v in (I32_MIN, I32_MAX):
            m = list(ok_meta)
            m[word] = v
            add(meta=m, valid=word == 1)   # any speed is taken: step = speed mod len
    for j in range(3):
        for k in range(2):
            for v in (I32_MIN, I32_MAX):
                pts = [list(q) for q in ok_path]
                pts[j][k] = v
                add(path=[tuple(q) for q in pts])
    for word in range(2):
        for v in (float("nan"), float("inf"), -float("inf"), -0.0):
            f = list(ok_fov)
            f[word] = v
            add(fov=f, valid=(word == 1 and v == 0.0))   # a heading of -0.0 is within bounds; a fov of -0.0 is not > 0
    add(meta=[P + 1, 1, 4, 0])   # len = P + 1
    add(meta=[3, 1, 4, 3])       # idx = len
    add(meta=[0, 1, 4, 0])       # len = 0
    add(meta=[3, 1, 4, -1])      # idx < 0
    add(meta=[3, 1, -1, 0])
    add(meta=[3, 1, 32768, 0])
    add(fov=[16000.5, 0.0])
    add(fov=[90.0, 1.1e300])
    # at the contract's bounds: valid
    add(meta=[3, -7, 32767, 2], fov=[16000.0, -1e300], valid=True)
    add(meta=[3, 5, 0, 1], fov=[1e-300, 1e300], valid=True)
    pa = torch.tensor([r[0] for r in rows], dtype=torch.int64).to(torch.int32)
    me = torch.tensor([r[1] for r in rows], dtype=torch.int64).to(torch.int32)
    fv = torch.tensor([r[2] for r in rows], dtype=torch.float64)
    pp = env.plan_place_guard(pa, me, fv, gamma=0.99, horizon=8, cells=True)
    assert pp.valid[0].tolist() == expect
    pf, pv = env.plan_field(horizon=8), env.plan_value(horizon=8, gamma=0.99)
    base = pf.vis[:, 0]
    for m, ok in enumerate(expect):
        if ok:
            assert torch.equal(pp.vis[:, 0, m] & base, base) and not torch.equal(pp.vis[:, 0, m], base), rows[m]
        else:
            _assert_twin(pp, 0, m, pf, pv, 0, pr.START, "row %r" % (rows[m],))
    # speed INT32_MIN and INT32_MAX are the steps Python's % gives: -2^31 % 3 = 1, (2^31 - 1) % 3 = 1: the plain candidate
    assert torch.equal(pp.vis[:, 0, 3], pp.vis[:, 0, 0]) and torch.equal(pp.vis[:, 0, 4], pp.vis[:, 0, 0])
    # range 32767 from (3, 3) after one backward step (speed -7 mod 3 = 2, idx 2 -> 1: (2, 3)): the exact path runs to the walls
    assert bool(pp.vis_mask(1, len(rows) - 2)[0, 2, 3])
    _check_padding(pp, [8])
    env.close()


# ---- 8. monotone where it must be

def test_monotone(gpu_device):
    n, R, budget, max_steps = 16, 20, 15, 60
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=R, max_steps=max_steps)
    env = HeistEnv(n, cfg, max_cams=MC, max_guards=MG, max_path=MP, device=gpu_device, auto_reset=False)
    env.set_layouts(synthetic_layouts(n, R, R, budget, seed=77), budget=budget)
    env.reset()
    grid = env.grid_snapshot()
    pa, me, fv = guard_candidates(grid)
    pf, pv = env.plan_field(), env.plan_value()
    pp = env.plan_place_guard(pa, me, fv, base=pf.vis)
    t0, v0 = pf.togo[:, 1, 1].reshape(-1, 1), pv.value[:, 1, 1].reshape(-1, 1)
    big = lambda t: torch.where(t < 0, torch.full_like(t, 30000), t)  # noqa: E731  -1 counts as largest
    assert bool((big(pp.ticks) >= big(t0)).all()), "one more guard never shortens the way"
    assert bool((big(pp.ticks) > big(t0)).any()), "some guard costs the Solver ticks"
    assert bool((pp.value <= v0).all()), "nor raises the optimal return: every play earns no more under more visibility"
    assert bool((pp.value < v0).any())
    assert torch.equal(pp.ticks[~pp.valid], t0.expand_as(pp.ticks)[~pp.valid])
    assert _same(pp.value[~pp.valid], v0.expand_as(pp.value)[~pp.valid])
    base = pf.vis.unsqueeze(2)
    assert torch.equal(pp.vis & base, base.expand_as(pp.vis)), "every row holds its base row"
    # valid exactly where the patrol start is EMPTY: the tile up-left of (r, c), clamped
    start = grid[:, pa[0, :, 0, 0].long(), pa[0, :, 0, 1].long()]
    assert torch.equal(pp.valid, start == 0) and torch.equal(pp.valid, me[:, :, 0] == 8)
    print("valid %d of %d, blocking %d, slower %d" % (int(pp.valid.sum()), pp.valid.numel(),
                                                      int(((pp.ticks < 0) & (t0 > 0)).sum()), int((pp.ticks > t0).sum())))
    env.close()


# ---- 9. the Architect's patrol is the decode kernel's

def test_architect_patrol_is_the_decode_kernels(gpu_device):
    from heist_amd.architect_decode import decode_layouts
    R, C = 7, 9
    tiles = [(r, c) for r in range(1, R - 1) for c in range(1, C - 1)]
    amap = torch.zeros((len(tiles), R, C), dtype=torch.int64, device=gpu_device)
    for e, (r, c) in enumerate(tiles):
        amap[e, r, c] = 3   # one guard, on another tile in every layout
    cam = torch.zeros((len(tiles), 3), dtype=torch.float32, device=gpu_device)
    lb = decode_layouts(amap, cam, budget=5, max_walls=4, max_cams=1, max_guards=1, max_path=MP)
    assert lb.n_guards.tolist() == [1] * len(tiles)
    paths = lb.guard_paths.cpu()
    for e, (r, c) in enumerate(tiles):
        assert [tuple(v) for v in paths[e, 0, :8].tolist()] == architect_patrol(r, c, R, C), (r, c)
    assert lb.guard_meta[:, 0].cpu().tolist() == [[8, 1, 4]] * len(tiles) and lb.guard_fov[:, 0].cpu().tolist() == [90.0] * len(tiles)
    gp, gm, gf = guard_candidates(torch.zeros((1, R, C), dtype=torch.int8))
    assert torch.equal(gp[0], paths[:, 0, :8].to(torch.int32)) and gm[0, 0].tolist() == [8, 1, 4, 0] and gf[0, 0].tolist() == [90.0, 0.0]


# ---- 10. guard_placement_scan: chunks of M give one call's tables

def test_guard_placement_scan_chunking(gpu_device):
    env = _make(2, _cfg(G, G, H), gpu_device)
    _set(env, [gr.BASE, (pr.WALLROW, [pr.cam(90, 0)], [])], gr.BUDGET)
    cands = guard_candidates(env.grid_snapshot())
    M = cands[0].shape[1]
    assert M == (G - 2) * (G - 2)
    one = env.plan_place_guard(*cands, gamma=0.99)
    per = 4 * H * 2 * record_words(G, G)
    calls = []
    inner = env.plan_place_guard

    def spy(p, m, f, **kw):
        calls.append(int(torch.as_tensor(p).shape[-3]))
        return inner(p, m, f, **kw)
    env.plan_place_guard = spy
    whole = guard_placement_scan(env, cands, gamma=0.99)
    assert calls == [1, M]
    del calls[:]
    parts = guard_placement_scan(env, cands, gamma=0.99, max_bytes=7 * per + 5)
    assert calls == [1] + [7] * (M // 7) + [M % 7]
    env.plan_place_guard = inner
    pf, pv = env.plan_field(), env.plan_value(gamma=0.99)
    for sc in (whole, parts):
        assert isinstance(sc, PlacementScan)
        assert torch.equal(sc.valid, one.valid) and torch.equal(sc.ticks, one.ticks) and _same(sc.value, one.value)
        assert torch.equal(sc.action, one.action) and all(torch.equal(a, b) for a, b in zip(sc.cands[:2], cands[:2]))
        assert torch.equal(sc.ticks0, pf.togo[:, SR, SC]) and _same(sc.value0, pv.value[:, SR, SC])
    assert whole.ticks0.tolist() == [22, -1]
    b = whole.best()
    assert int(b[1]) == -1 and int(b[0]) >= 0 and float(whole.headroom()[1]) == 0.0
    assert float(whole.headroom()[0]) == float(whole.value0[0]) - float(whole.value[0, int(b[0])])
    elig = (whole.valid[0] & (whole.ticks[0] >= 0)).cpu().numpy()
    v = whole.value[0].cpu().numpy()
    assert elig[int(b[0])] and int(b[0]) == int(np.nonzero(elig & (v == v[elig].min()))[0][0])
    assert float(whole.blocking()[1]) == 0.0 and 0.0 <= float(whole.blocking()[0]) < 1.0
    assert set(whole.metrics("guard")) == {"guard_headroom_mean", "guard_blocking_frac", "guard_headroom_envs"}
    env.close()


# ---- 11. greedy_adversary: two rounds, re-derived through a twin handle

def test_greedy_adversary(gpu_device):
    N, budget, extra = 8, 15, 8
    cfg = _cfg(G, G, H)
    env = _make(N, cfg, gpu_device)
    lays = synthetic_layouts(N, G, G, budget, seed=14, n_cams=1, n_guards=1)
    _set(env, lays, budget)
    grid = env.grid_snapshot()
    cd = camera_candidates(grid, [0.0, 90.0, 180.0, 270.0], 60.0, 15.0, 6)
    gc = guard_candidates(grid)
    # round 1 by hand: the two scans and the selection rule
    cs, gs = placement_scan(env, cd, gamma=0.99), guard_placement_scan(env, gc, gamma=0.99)
    kind1, index1, gain1 = greedy_pick(cs, gs, extra)
    ga = greedy_adversary(env, extra, cd, gc, gamma=0.99, max_rounds=2)
    assert isinstance(ga, GreedyAdversary) and 1 <= len(ga.kind) <= 2
    assert torch.equal(ga.kind[0], kind1) and torch.equal(ga.index[0], index1)
    for e in range(N):
        k, i = int(kind1[e]), int(index1[e])
        if k >= 0:
            sc = cs if k == 0 else gs
            assert _same(ga.value[0][e], sc.value[e, i]) and int(ga.ticks[0][e]) == int(sc.ticks[e, i])
            assert float(gain1[e]) == (float(sc.value0[e]) - float(sc.value[e, i])) / (3 if k == 0 else 5) > 0.0
    spent = ga.spent.tolist()
    assert spent == [3 * len(ga.cameras[e]) + 5 * len(ga.guards[e]) for e in range(N)] and max(spent) <= extra
    print("greedy adversary: kinds", [k.tolist() for k in ga.kind], "spent", spent)
    assert any(len(g) for g in ga.guards) or any(len(c) for c in ga.cameras)
    # the layouts rebuilt with what was bought: the same rows, the predicted ticks and value
    got, spent0 = env.layout_lists()
    twins = [(w, c + ga.cameras[e], g + ga.guards[e]) for e, (w, c, g) in enumerate(got)]
    twin = _make(N, cfg, gpu_device, mc=MC + 2, mg=MG + 2)
    _set(twin, twins, [spent0[e] + spent[e] for e in range(N)])
    pf, pv = twin.plan_field(), twin.plan_value(gamma=0.99)
    assert torch.equal(pf.vis, ga.vis)
    assert _same(pv.value[:, SR, SC], ga.value[-1]) and torch.equal(pf.togo[:, SR, SC], ga.ticks[-1])
    solvable0 = env.plan_field().togo[:, SR, SC] >= 0
    assert torch.equal(pf.togo[:, SR, SC] >= 0, solvable0), "the adversary keeps a solvable layout solvable"
    assert bool((pv.value[:, SR, SC] <= env.plan_value(gamma=0.99).value[:, SR, SC]).all())
    env.close()
    twin.close()


# ---- 12. trainer

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
    return {"guard_headroom_mean": float(np.sum(head) / len(head)) if head else 0.0,
            "guard_blocking_frac": float(np.sum(block) / len(block)) if block else 0.0,
            "guard_headroom_envs": len(head)}


def test_trainer_track_guard_headroom(gpu_device, tmp_path):
    from heist_amd.training import AdversarialTrainer
    outs, seen = {}, []
    for track in (False, True):
        cfg = EnvironmentConfig(grid_rows=G, grid_cols=G, max_steps=H)
        d = tmp_path / str(track)
        tr = AdversarialTrainer(cfg, solver_episodes_per_layout=1, total_episodes=10 ** 6, save_dir=str(d / "ck"),
                                log_dir=str(d / "logs"), n_envs=32, rollout_len=16, device=gpu_device, seed=0,
                                minibatch=256, track_guard_headroom=track, headroom_envs=8)
        inner = tr._guard_headroom_layout_batch

        def spy(env_ids, tr=tr, inner=inner):  # the state of every scanned batch, as the trainer saw it
            seen.append(tr.env.save_state([int(i) for i in env_ids][:8]))
            inner(env_ids)
        tr._guard_headroom_layout_batch = spy
        tr.global_episode = 200  # curriculum phase with cameras and guards
        tr._assign_layouts(np.arange(32))
        n_seen = len(seen)
        outs[track] = tr.train_iteration()
        if track:
            assert n_seen >= 1
            twin = HeistEnv(len(seen[-1]), cfg, max_cams=tr.env.max_cams, max_guards=tr.env.max_guards,
                            max_path=tr.env.max_path, device=gpu_device, auto_reset=True)
            assert bool(twin.load_state(seen[-1]).all())
            sc = guard_placement_scan(twin, guard_candidates(twin.grid_snapshot()), gamma=1.0)
            want = _metrics_restated(sc.valid, sc.ticks, sc.value, sc.ticks0, sc.value0)
            assert sc.metrics("guard") == pytest.approx(want, rel=1e-12, abs=0.0)
            twin.close()
            assert tr._headroom_env is not None
        else:
            assert not seen and tr._headroom_env is None
        tr.close()
        assert tr._headroom_env is None
    keys = {"guard_headroom_mean", "guard_blocking_frac", "guard_headroom_envs"}
    assert set(outs[True]) == set(outs[False]) | keys and not keys & set(outs[False])
    # the count is exact.  The two means are float64 sums of at most 8 terms taken in another order:
    # a relative 1e-12 is a thousand times their rounding
    for k in sorted(keys):
        print(k, outs[True][k], want[k])
        if k.endswith("_envs"):
            assert outs[True][k] == want[k], k
        else:
            assert outs[True][k] == pytest.approx(want[k], rel=1e-12, abs=0.0), k
    assert outs[True]["guard_headroom_envs"] >= 1
