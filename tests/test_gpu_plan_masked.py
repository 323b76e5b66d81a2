"""heist_plan_masked (HeistEnv.plan_masked / plan_ablate): every env planned under M sets of its
emitters in one launch -- the fewest ticks, the optimal return and first action from the Solver's
cell, every variant's visibility planes and the whole tick-0 tables.  Every comparison is equality,
float64 through its bits (int64).

Yardsticks, none of which uses the kernel under test: masked_ref (the C oracle on layouts with the
switched-off emitters removed from their lists, and the NumPy recurrences on its witness planes);
heist_plan_field / heist_plan_value on the same handle (all emitters on) and on twin handles whose
layouts lack the emitter (leave-one-out) or hold the walls alone (all off).
"""
import numpy as np
import pytest
import torch

import field_ref as fr
import masked_ref as mr
import plan_ref as pr
import value_ref as vr
from heist_amd import EnvironmentConfig, HeistEnv, PlanAblation, PlanMasked, _native as nat, ablation_masks
from heist_amd.layouts import synthetic_layout, synthetic_layouts
from heist_amd.obs_compact import record_words

pytestmark = pytest.mark.gpu

HEIST_EINVAL = 100000
MC, MG, MP = 5, 3, 16
NAMES = list(mr.FIXTURES)
G, H = pr.GRID, pr.MAX_STEPS
SR, SC = pr.START


def _cfg(R, C, max_steps, start=(1, 1)):
    return EnvironmentConfig(grid_rows=R, grid_cols=C, max_steps=max_steps, start_pos=start, architect_budget=C + 10)


def _make(n, cfg, dev, cones=True, mc=MC, mg=MG):
    env = HeistEnv(n, cfg, max_cams=mc, max_guards=mg, max_path=MP, device=dev, auto_reset=False)
    env.set_guard_cones(cones)
    return env


def _set(env, lays, budget):
    """Layouts set and reset, every emitter of every layout bought (a budget that drops one would
    make a twin's shorter list buy another)."""
    valid = env.set_layouts(lays, budget=budget)
    env.reset()
    x = env.export()
    assert bool(valid.all())
    assert x["n_cams"].tolist() == [len(l[1]) for l in lays] and x["n_guards"].tolist() == [len(l[2]) for l in lays]
    return x


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _planes(pm, e, m):
    """[H, R, C] bool: variant (e, m)'s visibility rows unpacked."""
    return torch.stack([pm.vis_mask(k, m)[e] for k in range(1, pm.vis.shape[0] + 1)]).cpu().numpy()


def _check_padding(pm, HK):
    """Bits past R C and words past ceil(R C / 32) are 0; rows >= HK[e] are 0."""
    RC = pm.rows * pm.cols
    words = pm.vis.cpu().numpy().view(np.uint32)  # [H, N, M, W]
    nvis = (RC + 31) // 32
    assert not words[..., nvis:].any(), "words past ceil(RC/32) must be 0"
    if RC % 32:
        assert not (words[..., nvis - 1] >> (RC % 32)).any(), "bits past RC must be 0"
    for e, hk in enumerate(HK):
        assert not words[hk:, e].any(), "env %d: vis rows >= HK must be 0" % e


def _fixture_env(dev, cones=True, mc=MC, mg=MG):
    env = _make(len(NAMES), _cfg(G, G, H), dev, cones, mc, mg)
    _set(env, [mr.FIXTURES[n] for n in NAMES], mr.BUDGET)
    return env


def _fixture_masks(mc, M=5):
    """(ons, masks): ons[i][m] the (cameras on, guards on) key of variant (i, m) -- the fixture's
    own variants, padded with its all-on variant -- and masks int64 [N, M]."""
    ons = [(mr.variants(n) + [mr.variants(n)[0]] * M)[:M] for n in NAMES]
    return ons, torch.tensor([[mr.mask_word(on, mc) for on in row] for row in ons], dtype=torch.int64)


def _assert_variant(pm, i, m, ref, what, planes=True):
    T = ref["ticks"]
    assert int(pm.ticks[i, m]) == T, what
    assert vr.bits(float(pm.value[i, m])) == vr.bits(ref["value"][pr.START]), what
    assert int(pm.action[i, m]) == int(ref["action"][pr.START]), what
    if pm.togo_cells is not None:
        np.testing.assert_array_equal(pm.togo_cells[i, m].cpu().numpy(), ref["togo"], what)
        np.testing.assert_array_equal(vr.bits(pm.value_cells[i, m].cpu().numpy()), vr.bits(ref["value"]), what)
    if planes:
        got = _planes(pm, i, m)
        diff = [k + 1 for k in range(got.shape[0]) if (got[k] != ref["planes"][k]).any()]
        assert not diff, "%s: vis differs from the witnesses first at tick %d" % (what, diff[0])


# ---- 1. the fixture table against the oracle on the reduced layouts

@pytest.mark.parametrize("cones", [True, False], ids=["cached_guards", "live_guards"])
@pytest.mark.parametrize("waves", [1, 2, 4])
def test_fixture_table(gpu_device, monkeypatch, waves, cones):
    monkeypatch.setenv("HEIST_MULTI_WAVES", str(waves))
    env = _fixture_env(gpu_device, cones)
    kc = env.kernel_config()
    assert kc["multi_waves"] == waves and kc["guard_cones"] == (1 if cones else 0) and env.plan_masked_supported == 1
    ons, masks = _fixture_masks(MC)
    N, M, W = len(NAMES), masks.shape[1], record_words(G, G)
    for gamma in (1.0, 0.99, 0.0):
        pm = env.plan_masked(masks, gamma=gamma, cells=True)
        assert isinstance(pm, PlanMasked) and pm.gamma == gamma and torch.equal(pm.masks.cpu(), masks)
        assert pm.ticks.shape == (N, M) and pm.ticks.dtype == torch.int16
        assert pm.value.shape == (N, M) and pm.value.dtype == torch.float64
        assert pm.action.shape == (N, M) and pm.action.dtype == torch.int8
        assert pm.vis.shape == (H, N, M, W) and pm.vis.dtype == torch.int32
        assert pm.togo_cells.shape == (N, M, G, G) and pm.togo_cells.dtype == torch.int16
        assert pm.value_cells.shape == (N, M, G, G) and pm.value_cells.dtype == torch.float64
        assert pm.tick.tolist() == [0] * N
        for i, n in enumerate(NAMES):
            for m, on in enumerate(ons[i]):
                ref = mr.reference(n, on, gamma)
                assert ref["ticks"] == mr.TICKS[n][on]
                print("%s %r gamma %r: ticks %d value %r" % (n, on, gamma, int(pm.ticks[i, m]), float(pm.value[i, m])))
                _assert_variant(pm, i, m, ref, "%s %r gamma %r" % (n, on, gamma), planes=gamma == 1.0)
                wm = torch.from_numpy(ref["walls"]).to(gpu_device)
                assert bool((pm.togo_cells[i, m][wm] == -1).all()) and not _bits(pm.value_cells[i, m][wm]).any()
        _check_padding(pm, [H] * N)
    lean = env.plan_masked(masks, gamma=0.0)
    assert lean.togo_cells is None and lean.value_cells is None
    assert torch.equal(lean.ticks, pm.ticks) and _same(lean.value, pm.value) and torch.equal(lean.vis, pm.vis)
    env.close()


# ---- 2. identity variants: all on = plan_field / plan_value here, all off = a twin of walls alone

def test_identity_variants(gpu_device):
    env = _fixture_env(gpu_device)
    twin = _make(len(NAMES), _cfg(G, G, H), gpu_device)
    _set(twin, [(mr.FIXTURES[n][0], [], []) for n in NAMES], mr.BUDGET)
    e = torch.arange(len(NAMES), device=gpu_device)
    # [M] masks, broadcast over the envs; every bit set: the bits of unfilled slots are ignored
    for gamma in (1.0, 0.99):
        pm = env.plan_masked(torch.tensor([-1, 0]), gamma=gamma, cells=True)
        assert pm.masks.shape == (len(NAMES), 2)
        for m, h in ((0, env), (1, twin)):
            pf, pv = h.plan_field(), h.plan_value(gamma=gamma)
            assert torch.equal(pm.togo_cells[:, m], pf.togo) and _same(pm.value_cells[:, m], pv.value), (m, gamma)
            assert torch.equal(pm.ticks[:, m], pf.togo[e, SR, SC]) and _same(pm.value[:, m], pv.value[e, SR, SC])
            assert torch.equal(pm.action[:, m], pv.action[e, SR, SC])
            assert torch.equal(pm.vis[:, :, m], pf.vis) and torch.equal(pf.vis, pv.vis)
    assert pm.ticks[:, 0].tolist() == [22, -1, -1, 22, 32] and pm.ticks[:, 1].tolist() == [14] * 5
    env.close()
    twin.close()


# ---- 3. leave-one-out variants against twin handles whose layouts lack the emitter

SHAPES = {"13x17": (13, 17, 50, 3, 2, 29), "20x20": (20, 20, 60, 5, 3, 46), "32x32": (32, 32, 80, 5, 3, 52)}


def shape_layouts(name):
    """Two layouts of the shape with every slot filled (walls from the budget's rest); the first
    guard of the second layout sees 8 tiles: off the cone cache, raycast live every tick.  A guard
    is placed without a placement check and its start tile replaces a wall under it
    (set_layout_kernel), so a layout without that guard would have one wall more: such walls are
    left out, and the test compares the twins' wall planes."""
    R, C, _, nc, ng, budget = SHAPES[name]
    rng = np.random.Generator(np.random.PCG64(100 * R + C))
    lays = [synthetic_layout(rng, R, C, budget, n_cams=nc, n_guards=ng) for _ in range(2)]
    lays = [([w for w in walls if w not in {g["patrol_path"][0] for g in guards}], cams, guards)
            for walls, cams, guards in lays]
    lays[1][2][0] = dict(lays[1][2][0], vision_range=8)
    return lays


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_leave_one_out_equals_twin(gpu_device, name):
    R, C, max_steps, nc, ng, budget = SHAPES[name]
    cfg = _cfg(R, C, max_steps)
    lays = shape_layouts(name)
    env = _make(len(lays), cfg, gpu_device)
    x = _set(env, lays, budget)
    assert env.plan_masked_supported == 1
    # the twin: every layout without its emitter j, one env per (layout, filled slot)
    reduced, where = [], {}
    for e, (walls, cams, guards) in enumerate(lays):
        for j in range(len(cams)):
            where[e, j] = len(reduced)
            reduced.append((walls, cams[:j] + cams[j + 1:], guards))
        for g in range(len(guards)):
            where[e, MC + g] = len(reduced)
            reduced.append((walls, cams, guards[:g] + guards[g + 1:]))
    twin = _make(len(reduced), cfg, gpu_device)
    _set(twin, reduced, budget)
    wall, twall = env.export(grid=True)["grid"] == 1, twin.export(grid=True)["grid"] == 1
    for (e, j), i in where.items():
        assert torch.equal(wall[e], twall[i]), "env %d without slot %d has other walls" % (e, j)
    masks = ablation_masks(x["n_cams"], x["n_guards"], MC, MG)
    assert masks.shape == (len(lays), 1 + MC + MG) and masks.device == x["n_cams"].device
    changed = 0
    for gamma in (1.0, 0.99):
        pm = env.plan_masked(masks, gamma=gamma, cells=True)
        pf, pv = twin.plan_field(), twin.plan_value(gamma=gamma)
        for e in range(len(lays)):
            for j in range(MC + MG):
                m, what = 1 + j, "%s env %d slot %d gamma %r" % (name, e, j, gamma)
                if (e, j) not in where:  # an unfilled slot: the all-on variant again
                    assert torch.equal(pm.togo_cells[e, m], pm.togo_cells[e, 0]), what
                    assert _same(pm.value_cells[e, m], pm.value_cells[e, 0]) and torch.equal(pm.vis[:, e, m], pm.vis[:, e, 0])
                    continue
                i = where[e, j]
                assert torch.equal(pm.togo_cells[e, m], pf.togo[i]), what
                assert _same(pm.value_cells[e, m], pv.value[i]), what
                assert int(pm.ticks[e, m]) == int(pf.togo[i, 1, 1]) and _same(pm.value[e, m], pv.value[i, 1, 1]), what
                assert int(pm.action[e, m]) == int(pv.action[i, 1, 1]), what
                assert torch.equal(pm.vis[:, e, m], pf.vis[:, i]), what
                changed += int(not torch.equal(pm.vis[:, e, m], pm.vis[:, e, 0]))
        _check_padding(pm, [max_steps] * len(lays))
    assert changed >= nc + ng  # the emitters matter: the planes of most variants differ from the full layout's
    env.close()
    twin.close()


# ---- 4. mid-episode state, horizons, the timeout, done envs

def test_mid_episode_and_horizons(gpu_device):
    name = "cam_guard"
    layout, plan = mr.FIXTURES[name], pr.CASES["wallrow_both"][3]  # the same layout: its canonical plan, 22 ticks
    seen_at_once = ([], [{"row": 1, "col": 4, "fov_angle": 60.0, "vision_range": 6, "heading": 180.0,
                          "rotation_speed": 0.0}], [])            # looks along row 1 at the start: done on tick 1
    env = _make(3, _cfg(G, G, H), gpu_device)
    _set(env, [layout, layout, seen_at_once], mr.BUDGET)
    ons = mr.variants(name)
    masks = torch.tensor([[mr.mask_word(on, MC) for on in ons]] * 3, dtype=torch.int64)
    pf0, pv0 = env.plan_field(all_ticks=True), env.plan_value(gamma=0.99, all_ticks=True)
    pm0 = env.plan_masked(masks, gamma=0.99)
    # horizon 5: the truncated plans, on the first five rows
    p5 = env.plan_masked(masks, horizon=5, gamma=0.99, cells=True)
    assert p5.vis.shape[0] == 5 and torch.equal(p5.vis, pm0.vis[:5])
    f5, v5 = env.plan_field(horizon=5), env.plan_value(horizon=5, gamma=0.99)
    assert torch.equal(p5.togo_cells[:, 0], f5.togo) and _same(p5.value_cells[:, 0], v5.value)
    assert p5.ticks.tolist() == [[-1] * 4] * 3 and not _same(p5.value, pm0.value)
    acts = torch.zeros((H, 3), dtype=torch.int64, device=gpu_device)
    acts[:len(plan), :2] = torch.tensor(plan, device=gpu_device).reshape(-1, 1)
    played = 0
    for k in (3, 7):
        env.step_multi(acts[played:k], auto_reset=False)
        played = k
        x = env.export()
        assert x["tick"].tolist()[:2] == [k, k] and x["done"].tolist() == [0, 0, 1]
        r, c = int(x["pos_r"][0]), int(x["pos_c"][0])
        pm = env.plan_masked(masks, gamma=0.99)
        assert pm.tick.tolist() == [k, k, -1]
        for e in (0, 1):
            # all on: the first call's tables of tick k at the cell the plan has reached
            assert int(pm.ticks[e, 0]) == int(pf0.togo_ticks[k][e, r, c]) == len(plan) - k
            assert _same(pm.value[e, 0], pv0.value_ticks[k][e, r, c])
            assert int(pm.action[e, 0]) == int(pv0.action_ticks[k][e, r, c])
            assert torch.equal(pm.vis[:H - k, e, 0], pv0.vis[k:, e]) and not pm.vis[H - k:, e].any()
            # the plan is unseen under the full layout, hence under every subset of it
            for m, on in enumerate(ons):
                T = mr.search(name, on, prefix=plan[:k])[0]
                print("after %d ticks, %r: %d" % (k, on, T))
                assert int(pm.ticks[e, m]) == T and T <= len(plan) - k, (k, on)
        # the env already done: no plan, nothing to collect, no visibility rows
        assert pm.ticks[2].tolist() == [-1] * 4 and not _bits(pm.value[2]).any() and pm.action[2].tolist() == [-1] * 4
        assert not pm.vis[:, 2].any()
        _check_padding(pm, [H - k, H - k, 0])
    pc = env.plan_masked(masks, cells=True)
    assert bool((pc.togo_cells[2] == -1).all()) and not _bits(pc.value_cells[2]).any()
    env.close()
    # one tick before the timeout: one step, the timeout's share of the reward included
    late = _make(2, _cfg(G, G, H), gpu_device)
    _set(late, [([], [], []), layout], mr.BUDGET)
    late.step_multi(torch.zeros((H - 1, 2), dtype=torch.int64), auto_reset=False)
    x = late.export()
    assert int(x["tick"][0]) == H - 1 and int(x["done"][0]) == 0
    pl = late.plan_masked(torch.tensor([-1, 0, 1 << MC]), cells=True)
    lf, lv = late.plan_field(), late.plan_value()
    assert torch.equal(pl.togo_cells[:, 0], lf.togo) and _same(pl.value_cells[:, 0], lv.value)
    assert torch.equal(pl.vis[:, :, 0], lf.vis) and not pl.vis[1:].any()
    assert pl.ticks[0].tolist() == [-1] * 3
    assert [float(v) for v in pl.value[0]] == [-0.01 + 1.0 * 0.1 + (1.0 - 13.0 / 14.0) * 2.0] * 3
    late.close()


# ---- 5. mask mechanics

def test_mask_mechanics(gpu_device):
    """A handle with 33 camera slots: the guard's bit is 33.  Garbage in the bits of unfilled slots
    and from max_cams + max_guards up changes nothing; repeated masks give identical columns."""
    mc, mg = 33, 1
    env = _make(len(NAMES), _cfg(G, G, H), gpu_device, mc=mc, mg=mg)
    x = _set(env, [mr.FIXTURES[n] for n in NAMES], mr.BUDGET)
    i = NAMES.index("cam_guard")
    junk = sum(1 << b for b in (1, 7, 31, 32, 34, 35, 47, 62, 63))  # camera slots 1 .. 32 are unfilled there; 34 up: no slot
    full, cam_off, guard_off, none = ((1,), (1,)), ((0,), (1,)), ((1,), (0,)), ((0,), (0,))
    cols = [(full, 0), (full, junk), (cam_off, 0), (cam_off, junk), (guard_off, junk), (full, 0), (cam_off, 0),
            (none, 0), (none, junk)]
    row = [mr.mask_word(on, mc, g) for on, g in cols]
    assert row[0] == 1 | 1 << 33 and row[4] < 0
    masks = torch.tensor([row] * len(NAMES), dtype=torch.int64)
    pm = env.plan_masked(masks, gamma=0.99, cells=True)
    assert pm.vis.shape == (H, len(NAMES), 9, record_words(G, G))
    for m, (on, g) in enumerate(cols):
        _assert_variant(pm, i, m, mr.reference("cam_guard", on, 0.99), "bit-33 guard, column %d" % m)
    for a, b in ((0, 1), (0, 5), (2, 3), (2, 6), (7, 8)):
        assert torch.equal(pm.togo_cells[i, a], pm.togo_cells[i, b]) and _same(pm.value_cells[i, a], pm.value_cells[i, b])
        assert torch.equal(pm.vis[:, i, a], pm.vis[:, i, b])
    # ablation_masks on this handle: the guard's column is 1 + 33
    ab = env.plan_ablate(gamma=0.99)
    assert isinstance(ab, PlanAblation) and ab.ticks.shape == (len(NAMES), 1 + mc + mg)
    assert ab.ticks[i, [0, 1, 1 + 33]].tolist() == [22, 16, 18] and ab.ticks[i, 2:1 + 33].tolist() == [22] * 32
    assert ab.filled[i].nonzero().reshape(-1).tolist() == [0, 33]
    assert ab.ticks_saved[i, [0, 33]].tolist() == [6, 4] and not ab.critical[i].any() and not ab.redundant[i].any()
    assert ab.critical[NAMES.index("fixed_cam")].tolist() == [True] + [False] * 33
    k = NAMES.index("two_fixed")
    assert not ab.critical[k].any() and ab.ticks[k].tolist() == [-1] * 35  # jointly blocking: no critical emitter
    # M = 1: the field's layout
    one = env.plan_masked(torch.full((len(NAMES), 1), -1, dtype=torch.int64), gamma=0.99)
    pf, pv = env.plan_field(), env.plan_value(gamma=0.99)
    assert one.vis.shape[2] == 1 and torch.equal(one.vis.reshape(pf.vis.shape), pf.vis)
    assert torch.equal(one.ticks[:, 0], pf.togo[:, SR, SC]) and _same(one.value[:, 0], pv.value[:, SR, SC])
    assert torch.equal(one.ticks[:, 0], ab.ticks[:, 0]) and _same(one.value[:, 0], ab.value[:, 0])
    with pytest.raises(ValueError):
        env.plan_masked(masks.to(torch.int32))
    with pytest.raises(ValueError):
        env.plan_masked(masks[:2])
    assert x["n_guards"][i] == 1
    env.close()


# ---- 6. the launch only reads the env

def test_plan_masked_reads_only(gpu_device, monkeypatch):
    """64 lean-served 20 x 20 envs with the shared fan table in use: the saved state is byte-equal
    before and after plan_ablate(), and the next 20-tick heist_step_multi launch is bit-identical
    to a twin's that never called it."""
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
    ab = a.plan_ablate(horizon=50, gamma=0.99)
    assert int(ab.filled.sum()) > n and bool((ab.credit > 0).any())
    assert torch.equal(a.save_state().blobs, before)
    out_a = a.step_multi(acts[4:], reward64=True)
    out_b = b.step_multi(acts[4:], reward64=True)
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
    assert env.plan_masked_supported == env.plan_value_supported == 1
    mk = torch.zeros((N, M), dtype=torch.int64)
    assert env.plan_masked(mk, horizon=1024).vis.shape[0] == 1024
    _einval(lambda: env.plan_masked(mk, horizon=0))
    _einval(lambda: env.plan_masked(mk, horizon=1025))
    for bad in (float("nan"), float("inf"), -float("inf"), -0.01, 1.01):
        _einval(lambda: env.plan_masked(mk, gamma=bad))
    _einval(lambda: env.plan_masked(torch.zeros((N, 0), dtype=torch.int64)))
    W, RC = record_words(R, C), R * C
    kw = dict(device=gpu_device)
    masks = torch.zeros(N * M + 1, dtype=torch.int64, **kw)
    ticks = torch.empty(N * M + 1, dtype=torch.int16, **kw)
    value = torch.empty(N * M + 1, dtype=torch.float64, **kw)
    action = torch.empty(N * M + 1, dtype=torch.int8, **kw)
    vis = torch.empty(Hh * N * M * W + 4, dtype=torch.int32, **kw)
    tcells = torch.empty(N * M * RC + 1, dtype=torch.int16, **kw)
    vcells = torch.empty(N * M * RC + 1, dtype=torch.float64, **kw)
    lib, st = nat.lib(), env._stream()
    good = [nat.ptr(masks), nat.ptr(ticks), nat.ptr(value), nat.ptr(action), nat.ptr(vis), nat.ptr(tcells), nat.ptr(vcells)]
    call = lambda *a, M_=M: lib.heist_plan_masked(env._h, Hh, 0.99, M_, *a, st)  # noqa: E731
    assert call(*good) == 0
    torch.cuda.synchronize(gpu_device)
    want_t, want_v = tcells[:N * M * RC].clone(), vcells[:N * M * RC].clone()
    want = (ticks[:N * M].clone(), value[:N * M].clone(), action[:N * M].clone())
    pf, pv = env.plan_field(horizon=Hh), env.plan_value(horizon=Hh, gamma=0.99)
    assert torch.equal(want_t.reshape(N, M, R, C)[:, 0], pf.togo) and _same(want_v.reshape(N, M, R, C)[:, 1], pv.value)
    # the optional outputs, each alone and neither
    for tc, vc in ((None, good[6]), (good[5], None), (None, None)):
        ticks.zero_(), value.zero_(), action.zero_(), tcells.zero_(), vcells.zero_()
        assert call(*good[:5], tc, vc) == 0
        torch.cuda.synchronize(gpu_device)
        assert torch.equal(ticks[:N * M], want[0]) and _same(value[:N * M], want[1]) and torch.equal(action[:N * M], want[2])
        assert tc is None or torch.equal(tcells[:N * M * RC], want_t)
        assert vc is None or _same(vcells[:N * M * RC], want_v)
        assert tc is not None or not tcells.any()
        assert vc is not None or not _bits(vcells).any()
    # 8-byte alignment is enough for the float64 arrays, 2-byte for the int16 ones, any for the int8 one
    assert call(nat.ptr(masks[1:]), nat.ptr(ticks[1:]), nat.ptr(value[1:]), nat.ptr(action[1:]), good[4],
                nat.ptr(tcells[1:]), nat.ptr(vcells[1:])) == 0
    torch.cuda.synchronize(gpu_device)
    assert torch.equal(ticks[1:], want[0]) and _same(value[1:], want[1]) and _same(vcells[1:], want_v)
    for i in range(5):  # every required pointer
        args = list(good)
        args[i] = None
        assert call(*args) == HEIST_EINVAL
    assert call(*good, M_=0) == HEIST_EINVAL and call(*good, M_=-1) == HEIST_EINVAL
    assert vis.data_ptr() % 16 == 0 and value.data_ptr() % 8 == 0
    args = list(good)
    args[4] = nat.ptr(vis[1:])
    assert call(*args) == HEIST_EINVAL
    for i, t in ((0, masks), (2, value), (6, vcells)):
        args = list(good)
        args[i] = nat.ptr(t.view(torch.int32)[1:])  # 4 bytes past an 8-byte boundary
        assert call(*args) == HEIST_EINVAL
    assert lib.heist_plan_masked(None, Hh, 0.99, M, *good, st) == HEIST_EINVAL
    assert lib.heist_plan_masked_supported(None) == -1
    torch.cuda.synchronize(gpu_device)
    env.close()
    # 64 x 64: not supported, as for plan_value
    big = _make(2, _cfg(64, 64, 50), gpu_device)
    assert big.plan_masked_supported == 0 and big.plan_value_supported == 0
    _einval(lambda: big.plan_masked(torch.zeros((2, 1), dtype=torch.int64), horizon=4))
    big.close()
    monkeypatch.setenv("HEIST_PROBE_MODE", "1")
    probe = _make(3, _cfg(20, 20, 60), gpu_device)
    assert probe.kernel_config()["probe_mode"] == 1
    _einval(lambda: probe.plan_masked(torch.zeros((3, 1), dtype=torch.int64)))
    probe.close()


# ---- 8. monotonicity: switching an emitter off never hurts the Solver

def test_monotone_in_the_emitter_set(gpu_device):
    n, R, budget = 256, 20, 15
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=R, max_steps=200)
    env = HeistEnv(n, cfg, max_cams=MC, max_guards=MG, max_path=MP, device=gpu_device, auto_reset=False)
    env.set_layouts(synthetic_layouts(n, R, R, budget, seed=77), budget=budget)
    env.reset()
    ab = env.plan_ablate(gamma=1.0)
    assert ab.ticks.shape == (n, 1 + MC + MG) and int(ab.filled.sum()) > n
    assert bool((ab.credit >= 0).all()), "an emitter's credit is never negative"
    assert not _bits(ab.credit[~ab.filled]).any() and bool((ab.credit > 0).any())
    t0, t1 = ab.ticks[:, :1], ab.ticks[:, 1:]
    assert bool(((t1 > 0) | (t0 < 0)).all()), "solvable with an emitter, solvable without it"
    both = (t0 > 0) & (t1 > 0)
    assert bool((t1 <= t0)[both].all()) and bool((ab.ticks_saved >= 0).all()) and bool((ab.ticks_saved > 0).any())
    print("critical %d, redundant %d of %d filled; unsolvable layouts %d" % (
        int(ab.critical.sum()), int(ab.redundant.sum()), int(ab.filled.sum()), int((t0 < 0).sum())))
    # random subsets, and the subsets of those subsets
    gen = torch.Generator().manual_seed(3)
    sub = torch.randint(0, 1 << (MC + MG), (n, 3), generator=gen)
    masks = torch.cat([torch.full((n, 1), -1, dtype=torch.int64), sub, sub & sub[:, [1, 2, 0]]], 1)
    pm = env.plan_masked(masks, gamma=1.0)
    assert torch.equal(pm.ticks[:, 0], ab.ticks[:, 0]) and _same(pm.value[:, 0], ab.value[:, 0])
    for wide, narrow in [(0, m) for m in range(1, 7)] + [(1, 4), (2, 4), (2, 5), (3, 5), (3, 6), (1, 6)]:
        tw, tn = pm.ticks[:, wide], pm.ticks[:, narrow]
        assert bool((pm.value[:, narrow] >= pm.value[:, wide]).all()), (wide, narrow)
        assert bool(((tn > 0) | (tw < 0)).all()) and bool((tn <= tw)[(tw > 0) & (tn > 0)].all()), (wide, narrow)
    env.close()


# ---- 9. trainer

def _metrics_restated(ticks, value, filled, mc):
    """The trainer's four figures from the leave-one-out tables, in NumPy."""
    t, v, f = ticks.cpu().numpy().astype(np.int64), value.cpu().numpy(), filled.cpu().numpy().astype(bool)
    unsolv = t[:, 0] < 0
    crit = f & (t[:, :1] < 0) & (t[:, 1:] > 0)
    red = f & (t[:, 1:] == t[:, :1]) & (v[:, 1:].view(np.int64) == v[:, :1].view(np.int64))
    credit = v[:, 1:] - v[:, :1]
    cam = np.arange(f.shape[1])[None, :] < mc
    mean = lambda sel: float(credit[sel].sum() / sel.sum()) if sel.any() else 0.0  # noqa: E731
    return {"critical_layout_frac": float((unsolv & crit.any(1)).sum() / unsolv.sum()) if unsolv.any() else 0.0,
            "redundant_emitter_frac": float(red.sum() / f.sum()) if f.any() else 0.0,
            "camera_credit_mean": mean(f & cam), "guard_credit_mean": mean(f & ~cam)}


def test_trainer_track_emitter_credit(gpu_device, tmp_path):
    from heist_amd.training import AdversarialTrainer
    outs, seen = {}, []
    for track in (False, True):
        cfg = EnvironmentConfig(grid_rows=20, grid_cols=20, max_steps=200)
        d = tmp_path / str(track)
        tr = AdversarialTrainer(cfg, solver_episodes_per_layout=1, total_episodes=10 ** 6, save_dir=str(d / "ck"),
                                log_dir=str(d / "logs"), n_envs=16, rollout_len=16, device=gpu_device, seed=0,
                                minibatch=256, track_emitter_credit=track)
        inner = tr._ablate_layout_batch

        def spy(env_ids, tr=tr, inner=inner):  # the state of every ablated batch, as the trainer saw it
            seen.append(tr.env.save_state([int(i) for i in env_ids]))
            inner(env_ids)
        tr._ablate_layout_batch = spy
        tr.global_episode = 200  # curriculum phase with cameras and guards
        tr._assign_layouts(np.arange(16))
        n_seen = len(seen)
        outs[track] = tr.train_iteration()
        if track:
            assert n_seen >= 1
            mc, mg = tr.env.max_cams, tr.env.max_guards
            twin = HeistEnv(len(seen[-1]), cfg, max_cams=mc, max_guards=mg, max_path=tr.env.max_path,
                            device=gpu_device, auto_reset=True)
            assert bool(twin.load_state(seen[-1]).all())
            x = twin.export()
            pm = twin.plan_masked(ablation_masks(x["n_cams"], x["n_guards"], mc, mg), gamma=1.0)
            filled = torch.from_numpy(mr.filled_flags(x["n_cams"].cpu().numpy(), x["n_guards"].cpu().numpy(), mc, mg))
            want = _metrics_restated(pm.ticks, pm.value, filled, mc)
            assert int(filled.sum()) > 0
            twin.close()
        else:
            assert not seen
        tr.env.close()
    keys = {"critical_layout_frac", "redundant_emitter_frac", "camera_credit_mean", "guard_credit_mean"}
    assert set(outs[True]) == set(outs[False]) | keys and not keys & set(outs[False])
    # the shares are ratios of counts: exact.  The means are float64 sums of at most 16 x n_slot exact
    # differences taken in another order: a relative 1e-12 is a thousand times their rounding
    for k in sorted(keys):
        print(k, outs[True][k], want[k])
        if k.endswith("_frac"):
            assert outs[True][k] == want[k], k
        else:
            assert outs[True][k] == pytest.approx(want[k], rel=1e-12, abs=0.0), k
