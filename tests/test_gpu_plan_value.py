"""heist_plan_value (HeistEnv.plan_value): the optimal discounted Solver return from every cell, the
first optimal action, every tick's visibility plane and the values and actions of every later
tick, in one launch.  Every comparison is equality, float64 through its bits (int64), except the
exhaustive lookahead's, whose returns are summed in the other order (bound stated there).

Yardsticks, none of which uses the kernel under test: the NumPy recurrence (value_ref.py) on the C
oracle's witness planes and on the launch's own visibility rows (which are pinned to
heist_plan_field's); the env kernels' float64 rewards of replays through heist_step_multi;
exhaustive_lookahead over all 5^4 action sequences.
"""
import numpy as np
import pytest
import torch

import field_ref as fr
import plan_ref as pr
import value_ref as vr
from heist_amd import EnvironmentConfig, HeistEnv, PlanValue, _native as nat, exhaustive_lookahead
from heist_amd.layouts import synthetic_layouts
from heist_amd.obs_compact import record_words
from heist_amd.search import N_ACTIONS, discounted_return, follow_value, value_targets

pytestmark = pytest.mark.gpu

HEIST_EINVAL = 100000
MC, MG, MP = 5, 3, 16
NAMES = list(pr.CASES)
GAMMAS = (1.0, 0.99)


def _cfg(R, C, max_steps, start=(1, 1)):
    return EnvironmentConfig(grid_rows=R, grid_cols=C, max_steps=max_steps, start_pos=start, architect_budget=C + 10)


def _make(n, cfg, dev, cones=True):
    env = HeistEnv(n, cfg, max_cams=MC, max_guards=MG, max_path=MP, device=dev, auto_reset=False)
    env.set_guard_cones(cones)
    return env


def _edit(env, e, cell=None, tick=None):
    """Env e's Solver parked on `cell` through a saved state: the EnvScalars follow the blob's
    64-byte header (pos_r, pos_c, tick, done, detected, vault_reached, prev_dist, ...: int32 each);
    prev_dist is written as the cell's distance to the vault, which every reset and step keeps."""
    st = env.save_state([e])
    scal = st.blobs[0, 64:112].view(torch.int32)
    if cell is not None:
        vr_, vc_ = env.config.vault_pos
        scal[0], scal[1] = cell
        scal[6] = abs(cell[0] - vr_) + abs(cell[1] - vc_)
    if tick is not None:
        scal[2] = tick
    assert bool(env.load_state(st, env_ids=[e]).all())


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check_padding(pv, HK):
    """Bits past R C and words past ceil(R C / 32) are 0; rows >= HK[e] are 0 (vis), 0.0 and -1."""
    RC = pv.rows * pv.cols
    words = pv.vis.cpu().numpy().view(np.uint32)
    nvis = (RC + 31) // 32
    assert not words[:, :, nvis:].any(), "words past ceil(RC/32) must be 0"
    if RC % 32:
        assert not (words[:, :, nvis - 1] >> (RC % 32)).any(), "bits past RC must be 0"
    for e, hk in enumerate(HK):
        assert not words[hk:, e].any(), "env %d: vis rows >= HK must be 0" % e
        if pv.value_ticks is not None:
            assert not _bits(pv.value_ticks[hk:, e]).any(), "env %d: value rows >= HK must be +0.0" % e
        if pv.action_ticks is not None:
            assert bool((pv.action_ticks[hk:, e] == -1).all()), "env %d: action rows >= HK must be -1" % e


def _restate(pv, x, e, tick0, max_steps):
    """value_ref.value_from_planes for env e on the launch's own unpacked visibility rows."""
    H = pv.vis.shape[0]
    masks = torch.stack([pv.vis_mask(k)[e] for k in range(1, H + 1)]).cpu().numpy()
    walls = (x["grid"][e] == 1).cpu().numpy()
    return vr.value_from_planes(walls, pv.vault, list(masks), int(x["initial_dist"][e]), tick0, max_steps, pv.gamma,
                                done=bool(x["done"][e]))


def _assert_equals_ref(pv, e, ref, what):
    value, action, vt, at = ref
    HK = vt.shape[0]
    np.testing.assert_array_equal(vr.bits(pv.value[e].cpu().numpy()), vr.bits(value), what)
    np.testing.assert_array_equal(pv.action[e].cpu().numpy(), action, what)
    if pv.value_ticks is not None:
        np.testing.assert_array_equal(vr.bits(pv.value_ticks[:HK, e].cpu().numpy()), vr.bits(vt), what)
        np.testing.assert_array_equal(pv.action_ticks[:HK, e].cpu().numpy(), at, what)


# ---- 1. the 10 x 10 fixtures against the recurrence on the oracle's witness planes

def _table_env(dev):
    """plan_ref.CASES (the six BFS-valid fixtures and full_wallrow) in one handle; the env of
    start_on_vault gets its Solver's cell by a saved state (its initial_dist stays the handle's)."""
    cfg = _cfg(pr.GRID, pr.GRID, pr.MAX_STEPS)
    env = _make(len(NAMES), cfg, dev)
    env.set_layouts([pr.CASES[n][0] for n in NAMES], budget=pr.BUDGET)
    env.reset()
    _edit(env, NAMES.index("start_on_vault"), pr.VAULT)
    return env


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_fixture_table(gpu_device, monkeypatch, waves):
    monkeypatch.setenv("HEIST_MULTI_WAVES", str(waves))
    env = _table_env(gpu_device)
    assert env.kernel_config()["multi_waves"] == waves and env.plan_value_supported == 1
    H, N, G = pr.MAX_STEPS, len(NAMES), pr.GRID
    W = record_words(G, G)
    for gamma in (1.0, 0.99, 0.0):
        pv = env.plan_value(gamma=gamma, all_ticks=True)
        assert isinstance(pv, PlanValue) and pv.gamma == gamma
        assert pv.value.shape == (N, G, G) and pv.value.dtype == torch.float64
        assert pv.action.shape == (N, G, G) and pv.action.dtype == torch.int8
        assert pv.vis.shape == (H, N, W) and pv.vis.dtype == torch.int32
        assert pv.value_ticks.shape == (H, N, G, G) and pv.value_ticks.dtype == torch.float64
        assert pv.action_ticks.shape == (H, N, G, G) and pv.action_ticks.dtype == torch.int8
        assert (pv.rows, pv.cols, pv.vault) == (G, G, pr.VAULT) and pv.grid.shape == (N, G, G)
        masks = torch.stack([pv.vis_mask(k) for k in range(1, H + 1)]).cpu().numpy()  # [H, N, R, C]
        for i, n in enumerate(NAMES):
            planes, walls = fr.case_reference(n)[:2]
            diff = [k + 1 for k in range(H) if (masks[k, i] != planes[k]).any()]
            assert not diff, "%s: vis differs from the witnesses first at tick %d" % (n, diff[0])
            _assert_equals_ref(pv, i, vr.case_value(n, gamma), "%s gamma %r" % (n, gamma))
            wm = torch.from_numpy(walls).to(gpu_device)
            assert not _bits(pv.value_ticks[:, i][:, wm]).any(), n  # +0.0 on walls
            assert bool((pv.action_ticks[:, i][:, wm] == -1).all()), n
            assert bool((pv.action_ticks[:, i][:, ~wm] >= 0).all()), n
        _check_padding(pv, [H] * N)
    # (gamma is 0.0 here) without all_ticks; a horizon past max_steps: HK = max_steps, the rows after it empty
    lean = env.plan_value(gamma=0.0)
    assert lean.value_ticks is None and lean.action_ticks is None
    assert _same(lean.value, pv.value) and torch.equal(lean.action, pv.action) and torch.equal(lean.vis, pv.vis)
    g = env.plan_value(horizon=H + 8, gamma=0.0, all_ticks=True)
    assert g.vis.shape[0] == H + 8
    assert torch.equal(g.vis[:H], pv.vis) and _same(g.value_ticks[:H], pv.value_ticks)
    assert torch.equal(g.action_ticks[:H], pv.action_ticks)
    assert _same(g.value, pv.value) and torch.equal(g.action, pv.action)
    _check_padding(g, [H] * N)
    # the pinned start-cell values at gamma 1
    one = env.plan_value(gamma=1.0)
    assert float(one.value[NAMES.index("empty")][pr.START]) == 15.899999999999995
    assert float(one.value[NAMES.index("wallrow_fixed_cam")][pr.START]) == 0.5714285714285716
    env.close()


# ---- 2. larger shapes: vis pinned to plan_field's, the values to the recurrence on those rows

def _shape_env(name, dev):
    R, C, max_steps, cones = fr.SHAPES[name]
    cfg = _cfg(R, C, max_steps)
    lays = fr.shape_layouts(R, C, seed=R * 100 + C)
    env = _make(len(lays), cfg, dev, cones)
    env.set_layouts(lays, budget=C + 10)
    env.reset()
    assert env.plan_value_supported == 1 and env.kernel_config()["guard_cones"] == (1 if cones else 0)
    return env, lays


@pytest.mark.parametrize("name", sorted(fr.SHAPES))
def test_shapes_equal_restatement(gpu_device, name):
    R, C, max_steps, _ = fr.SHAPES[name]
    env, lays = _shape_env(name, gpu_device)
    field_vis = env.plan_field().vis
    x = env.export(grid=True)
    longer = 0
    for gamma in GAMMAS:
        pv = env.plan_value(gamma=gamma, all_ticks=True)
        assert torch.equal(pv.vis, field_vis), "vis differs from plan_field's"
        assert torch.equal(pv.grid, x["grid"])
        for e in range(len(lays)):
            ref = _restate(pv, x, e, 0, max_steps)
            _assert_equals_ref(pv, e, ref, "%s env %d gamma %r" % (name, e, gamma))
            print("%s env %d gamma %r: V0[start] %r" % (name, e, gamma, float(pv.value[e, 1, 1])))
        _check_padding(pv, [max_steps] * len(lays))
        longer += int((pv.value[:, 1, 1] > 5).sum())
    assert longer >= 2  # some layouts pay the vault's reward from the start
    assert any(g["vision_range"] > 7 for lay in lays for g in lay[2])  # a guard raycast live
    env.close()


# ---- 3. against the env kernels: the value's own play collects exactly the value

@pytest.mark.parametrize("name", sorted(fr.SHAPES))
def test_follow_value_collects_the_value(gpu_device, name):
    R, C, max_steps, _ = fr.SHAPES[name]
    nvis = (R * C + 31) // 32
    for gamma in GAMMAS:
        env, lays = _shape_env(name, gpu_device)
        n = len(lays)
        pv = env.plan_value(gamma=gamma, all_ticks=True)
        start = torch.ones(n, dtype=torch.int64, device=gpu_device)
        acts = follow_value(pv, start, start)
        assert acts.shape == (max_steps, n) and acts.dtype == torch.int64
        records, _, done, _, r64 = env.step_multi_records(acts, auto_reset=False, reward64=True)
        assert bool(done[-1].all())  # every env ends by max_steps
        ret = discounted_return(r64, done, gamma)
        v0 = pv.value[:, 1, 1]
        print(name, gamma, "V0[start]", v0.tolist(), "episode ticks", (done.int().argmax(0) + 1).tolist())
        assert _same(ret, v0), (ret.tolist(), v0.tolist())
        # value_targets along the played cells equals the Horner tail of the same rewards at every tick
        word = records[:, :, nvis].cpu().numpy()
        pos_r, pos_c = np.ones((max_steps, n), np.int64), np.ones((max_steps, n), np.int64)
        pos_r[1:], pos_c[1:] = (word & 0xFF)[:-1], ((word >> 8) & 0xFF)[:-1]
        val, act = value_targets(pv, torch.from_numpy(pos_r).to(gpu_device), torch.from_numpy(pos_c).to(gpu_device))
        val, act = val.cpu().numpy(), act.cpu().numpy()
        r64, done, acts = r64.cpu().numpy(), done.cpu().numpy(), acts.cpu().numpy()
        for e in range(n):
            T = int(np.argmax(done[:, e])) + 1
            tails = [vr.horner(r64[k:T, e], gamma) for k in range(T)]
            np.testing.assert_array_equal(vr.bits(val[:T, e]), vr.bits(np.array(tails)), "env %d" % e)
            assert list(act[:T, e]) == list(acts[:T, e]), e
            assert not acts[T:, e].any(), e
        env.close()


# ---- 4. optimality: no action sequence does better

def _lookahead(env, roots, depth, what):
    B = N_ACTIONS ** depth
    x = env.export()
    cells = [(int(x["pos_r"][i]), int(x["pos_c"][i])) for i in roots]
    pv = env.plan_value(horizon=depth, gamma=1.0)
    v0 = torch.stack([pv.value[i][cells[k]] for k, i in enumerate(roots)]).cpu().numpy()
    res = exhaustive_lookahead(env, roots, depth)
    assert res.returns.shape == (len(roots), B)
    ret = res.returns.cpu().numpy()
    c = env.config
    # the two summation orders (tick order there, from the back here) of depth terms, each at most
    # the sum of the reward's parts in magnitude: depth roundings of at most 2^-52 times that sum
    bound = depth * 2.0 ** -52 * depth * (abs(c.reward_step) + 0.1 + 0.15 + abs(c.reward_detection) +
                                          abs(c.reward_vault) + 2)
    for k in range(len(roots)):
        print("%s root %d at %s: V0 %r, best of %d sequences %r" % (what, roots[k], cells[k], v0[k], B, ret[k].max()))
        assert abs(ret[k].max() - v0[k]) <= bound, (what, k, ret[k].max(), v0[k])
        assert (ret[k] - v0[k]).max() <= bound, (what, k)
    return v0


def test_optimal_against_exhaustive_lookahead(gpu_device):
    depth = 4
    B = N_ACTIONS ** depth
    G, H = pr.GRID, pr.MAX_STEPS
    layout = pr.CASES["wallrow_both"][0]
    # the next tick's plane (the oracle's; test 1 pins the kernel's to it) picks the cone's cells
    planes, walls = fr.case_reference("wallrow_both")[:2]
    mv, seen, wall = fr.moves(walls).reshape(5, -1), planes[0].reshape(-1), walls.reshape(-1)
    inside = [c for c in range(G * G) if not wall[c] and all(seen[mv[a][c]] for a in range(5))]
    edge = [c for c in range(G * G) if not wall[c] and seen[c] and not all(seen[mv[a][c]] for a in range(5))]
    cells = [(7, 8), divmod(inside[0], G), divmod(edge[0], G), (7, 7)]  # next to the vault; the cone; the last ticks
    m = len(cells)
    env = _make(m + m * B, _cfg(G, G, H), gpu_device)
    env.set_layouts([layout] * m + [([], [], [])] * (m * B), budget=pr.BUDGET)
    env.reset()
    for i, cell in enumerate(cells):
        _edit(env, i, cell, tick=H - 2 if i == m - 1 else None)
    x = env.export()
    assert x["tick"][:m].tolist() == [0, 0, 0, H - 2] and bool((x["initial_dist"][:m] > 3).all())
    v0 = _lookahead(env, list(range(m)), depth, "wallrow_both")
    assert v0[0] > 9 and v0[1] < 0  # the vault is one move away; every move from inside the cone is seen
    env.close()
    # a handle whose start lies within 3 of the vault: D0 = 2, no proximity bonus anywhere
    near = _make(1 + B, _cfg(G, G, H, start=(7, 7)), gpu_device)
    near.set_layouts([layout] + [([], [], [])] * B, budget=pr.BUDGET)
    near.reset()
    assert int(near.export()["initial_dist"][0]) == 2
    _lookahead(near, [0], depth, "start (7, 7)")
    near.close()


# ---- 5. mid-episode state, horizons, the timeout, done envs

def test_mid_episode_and_horizons(gpu_device):
    R = C = pr.GRID
    H = pr.MAX_STEPS
    cfg = _cfg(R, C, H)
    lays = fr.shape_layouts(R, C, seed=7)
    # a camera that never turns and looks along row 1 at the start cell: detected on tick 1
    lays.append(([], [{"row": 1, "col": 4, "fov_angle": 60.0, "vision_range": 6, "heading": 180.0,
                       "rotation_speed": 0.0}], []))
    N = len(lays)
    env = _make(N, cfg, gpu_device)
    env.set_layouts(lays, budget=C + 10)
    env.reset()
    x0 = env.export(grid=True)
    p0 = env.plan_value(gamma=0.99, all_ticks=True)
    start = torch.ones(N, dtype=torch.int64, device=gpu_device)
    acts = follow_value(p0, start, start)
    # horizon 5: the horizon-truncated return, on the first five rows
    p5 = env.plan_value(horizon=5, gamma=0.99, all_ticks=True)
    assert torch.equal(p5.vis, p0.vis[:5])
    for e in range(N):
        _assert_equals_ref(p5, e, _restate(p5, x0, e, 0, H), "horizon 5 env %d" % e)
    assert not _same(p5.value, p0.value)
    played = 0
    for k in (3, 7):
        env.step_multi(acts[played:k], auto_reset=False)
        played = k
        x = env.export()
        live = x["done"] == 0
        assert bool((x["tick"][live] == k).all()) and int(live.sum()) >= 3
        pk = env.plan_value(horizon=H - k, gamma=0.99, all_ticks=True)
        assert _same(pk.value[live], p0.value_ticks[k][live]), "after %d ticks" % k
        assert torch.equal(pk.action[live], p0.action_ticks[k][live])
        assert _same(pk.value_ticks[:, live], p0.value_ticks[k:, live])
        assert torch.equal(pk.action_ticks[:, live], p0.action_ticks[k:, live])
        assert torch.equal(pk.vis[:, live], p0.vis[k:, live])
        gone = ~live
        assert bool(gone[-1]) and not _bits(pk.value[gone]).any() and bool((pk.action[gone] == -1).all())
        assert not pk.vis[:, gone].any()
        _check_padding(pk, [0 if g else H - k for g in gone.tolist()])
        # the default horizon is cut at max_steps - tick
        pd = env.plan_value(gamma=0.99)
        assert _same(pd.value, pk.value) and not pd.vis[H - k:].any()
    env.close()
    # one tick before the timeout: one step, the timeout's share of the reward included
    late = _make(2, cfg, gpu_device)
    late.set_layouts([([], [], []), lays[-1]], budget=C + 10)
    late.reset()
    late.step_multi(torch.zeros((H - 1, 2), dtype=torch.int64), auto_reset=False)
    x = late.export(grid=True)
    assert int(x["tick"][0]) == H - 1 and x["done"].tolist() == [0, 1]
    pl = late.plan_value(all_ticks=True)
    _assert_equals_ref(pl, 0, _restate(pl, x, 0, H - 1, H), "tick = max_steps - 1")
    assert float(pl.value[0, 1, 1]) == -0.01 + 1.0 * 0.1 + (1.0 - 13.0 / 14.0) * 2.0
    # the env already done: nothing to collect, no visibility rows
    assert not _bits(pl.value[1]).any() and bool((pl.action[1] == -1).all()) and not pl.vis[:, 1].any()
    _check_padding(pl, [1, 0])
    late.close()


# ---- 6. the launch only reads the env

def test_plan_value_reads_only(gpu_device, monkeypatch):
    """64 lean-served 20 x 20 envs with the shared fan table in use: the saved state is equal
    before and after plan_value(), and the next 20-tick heist_step_multi launch is bit-identical
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
    pv = a.plan_value(horizon=50, gamma=0.99, all_ticks=True)
    assert int((pv.value > 5).sum()) > 0
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
    R, C = 13, 17
    env = _make(3, _cfg(R, C, 50), gpu_device)
    env.set_layouts([([], [], [])] * 3, budget=10)
    env.reset()
    assert env.plan_value_supported == env.plan_field_supported == 1
    assert env.plan_value(horizon=1024).vis.shape[0] == 1024
    _einval(lambda: env.plan_value(horizon=0))
    _einval(lambda: env.plan_value(horizon=1025))
    for bad in (float("nan"), float("inf"), -float("inf"), -0.01, 1.01):
        _einval(lambda: env.plan_value(gamma=bad))
    H, W = 4, record_words(R, C)
    kw = dict(device=gpu_device)
    value = torch.empty(3 * R * C + 1, dtype=torch.float64, **kw)
    action = torch.empty((3, R * C), dtype=torch.int8, **kw)
    vis = torch.empty(H * 3 * W + 4, dtype=torch.int32, **kw)
    vticks = torch.empty(H * 3 * R * C + 1, dtype=torch.float64, **kw)
    aticks = torch.empty(H * 3 * R * C + 1, dtype=torch.int8, **kw)
    lib, st = nat.lib(), env._stream()
    good = [nat.ptr(value), nat.ptr(action), nat.ptr(vis), nat.ptr(vticks), nat.ptr(aticks)]
    call = lambda *a: lib.heist_plan_value(env._h, H, 0.99, *a, st)  # noqa: E731
    assert call(*good) == 0
    torch.cuda.synchronize(gpu_device)
    want_v, want_a = value[:3 * R * C].clone(), aticks[:3 * R * C].clone()
    assert _same(vticks[:3 * R * C], want_v) and torch.equal(action.reshape(-1), want_a)
    # the optional outputs, each alone and neither
    for vt, at in ((None, good[4]), (good[3], None), (None, None)):
        value.zero_()
        assert call(*good[:3], vt, at) == 0
        torch.cuda.synchronize(gpu_device)
        assert _same(value[:3 * R * C], want_v)
    # 8-byte alignment is enough for the float64 outputs, any for the int8 ones
    assert call(nat.ptr(value[1:]), good[1], good[2], nat.ptr(vticks[1:]), nat.ptr(aticks[1:])) == 0
    torch.cuda.synchronize(gpu_device)
    assert _same(value[1:], want_v) and torch.equal(aticks[1:1 + 3 * R * C], want_a)
    for i in range(3):
        args = list(good)
        args[i] = None
        assert call(*args) == HEIST_EINVAL
    assert vis.data_ptr() % 16 == 0 and value.data_ptr() % 8 == 0
    assert call(good[0], good[1], nat.ptr(vis[1:]), good[3], good[4]) == HEIST_EINVAL
    odd = value.view(torch.int32)[1:]   # 4 bytes past an 8-byte boundary
    assert call(nat.ptr(odd), *good[1:]) == HEIST_EINVAL
    assert call(good[0], good[1], good[2], nat.ptr(vticks.view(torch.int32)[1:]), good[4]) == HEIST_EINVAL
    assert lib.heist_plan_value(None, H, 0.99, *good, st) == HEIST_EINVAL and lib.heist_plan_value_supported(None) == -1
    torch.cuda.synchronize(gpu_device)
    env.close()
    # 64 x 64: the two value arrays alone fill a workgroup's 64 KB of LDS -- not supported
    big = _make(2, _cfg(64, 64, 50), gpu_device)
    assert big.plan_value_supported == 0
    _einval(lambda: big.plan_value(horizon=4))
    big.close()
    monkeypatch.setenv("HEIST_PROBE_MODE", "1")
    probe = _make(3, _cfg(20, 20, 60), gpu_device)
    assert probe.kernel_config()["probe_mode"] == 1
    _einval(lambda: probe.plan_value())
    probe.close()


# ---- 8. trainer

def test_trainer_track_optimal_return(gpu_device, tmp_path):
    from heist_amd.training import AdversarialTrainer
    outs, seen = {}, []
    for track in (False, True):
        cfg = EnvironmentConfig(grid_rows=20, grid_cols=20, max_steps=200)
        d = tmp_path / str(track)
        tr = AdversarialTrainer(cfg, solver_episodes_per_layout=1, total_episodes=10 ** 6, save_dir=str(d / "ck"),
                                log_dir=str(d / "logs"), n_envs=16, rollout_len=16, device=gpu_device, seed=0,
                                minibatch=256, track_optimal_return=track)
        inner = tr._value_layout_batch

        def spy(env_ids, tr=tr, inner=inner):  # the state of every valued batch, as the trainer saw it
            seen.append(tr.env.save_state([int(i) for i in env_ids]))
            inner(env_ids)
        tr._value_layout_batch = spy
        tr.global_episode = 200  # curriculum phase with cameras and guards
        tr._assign_layouts(np.arange(16))
        n_seen = len(seen)
        outs[track] = tr.train_iteration()
        if track:
            assert n_seen >= 1
            twin = HeistEnv(len(seen[-1]), cfg, max_cams=tr.env.max_cams, max_guards=tr.env.max_guards,
                            max_path=tr.env.max_path, device=gpu_device, auto_reset=True)
            assert bool(twin.load_state(seen[-1]).all())
            want = float(twin.plan_value(gamma=1.0).value[:, cfg.start_pos[0], cfg.start_pos[1]].mean())
            twin.close()
        else:
            assert not seen
        tr.env.close()
    assert set(outs[True]) == set(outs[False]) | {"optimal_return_mean"}
    assert outs[True]["optimal_return_mean"] == want
    assert -1.5 <= want <= 200 * 0.15 + 10 + 2  # detected on tick 1 .. the bonus every tick, the vault, the timeout
