"""GPU tests of the fork inside a handle (heist_state_fork, HeistEnv.fork_state) and of its consumer
heist_amd.search.exhaustive_lookahead.

Bar: bit-exact.  A forked env must continue exactly as its source does -- rows, float32 and
float64 reward, done, status, saved blob, plan -- and exactly as an env filled by save_state +
load_state on a control handle does.  The status pins which guard cone blocks the fork copied
and which it kept; the continuation after each case reads every cone slot (auto-reset keeps the
guards walking for twice the longest patrol).
"""
import numpy as np
import pytest
import torch

import plan_ref as pr
from heist_amd import EnvironmentConfig, HeistEnv, exhaustive_lookahead
from heist_amd import _native as nat
from heist_amd.layouts import architect_patrol, synthetic_layouts
from heist_amd.search import N_ACTIONS

pytestmark = pytest.mark.gpu

HEIST_EINVAL = 100000
MAX_STEPS = 20  # every env times out and auto-resets inside the continuations
PRE = 7         # ticks played before the fork
MP = 16

# name -> rows, cols, envs, cameras, guards per layout, env vars of the handle
SIZES = {
    "10x10": (10, 10, 8, 2, 2, {}),
    "13x17": (13, 17, 8, 2, 2, {}),
    "20x20_lean": (20, 20, 64, 5, 3, {"HEIST_MULTI_WAVES": "1"}),
    "32x32": (32, 32, 8, 4, 3, {}),
}


def _budget(nc, ng):
    return 3 * nc + 5 * ng + 5  # five walls


def _layouts(n, R, C, nc, ng, seed):
    """Random layouts with nc cameras and ng guards on 8-point patrols of range 4 (cached); in every
    other layout the last guard sees 8 cells, which keeps it off the cone cache."""
    lays = synthetic_layouts(n, R, C, _budget(nc, ng), seed=seed, n_cams=nc, n_guards=ng)
    for e in range(0, n, 2):
        lays[e][2][-1]["vision_range"] = 8
    return lays


def _handle(name, dev, monkeypatch, n=None):
    R, C, n0, nc, ng, envvars = SIZES[name]
    for k, v in envvars.items():
        monkeypatch.setenv(k, v)
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=C, max_steps=MAX_STEPS, architect_budget=_budget(nc, ng))
    env = HeistEnv(n or n0, cfg, max_cams=nc, max_guards=ng, max_path=MP, device=dev)
    if name == "20x20_lean":
        kc = env.kernel_config()
        assert kc["lean"] == 1 and kc["multi_waves"] == 1, kc
    return env


def _actions(T, n, seed, dev):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 5, (T, n))).to(dev)


def _multi(env, acts, auto=True):
    o, r, d, s, r64 = env.step_multi(acts, auto_reset=auto, reward64=True)
    return {"obs": o.view(torch.int32), "reward": r.view(torch.int32), "reward64": r64.view(torch.int64), "done": d,
            "status": s}


def _single(env, acts, auto=True):
    out = {"obs": [], "reward": [], "reward64": [], "done": [], "status": []}
    for a in acts:
        o, r, d, s = env.step(a, auto_reset=auto)
        for k, v in (("obs", o), ("reward", r), ("reward64", env.reward64), ("done", d), ("status", s)):
            out[k].append(v.clone())
    res = {k: torch.stack(v) for k, v in out.items()}
    return {"obs": res["obs"].view(torch.int32), "reward": res["reward"].view(torch.int32),
            "reward64": res["reward64"].view(torch.int64), "done": res["done"], "status": res["status"]}


def _assert_cols_equal(run, a, b, ctx):
    """Columns a of every output equal columns b, bit for bit."""
    for k, v in run.items():
        x, y = v[:, a], v[:, b]
        if not torch.equal(x, y):
            t = int((x != y).reshape(x.shape[0], -1).any(1).nonzero()[0])
            raise AssertionError("%s: %s differs, first at tick %d" % (ctx, k, t))


def _assert_runs_equal(a, b, ctx):
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s" % (ctx, k)


def _guard_slots(env, blobs):
    """(live [m, G] bool, cached [m, G] bool) of saved blobs: n_guards is scalar 9 behind the 64-byte
    header, the guard records follow the cameras, hslot is byte 30 of a 32-byte record."""
    b = blobs.cpu()
    ng = b[:, 64 + 36:64 + 40].contiguous().view(torch.int32).reshape(-1)
    g0 = 64 + 48 + 32 * env.max_cams
    hslot = torch.stack([b[:, g0 + 32 * g + 30] for g in range(env.max_guards)], 1)
    live = torch.arange(env.max_guards).reshape(1, -1) < ng.reshape(-1, 1)
    return live, live & (hslot != 0xFF)


def _pairs(n):
    """Sources in the first half of the handle, destinations in the second; some sources twice."""
    half = n // 2
    dst = list(range(half, n))
    src = [i * 3 // 4 for i in range(half)]
    return src, dst


# -- 1. equals the blob fork -------------------------------------------------------------------
def _filled(name, dev, monkeypatch, how):
    """A handle whose envs were laid out, reset and played PRE ticks, and whose destinations were
    then filled from their sources by fork_state ("fork") or by save_state + load_state ("blob")."""
    R, C, n, nc, ng, _ = SIZES[name]
    env = _handle(name, dev, monkeypatch)
    env.set_layouts(_layouts(n, R, C, nc, ng, seed=R * 100 + C), budget=_budget(nc, ng))
    env.reset()
    _single(env, _actions(PRE, n, 3, dev))
    src, dst = _pairs(n)
    if how == "fork":
        status = env.fork_state(src, dst)
        assert status.dtype == torch.uint8 and status.device == env.device
        assert status.cpu().tolist() == [1] * len(dst)  # the destinations held other layouts
    else:
        st = env.save_state(sorted(set(src)))
        index = [sorted(set(src)).index(s) for s in src]
        assert bool(env.load_state(st, env_ids=dst, index=index).all())
    return env, src, dst


@pytest.mark.parametrize("name", list(SIZES))
def test_fork_equals_blob_fork(gpu_device, monkeypatch, name):
    R, C, n, nc, ng, _ = SIZES[name]
    env, src, dst = _filled(name, gpu_device, monkeypatch, "fork")
    ctl, _, _ = _filled(name, gpu_device, monkeypatch, "blob")
    x = env.export()
    assert bool((x["guard_idx"][src] != 0).any())  # guards off their patrol start
    live, cached = _guard_slots(env, env.save_state(src).blobs)
    assert bool(cached.any()) and bool((live & ~cached).any())  # cached guards beside uncached ones
    assert torch.equal(env.save_state(dst).blobs, env.save_state(src).blobs)
    assert torch.equal(env.save_state().blobs, ctl.save_state().blobs)
    K = 2 * MP  # >= 2 x the longest patrol (8 points), past MAX_STEPS: every env auto-resets
    acts = _actions(K, n, 4, gpu_device)
    acts[:, dst] = acts[:, src]
    run = _multi(env, acts)
    assert bool(run["done"].any())
    _assert_cols_equal(run, dst, src, name)
    _assert_runs_equal(run, _multi(ctl, acts), name + " control, K-tick launch")
    assert torch.equal(env.save_state().blobs, ctl.save_state().blobs)
    env.close()
    ctl.close()
    if name == "20x20_lean":  # the same ticks as single heist_step calls: the order array, the stale fan table
        for how in ("blob", "fork"):
            one, _, _ = _filled(name, gpu_device, monkeypatch, how)
            _assert_runs_equal(run, _single(one, acts), name + " single ticks after " + how)
            one.close()


# -- 2. cone paths -----------------------------------------------------------------------------
def _cam(r, c):
    return {"row": r, "col": c, "fov_angle": 70.0, "vision_range": 6, "heading": 45.0, "rotation_speed": 15.0}


def _guard(path, rng=4):
    return {"patrol_path": path, "speed": 1, "vision_range": rng, "fov_angle": 90.0}


LINE = [(14, c) for c in range(3, 9)]
WALLS = [(3, 3), (7, 12), (12, 7), (15, 15)]
# guard 0 and guard 1 cached (patrols of 8 and 6 points, range 4), guard 2 raycast live (range 8)
BASE = (WALLS, [_cam(10, 10)], [_guard(architect_patrol(5, 5, 20, 20)), _guard(LINE), _guard(architect_patrol(10, 14, 20, 20), 8)])
OTHER = ([(2, 9), (9, 2), (17, 9)], [_cam(6, 13)],
         [_guard(architect_patrol(12, 12, 20, 20)), _guard([(4, c) for c in range(10, 16)]), _guard(architect_patrol(15, 4, 20, 20))])
NO_GUARDS = (WALLS, [_cam(10, 10), _cam(4, 15)], [])


def _with_guard1(**kw):
    gs = [dict(g) for g in BASE[2]]
    gs[1] = dict(gs[1], **kw)
    return (BASE[0], BASE[1], gs)


# case -> (source layout, destination layout, destination laid out with the cone cache off, status)
CONE_CASES = {
    "other_layout": (BASE, OTHER, False, 1),
    "one_wall_cell": (BASE, (WALLS + [(16, 9)], BASE[1], BASE[2]), False, 1),
    "one_patrol_point": (BASE, _with_guard1(patrol_path=LINE[:5] + [(13, 7)]), False, 3),
    "guard_range": (BASE, _with_guard1(vision_range=3), False, 3),
    "same_layout_uncached": (BASE, BASE, True, 1),
    "no_guards": (NO_GUARDS, OTHER, False, 1),
}


def _cone_env(dev, case):
    """Four 20 x 20 envs: 0 the source, 1 the destination, 2 and 3 bystanders on OTHER."""
    src_lay, dst_lay, dst_off, want = CONE_CASES[case]
    cfg = EnvironmentConfig(grid_rows=20, grid_cols=20, max_steps=MAX_STEPS, architect_budget=30)
    env = HeistEnv(4, cfg, max_cams=2, max_guards=3, max_path=MP, device=dev)
    assert bool(env.set_layouts([src_lay, OTHER if dst_off else dst_lay, OTHER, OTHER], budget=30).all())
    if dst_off:  # the destination's cone blocks hold OTHER's cones; its guards of dst_lay raycast live
        env.set_guard_cones(False)
        env.set_layouts([dst_lay], budget=30, env_ids=[1])
        env.set_guard_cones(True)
    env.reset()
    _single(env, _actions(PRE, 4, 5, dev))
    return env, want


def _continue_equal(env, seed, ctx):
    K = 2 * 8  # twice the longest patrol
    acts = _actions(K, 4, seed, env.device)
    acts[:, 1] = acts[:, 0]
    run = _multi(env, acts)
    _assert_cols_equal(run, [1], [0], ctx)
    assert torch.equal(env.save_state([1]).blobs, env.save_state([0]).blobs), ctx
    return run


@pytest.mark.parametrize("case", list(CONE_CASES))
def test_cone_paths(gpu_device, case):
    env, want = _cone_env(gpu_device, case)
    live, cached = _guard_slots(env, env.save_state([0, 1]).blobs)
    if case == "no_guards":
        assert not bool(live[0].any())
    else:
        assert cached[0].tolist() == [True, True, False]
        dst_lay, dst_off = CONE_CASES[case][1:3]  # patrols are at most 8 points: the range decides
        assert cached[1].tolist() == [not dst_off and g["vision_range"] <= 7 for g in dst_lay[2]]
    assert env.fork_state([0], [1]).cpu().tolist() == [want]
    run = _continue_equal(env, 6, case)
    assert bool(run["done"].any())
    # both sides played on with different actions: the destination now holds the source's layout
    _single(env, _actions(5, 4, 7, gpu_device))
    assert not torch.equal(env.save_state([1]).blobs, env.save_state([0]).blobs)
    assert env.fork_state([0], [1]).cpu().tolist() == [1 if case == "no_guards" else 2]
    _continue_equal(env, 8, case + ", forked again")
    env.close()


# -- 3. rejections -----------------------------------------------------------------------------
def test_rejections(gpu_device, monkeypatch):
    name = "20x20_lean"
    R, C, _, nc, ng, _ = SIZES[name]
    n = 8
    envs = []
    for _ in range(2):  # [0] forks, [1] never does
        e = _handle(name, gpu_device, monkeypatch, n)
        e.set_layouts(_layouts(n, R, C, nc, ng, seed=77), budget=_budget(nc, ng))
        e.reset()
        _single(e, _actions(PRE, n, 9, gpu_device))
        envs.append(e)
    env, ctl = envs
    assert torch.equal(env.save_state().blobs, ctl.save_state().blobs)
    calls = [  # src, dst, accepted items
        ([0, -1, 2], [4, 5, 6], [True, False, True]),   # an id of -1
        ([0, 1], [n, 5], [False, True]),                # an id of n_envs
        ([0, n, 2], [4, 5, 6], [True, False, True]),
        ([3, 0], [3, 4], [False, True]),                # src == dst
        ([0, 1, 2], [5, 5, 6], [False, False, True]),   # a dst named twice: both rejected
        ([0, 4], [4, 5], [False, True]),                # a dst that is another item's src
        ([6, 7], [7, 6], [False, False]),               # a swap: each dst is the other's src
    ]
    touched = set()
    for src, dst, ok in calls:
        before = env.save_state().blobs.clone()
        status = env.fork_state(src, dst).cpu().tolist()
        after = env.save_state().blobs
        assert [s != 0 for s in status] == ok, (src, dst, status)
        assert all(s in (0, 1, 2) for s in status), status
        taken = {d: s for s, d, k in zip(src, dst, ok) if k}
        touched |= set(taken)
        for e in range(n):
            assert torch.equal(after[e], before[taken.get(e, e)]), (src, dst, e)
    rest = sorted(set(range(n)) - touched)
    assert rest == [0, 1, 2, 3, 7]
    acts = _actions(8, n, 10, gpu_device)
    a, b = _single(env, acts), _single(ctl, acts)
    for k in a:
        assert torch.equal(a[k][:, rest], b[k][:, rest]), k
    env.close()
    ctl.close()


# -- 4. arguments ------------------------------------------------------------------------------
def test_arguments(gpu_device, monkeypatch):
    env = _handle("10x10", gpu_device, monkeypatch)
    env.set_layouts([([], [], [])] * env.n_envs, budget=0)
    env.reset()
    _single(env, _actions(3, env.n_envs, 2, gpu_device))  # the solvers stand on different cells
    L, P, s = nat.lib(), nat.ptr, nat.stream(gpu_device)
    ids = torch.tensor([0, 1], dtype=torch.int32, device=gpu_device)
    dst = torch.tensor([2, 3], dtype=torch.int32, device=gpu_device)
    before = env.save_state().blobs.clone()
    assert L.heist_state_fork(env._h, P(ids), P(dst), -1, None, s) == HEIST_EINVAL
    assert b"m < 0" in L.heist_last_error()
    assert L.heist_state_fork(env._h, None, P(dst), 2, None, s) == HEIST_EINVAL
    assert b"null" in L.heist_last_error()
    assert L.heist_state_fork(env._h, P(ids), None, 2, None, s) == HEIST_EINVAL
    assert L.heist_state_fork(None, P(ids), P(dst), 2, None, s) == HEIST_EINVAL
    assert L.heist_state_fork(env._h, None, None, 0, None, s) == 0
    assert torch.equal(env.save_state().blobs, before)
    assert L.heist_state_fork(env._h, P(ids), P(dst), 2, None, s) == 0  # status_out may be NULL
    assert torch.equal(env.save_state([2, 3]).blobs, before[:2])
    with pytest.raises(ValueError):
        env.fork_state([0, 1], [2])
    with pytest.raises(ValueError):
        env.fork_state([], [])
    env.close()


# -- 5. planner agreement ----------------------------------------------------------------------
def test_plan_after_fork(gpu_device):
    R = C = pr.GRID
    lays = [pr.CASES[k][0] for k in pr.CASES if pr.CASES[k][1] == pr.START]
    lays.append((pr.WALLROW, [], [dict(pr.GUARD, vision_range=8)]))  # a guard the cone cache does not hold
    m = len(lays)
    assert m == 7
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=C, max_steps=pr.MAX_STEPS, start_pos=pr.START, vault_pos=pr.VAULT,
                            architect_budget=pr.BUDGET)
    env = HeistEnv(2 * m, cfg, max_cams=5, max_guards=3, max_path=MP, device=gpu_device, auto_reset=False)
    env.set_layouts(lays + lays[::-1], budget=pr.BUDGET)
    env.reset()
    for a in (4, 4, 0, 2):  # cameras have turned, guards are mid-patrol
        env.step(torch.full((2 * m,), a, dtype=torch.int64), auto_reset=False)
    src, dst = list(range(m)), list(range(m, 2 * m))
    status = env.fork_state(src, dst).cpu().tolist()
    assert all(s in (1, 2) for s in status), status  # the middle layout of lays + lays[::-1] meets itself
    before = env.save_state().blobs.clone()
    res = env.plan()
    assert torch.equal(env.save_state().blobs, before)
    assert int((res.ticks[src] > 0).sum()) >= 1 and int((res.ticks[src] == -1).sum()) >= 1
    assert torch.equal(res.ticks[dst], res.ticks[src])
    assert torch.equal(res.actions[:, dst], res.actions[:, src])
    assert torch.equal(res.reach[:, dst], res.reach[:, src])
    env.close()


# -- 6. lookahead ------------------------------------------------------------------------------
def _lookahead_cases():
    """Three of plan_ref.CASES, chosen on the CPU: one the planner solves within the depth, one it
    solves later, one it never solves."""
    depth = 3
    names = list(pr.CASES)
    within = next(n for n in names if 1 <= pr.CASES[n][2] <= depth)
    later = next(n for n in names if pr.CASES[n][2] > depth)
    never = next(n for n in names if pr.CASES[n][2] == -1)
    return depth, [within, later, never]


def test_exhaustive_lookahead(gpu_device):
    depth, names = _lookahead_cases()
    B = N_ACTIONS ** depth
    m = len(names)
    n = m + m * B
    assert n == 378
    cfg = EnvironmentConfig(grid_rows=pr.GRID, grid_cols=pr.GRID, max_steps=pr.MAX_STEPS, start_pos=pr.START,
                            vault_pos=pr.VAULT, architect_budget=pr.BUDGET)
    env = HeistEnv(n, cfg, max_cams=5, max_guards=3, max_path=MP, device=gpu_device, auto_reset=False)
    env.set_layouts([pr.CASES[k][0] for k in names] + [([], [], [])] * (m * B), budget=pr.BUDGET)
    env.reset()
    for i, k in enumerate(names):  # a case that starts elsewhere: its solver's cell through a saved state
        if pr.CASES[k][1] != pr.START:
            st = env.save_state([i])
            scal = st.blobs[0, 64:72].view(torch.int32)
            scal[0], scal[1] = pr.CASES[k][1]
            assert bool(env.load_state(st, env_ids=[i]).all())
    roots = list(range(m))
    root_state = env.save_state(roots)
    plan = env.plan()
    T = plan.ticks[:m].cpu().tolist()
    assert T == [pr.CASES[k][2] for k in names]
    assert any(1 <= t <= depth for t in T) and any(t > depth for t in T) and any(t == -1 for t in T)

    res = exhaustive_lookahead(env, roots, depth)
    assert res.returns.shape == (m, B) and res.returns.dtype == torch.float64
    assert res.first_reach.shape == (m, B) and res.first_reach.dtype == torch.int32
    assert res.best.shape == (m,) and res.best_actions.shape == (m, depth) and res.best_actions.dtype == torch.int64
    assert res.workers.cpu().tolist() == [list(range(m + i * B, m + (i + 1) * B)) for i in range(m)]
    first = res.first_reach.cpu().numpy()
    for i, t in enumerate(T):
        if 1 <= t <= depth:
            assert first[i][first[i] > 0].min() == t, names[i]
            seq = plan.actions[:t, i].cpu().tolist() + [0] * (depth - t)  # the canonical plan, then WAIT
            j = sum(a * N_ACTIONS ** (depth - 1 - k) for k, a in enumerate(seq))
            assert first[i, j] == t, names[i]
        else:
            assert (first[i] == -1).all(), names[i]

    # every sequence replayed tick by tick (heist_step) from the saved roots on a control handle
    ctl = HeistEnv(m * B, cfg, max_cams=5, max_guards=3, max_path=MP, device=gpu_device, auto_reset=False)
    assert bool(ctl.load_state(root_state, index=torch.arange(m).repeat_interleave(B)).all())
    digits = torch.tensor([[(j // N_ACTIONS ** (depth - 1 - k)) % N_ACTIONS for j in range(B)] for k in range(depth)])
    total = None
    for k in range(depth):
        ctl.step(digits[k].repeat(m), auto_reset=False)
        total = ctl.reward64.clone() if total is None else total + ctl.reward64
    assert torch.equal(res.returns, total.reshape(m, B))
    best = res.best.cpu().tolist()
    ret = res.returns.cpu().numpy()
    for i in range(m):
        assert best[i] == int(np.flatnonzero(ret[i] == ret[i].max())[0])
        assert res.best_actions[i].cpu().tolist() == digits[:, best[i]].tolist()
    assert ret[0].max() > ret[1].max()  # the root on the vault collects the vault reward
    with pytest.raises(ValueError):
        exhaustive_lookahead(env, roots, depth + 1)  # 3 x 625 workers are not there
    with pytest.raises(ValueError):
        exhaustive_lookahead(env, roots, 1, workers=list(range(2, 17)))  # overlaps root 2
    env.close()
    ctl.close()
