"""heist_plan_q (HeistEnv.plan_q): the exact action values of visited states in one read-only
launch, and the on-policy loop that consumes them (AdversarialTrainer.dagger_solver).  Every
comparison of the kernel's outputs is equality, float64 through its bits (int64).

Yardsticks, none of which uses the kernel under test: heist_amd.search.q_values (the contract in
torch, pinned to the NumPy reference tables and the C oracle by test_plan_q_cpu.py) on the same
device tensors; heist_plan_value's own value_ticks / action_ticks gathered at the same states.
"""
import copy

import numpy as np
import pytest
import torch

import field_ref as fr
from heist_amd import EnvironmentConfig, HeistEnv, PlanQ, _native as nat
from heist_amd.layouts import synthetic_layouts
from heist_amd.obs_compact import record_cells, record_words
from heist_amd.search import q_values

pytestmark = pytest.mark.gpu

HEIST_EINVAL = 100000
MC, MG, MP = 5, 3, 16
GAMMA = 0.99
SEED = 11
HMAX = 48
FIELDS = ("q", "value", "best", "optimal", "gap")
REGRET_TOL = 1e-9  # test_plan_q_cpu's rounding bound


def _cfg(R, C, max_steps):
    return EnvironmentConfig(grid_rows=R, grid_cols=C, max_steps=max_steps, architect_budget=C + 10)


def _make(n, cfg, dev, cones=True):
    env = HeistEnv(n, cfg, max_cams=MC, max_guards=MG, max_path=MP, device=dev, auto_reset=False)
    env.set_guard_cones(cones)
    return env


def _shape_env(name, dev):
    R, C, max_steps, cones = fr.SHAPES[name]
    lays = fr.shape_layouts(R, C, seed=R * 100 + C)
    env = _make(len(lays), _cfg(R, C, max_steps), dev, cones)
    env.set_layouts(lays, budget=C + 10)
    env.reset()
    return env, lays


def _bits(t):
    return t.contiguous().view(torch.int64)


def _tick0(env):
    x = env.export()
    return torch.where(x["done"] != 0, torch.full_like(x["tick"], -1), x["tick"])


def _reference(env, values, vis, pos, taken=None, tick0=None, gamma=GAMMA):
    """search.q_values on the launch's own device tensors and the handle's exported state."""
    c = env.config
    x = env.export(grid=True)
    return q_values(values, vis, x["grid"], _tick0(env) if tick0 is None else tick0, pos, c.max_steps,
                    x["initial_dist"], c.vault_pos, (c.reward_step, c.reward_detection, c.reward_vault), gamma=gamma,
                    taken=taken)


def _assert_same(got, want, what):
    assert isinstance(got, PlanQ)
    for f in FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert (g is None) == (w is None), (what, f)
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, f, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == torch.float64:
            g, w = _bits(g), _bits(w)
        bad = (g != w).nonzero()
        assert not len(bad), "%s: %s differs first at %s" % (what, f, bad[0].tolist())


def _play_states(env, play):
    """pos [H, N, 2] of a play from the envs' own cells: row 0 the cell now, row k record k - 1's."""
    x = env.export()
    start = torch.stack([x["pos_r"], x["pos_c"]], 1).to(torch.int32).unsqueeze(0)
    return torch.cat([start, record_cells(play.records, env.rows, env.cols)[:-1]])


def _shifted(pos, s, R, C):
    """The play's cells pushed off its path: rows and columns shifted by amounts that change with
    the tick and the env, wrapped over -1 .. R and -1 .. C, so cells off the grid, border cells and
    wall cells are hit."""
    K, N = pos.shape[:2]
    k = torch.arange(K, device=pos.device).reshape(K, 1)
    e = torch.arange(N, device=pos.device).reshape(1, N)
    r = (pos[..., 0].long() + 1 + s * k + e) % (R + 2) - 1
    c = (pos[..., 1].long() + 1 + 2 * s + k + 3 * e) % (C + 2) - 1
    return torch.stack([r, c], -1).to(torch.int32)


# ---- 1. the kernel against the contract in torch and against the planner's own tables

@pytest.mark.parametrize("name", sorted(fr.SHAPES))
def test_kernel_equals_q_values(gpu_device, name):
    R, C, max_steps, _ = fr.SHAPES[name]
    env, lays = _shape_env(name, gpu_device)
    n, H = len(lays), min(max_steps, HMAX)
    pv = env.plan_value(horizon=H, gamma=GAMMA, all_ticks=True)
    assert torch.equal(pv.tick, _tick0(env)) and pv.tick.dtype == torch.int32
    play = env.plan_play(pv.action_ticks, pv.vis, values=pv.value_ticks, noise=0.25, seed=SEED)
    pos, taken = _play_states(env, play), play.actions
    walls = pv.grid == 1
    k = torch.arange(H, device=gpu_device).reshape(H, 1).expand(H, n)
    e = torch.arange(n, device=gpu_device).reshape(1, n).expand(H, n)
    dead = off = wall = 0
    for s in range(4):
        cells = pos if s == 0 else _shifted(pos, s, R, C)
        got = env.plan_q(pv, cells, taken)
        _assert_same(got, _reference(env, pv.value_ticks, pv.vis, cells, taken), "%s pattern %d" % (name, s))
        r, c = cells[..., 0].long(), cells[..., 1].long()
        inside = (r >= 0) & (r < R) & (c >= 0) & (c < C)
        rc, cc = r.clamp(0, R - 1), c.clamp(0, C - 1)
        # the planner's own tables at the same states (wall cells hold the fill there too)
        assert torch.equal(_bits(got.value[inside]), _bits(pv.value_ticks[k, e, rc, cc][inside])), (name, s)
        assert torch.equal(got.best[inside], pv.action_ticks[k, e, rc, cc][inside]), (name, s)
        live = got.best >= 0
        assert bool((((got.optimal.long() >> got.best.long().clamp(min=0)) & 1) == 1)[live].all())
        assert torch.equal(got.gap == 0.0, ~live | (((got.optimal.long() >> taken.clamp(0, 4)) & 1) == 1))
        dead += int((~live).sum())
        off += int((~inside).sum())
        wall += int((inside & walls[e, rc, cc]).sum())
        if s:
            border = inside & ((r == 0) | (r == R - 1) | (c == 0) | (c == C - 1))
            assert int(border.sum()) >= 1
    print("%s: %d states not live, %d off the grid, %d on wall cells" % (name, dead, off, wall))
    assert off >= 1 and wall >= 1 and dead >= off + wall
    # the table's own play loses nothing, step by step
    p0 = env.plan_play(pv.action_ticks, pv.vis, values=pv.value_ticks, noise=0.0, seed=SEED)
    g0 = env.plan_q(pv, _play_states(env, p0), p0.actions)
    valid = k < p0.length.reshape(1, n)
    assert not _bits(g0.gap[valid]).any() and bool((g0.best[valid] >= 0).all())
    assert torch.equal(g0.best[valid].long(), p0.actions[valid])
    env.close()


# ---- 2. mid-episode: tick0 labels a rollout after the handle has been stepped through it

@pytest.mark.parametrize("k0", (3, 7))
def test_mid_episode_tick0(gpu_device, k0):
    R, C, H, _ = fr.SHAPES["10x10"]
    env, lays = _shape_env("10x10", gpu_device)
    n = len(lays)
    first = env.plan_value(gamma=GAMMA, all_ticks=True)
    p0 = env.plan_play(first.action_ticks, first.vis, noise=0.25, seed=SEED)
    env.step_multi(p0.actions[:k0], auto_reset=False)  # k0 real ticks
    pv = env.plan_value(horizon=H - k0, gamma=GAMMA, all_ticks=True)
    live = pv.tick >= 0
    assert int(live.sum()) >= 2 and bool((pv.tick[live] == k0).all())
    play = env.plan_play(pv.action_ticks, pv.vis, noise=0.25, seed=SEED)
    pos, taken = _play_states(env, play), play.actions
    before = env.plan_q(pv, pos, taken)
    _assert_same(before, _reference(env, pv.value_ticks, pv.vis, pos, taken), "before the stepping")
    assert bool((before.best[0][live] >= 0).all()) and bool((before.best[:, ~live] == -1).all())
    env.step_multi(play.actions[:5], auto_reset=False)  # the handle moves on
    after = env.plan_q(pv, pos, taken)
    _assert_same(after, before, "with pv.tick after the stepping")
    now = env.plan_q((pv.value_ticks, pv.vis), pos, taken, gamma=GAMMA)  # tick0=None: the handle's tick now
    _assert_same(now, _reference(env, pv.value_ticks, pv.vis, pos, taken), "tick0=None after the stepping")
    # on the start cell at every row, the handle's later tick moves the timeout five rows up and
    # drops the rows after it: the reason the argument exists
    stay = torch.ones((H - k0, n, 2), dtype=torch.int32, device=gpu_device)
    with_tick, without = env.plan_q(pv, stay), env.plan_q((pv.value_ticks, pv.vis), stay, gamma=GAMMA)
    _assert_same(with_tick, _reference(env, pv.value_ticks, pv.vis, stay, tick0=pv.tick), "the start cell, pv.tick")
    row = H - k0 - 6  # the handle's last tick now
    assert not torch.equal(_bits(without.q[row][live]), _bits(with_tick.q[row][live]))
    assert bool((without.best[row + 1:] == -1).all()) and bool((with_tick.best[row + 1:, live] >= 0).all())
    given =env.plan_q((pv.value_ticks, pv.vis), pos, taken, tick0=pv.tick, gamma=GAMMA)
    _assert_same(given, before, "tick0 given for a pair of tables")
    env.close()


# ---- 3. the launch only reads the env

def test_plan_q_reads_only(gpu_device):
    n, R, budget = 64, 20, 15
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=R, max_steps=200)
    env = HeistEnv(n, cfg, max_cams=MC, max_guards=MG, max_path=MP, device=gpu_device, auto_reset=True)
    env.set_layouts(synthetic_layouts(n, R, R, budget, seed=43), budget=budget)
    env.reset()
    env.step_multi(torch.randint(0, 5, (4, n), generator=torch.Generator().manual_seed(5)).to(gpu_device))
    pv = env.plan_value(horizon=HMAX, gamma=GAMMA, all_ticks=True)
    play = env.plan_play(pv.action_ticks, pv.vis, noise=0.25, seed=SEED)
    before = env.save_state().blobs.clone()
    got = env.plan_q(pv, _play_states(env, play), play.actions)
    assert int((got.best >= 0).sum()) > n
    assert torch.equal(env.save_state().blobs, before)
    env.close()


# ---- 4. arguments

def test_arguments(gpu_device, monkeypatch):
    R, C, N, H, K = 13, 17, 3, 6, 5
    env = _make(N, _cfg(R, C, 50), gpu_device)
    env.set_layouts([([], [], [])] * N, budget=10)
    env.reset()
    pv = env.plan_value(horizon=H, gamma=GAMMA, all_ticks=True)
    play = env.plan_play(pv.action_ticks, pv.vis, noise=0.25, seed=SEED)
    pos, taken = _play_states(env, play)[:K].contiguous(), play.actions[:K].contiguous()
    want = env.plan_q(pv, pos, taken)
    _assert_same(want, _reference(env, pv.value_ticks, pv.vis, pos, taken), "13x17, K < horizon")
    kw = dict(device=gpu_device)
    vals, vis, tick0 = pv.value_ticks.contiguous(), pv.vis.contiguous(), pv.tick.contiguous()
    q = torch.empty(K * N * 5 + 1, dtype=torch.float64, **kw)
    value = torch.empty(K * N + 1, dtype=torch.float64, **kw)
    best = torch.empty(K * N, dtype=torch.int8, **kw)
    opt = torch.empty(K * N, dtype=torch.uint8, **kw)
    gap = torch.empty(K * N + 1, dtype=torch.float64, **kw)
    lib, st, P = nat.lib(), env._stream(), nat.ptr
    ins = [P(vals), P(vis), P(tick0), P(pos), P(taken)]
    outs = [P(q), P(value), P(best), P(opt), P(gap)]

    def call(ins=ins, outs=outs, h=H, k=K, gamma=GAMMA, handle=env._h):
        return lib.heist_plan_q(handle, h, k, gamma, *ins, *outs, st)

    def check(which):
        torch.cuda.synchronize(gpu_device)
        got = {"q": q[:K * N * 5], "value": value[:K * N], "best": best, "optimal": opt, "gap": gap[:K * N]}
        for f in which:
            g, w = got[f].reshape(getattr(want, f).shape), getattr(want, f)
            if g.dtype == torch.float64:
                g, w = _bits(g), _bits(w)
            assert torch.equal(g, w), f
    assert call() == 0
    check(FIELDS)
    # each optional output alone
    for i, f in enumerate(FIELDS):
        for t in (q, value, best, opt, gap):
            t.fill_(7)
        o = [None] * 5
        o[i] = outs[i]
        assert call(outs=o) == 0, f
        check([f])
        torch.cuda.synchronize(gpu_device)
        others = {"q": q, "value": value, "best": best, "optimal": opt, "gap": gap}
        assert all(bool((t == 7).all()) for g, t in others.items() if g != f), f
    # without taken: everything but the gap; tick0 NULL is the handle's tick (not stepped since)
    assert call(ins=ins[:4] + [None], outs=outs[:4] + [None]) == 0
    check(FIELDS[:4])
    assert call(ins=ins[:2] + [None] + ins[3:]) == 0
    check(FIELDS)
    out = env.plan_q(pv, pos, outputs=("optimal",))
    assert out.q is None and out.gap is None and torch.equal(out.optimal, want.optimal)
    assert env.plan_q(pv, pos).gap is None
    # HEIST_EINVAL
    for h in (0, 1025, -1):
        assert call(h=h) == HEIST_EINVAL
    for k in (0, H + 1, -1):
        assert call(k=k) == HEIST_EINVAL
    for g in (-0.1, 1.5, float("nan"), float("inf")):
        assert call(gamma=g) == HEIST_EINVAL
    for i in (0, 1, 3):
        bad = list(ins)
        bad[i] = None
        assert call(ins=bad) == HEIST_EINVAL
    assert call(outs=[None] * 5) == HEIST_EINVAL
    assert call(ins=ins[:4] + [None]) == HEIST_EINVAL  # gap_out without taken
    assert vis.data_ptr() % 16 == 0
    odd_vis = torch.cat([vis.reshape(-1), vis.reshape(-1)[:4]])[1:]
    assert call(ins=[ins[0], P(odd_vis)] + ins[2:]) == HEIST_EINVAL
    odd_vals = torch.cat([vals.reshape(-1), vals.reshape(-1)[:1]]).view(torch.int32)[1:]
    assert call(ins=[P(odd_vals)] + ins[1:]) == HEIST_EINVAL
    odd_taken = torch.cat([taken.reshape(-1), taken.reshape(-1)[:1]]).view(torch.int32)[1:]
    assert call(ins=ins[:4] + [P(odd_taken)]) == HEIST_EINVAL
    for i, t in ((0, q), (1, value), (4, gap)):
        o = list(outs)
        o[i] = P(t.view(torch.int32)[1:])
        assert call(outs=o) == HEIST_EINVAL
    for i, t in ((2, tick0), (3, pos)):
        bad = list(ins)
        bad[i] = P(torch.cat([t.reshape(-1), t.reshape(-1)[:1]]).view(torch.int8)[1:])
        assert call(ins=bad) == HEIST_EINVAL
    assert call(handle=None) == HEIST_EINVAL
    # 8-byte alignment is enough for the float64 arrays
    o = list(outs)
    o[0], o[1], o[4] = P(q[1:]), P(value[1:]), P(gap[1:])
    assert call(outs=o) == 0
    torch.cuda.synchronize(gpu_device)
    assert torch.equal(_bits(q[1:]), _bits(want.q.reshape(-1))) and torch.equal(_bits(gap[1:]), _bits(want.gap.reshape(-1)))
    with pytest.raises(ValueError):
        env.plan_q(pv, pos[:, :2], taken[:, :2])
    with pytest.raises(ValueError):
        env.plan_q(pv, pos, outputs=("values",))
    with pytest.raises(ValueError):
        env.plan_q(env.plan_value(horizon=H), pos)
    env.close()
    monkeypatch.setenv("HEIST_PROBE_MODE", "1")
    probe = _make(N, _cfg(R, C, 50), gpu_device)
    assert probe.kernel_config()["probe_mode"] == 1
    assert call(handle=probe._h) == HEIST_EINVAL
    probe.close()


# ---- 5. 64 x 64: served with hand-made tables (plan_value has no kernel there)

def test_64x64_hand_made_tables(gpu_device):
    R = C = 64
    H, N = 40, 3
    walls, rw, g = fr.wallrow(R, C)
    cam = {"row": 3, "col": 6, "fov_angle": 60.0, "vision_range": 6, "heading": 180.0, "rotation_speed": 15.0}
    env = _make(N, _cfg(R, C, 50), gpu_device)
    env.set_layouts([([], [], []), (walls, [cam], []), ([(1, 4), (5, 1)], [cam], [])], budget=C + 10)
    env.reset()
    assert env.plan_value_supported == 0 and env.plan_field_supported == 1
    vis = env.plan_field(horizon=H).vis
    gen = torch.Generator().manual_seed(3)
    values = torch.randn((H, N, R, C), dtype=torch.float64, generator=gen).to(gpu_device)
    pos = torch.stack([torch.randint(-1, R + 1, (H, N), generator=gen), torch.randint(-1, C + 1, (H, N), generator=gen)], -1)
    pos[:, 1, 0] = rw  # the wall row and its gap
    pos[:8, 2] = torch.tensor([2, 5])  # inside the camera's reach
    pos[-1] = torch.tensor([R - 1, C - 1])  # the last cell of the last row
    taken = torch.randint(-1, 6, (H, N), generator=gen)
    pos, taken = pos.to(gpu_device), taken.to(gpu_device)
    got = env.plan_q((values, vis), pos, taken, gamma=GAMMA)
    _assert_same(got, _reference(env, values, vis, pos, taken), "64x64")
    assert int((got.best >= 0).sum()) >= H and int((got.best < 0).sum()) >= 1
    assert bool((got.gap > 0.0).any())
    env.close()


# ---- 6. the trainer's on-policy loop

def test_dagger_solver(gpu_device, tmp_path):
    from heist_amd.training import AdversarialTrainer
    cfg = EnvironmentConfig(grid_rows=10, grid_cols=10, max_steps=40)
    tr = AdversarialTrainer(cfg, solver_episodes_per_layout=1, total_episodes=10 ** 6, save_dir=str(tmp_path / "ck"),
                            log_dir=str(tmp_path / "logs"), n_envs=16, rollout_len=16, device=gpu_device, seed=0,
                            minibatch=256)
    tr.global_episode = 200  # curriculum phase with cameras and guards
    tr._assign_layouts(np.arange(16))
    tr.train_iteration()

    def snapshot():
        names = [k for k in vars(tr) if k.startswith("b_")]
        s = {k: (getattr(tr, k).clone() if torch.is_tensor(getattr(tr, k)) else copy.deepcopy(getattr(tr, k)))
             for k in names if k != "b_layout"}
        s["layout_rows"] = [None if v is None else v[1] for v in tr.b_layout]
        s["global_episode"] = tr.global_episode
        s["game_log"] = [g.to_dict() for g in tr.game_log]
        s["metrics"] = copy.deepcopy(tr.metrics.records())
        s["env"] = tr.env.save_state().blobs.clone()
        s["h"], s["c"] = tr.h.clone(), tr.c.clone()
        a = tr.architect
        s["arch"] = [p.detach().clone() for p in a.network.parameters()]
        s["arch_buf"] = ([t.clone() for t in a.log_probs], [t.clone() for t in a.values], list(a.rewards),
                         a.budget, a.episode_count, a.total_reward)
        return s

    def solver_state():
        opt = tr.solver.optimizer.state_dict()
        return ([p.detach().clone() for p in tr.solver.network.parameters()],
                [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in s.items()} for s in opt["state"].values()],
                copy.deepcopy(opt["param_groups"]))

    def same(u, v):
        if torch.is_tensor(u):
            return torch.is_tensor(v) and torch.equal(u, v)
        if isinstance(u, np.ndarray):
            return bool((u == v).all())
        if isinstance(u, dict):
            return u.keys() == v.keys() and all(same(u[k], v[k]) for k in u)
        if isinstance(u, (list, tuple)):
            return len(u) == len(v) and all(same(a, b) for a, b in zip(u, v))
        return u == v

    before, solver0 = snapshot(), solver_state()
    assert len(solver0[1]) >= 1  # the optimizer has stepped: there is state to leave alone
    keys = {"dagger_optimal_rate", "dagger_gap_mean", "dagger_regret_mean", "dagger_discounted_gap_mean",
            "dagger_decisions", "pretrain_valid_envs"}
    # evaluation: nothing of the Solver changes
    for layouts in ("architect",):
        out = tr.dagger_solver(1, n_envs=64, seed=1, layouts=layouts, update=False)
        assert len(out) == 1
        for m in out:
            print(layouts, m)
            assert set(m) == keys and all(np.isfinite(float(v)) for v in m.values())
            assert m["dagger_decisions"] >= m["pretrain_valid_envs"] >= 1
            assert 0.0 <= m["dagger_optimal_rate"] <= 1.0 and m["dagger_gap_mean"] >= 0.0
            assert abs(m["dagger_regret_mean"] - m["dagger_discounted_gap_mean"]) <= REGRET_TOL
    assert same(solver0, solver_state())
    assert tr._pretrain_env.n_envs == 64 and tr._pretrain_env is not tr.env
    # the table's own action on every step: no decision loses anything
    for m in tr.dagger_solver(1, n_envs=64, beta=1.0, seed=2, update=False):
        assert m["dagger_optimal_rate"] == 1.0 and m["dagger_gap_mean"] == 0.0 and m["dagger_regret_mean"] == 0.0
    assert same(solver0, solver_state())
    # a cut horizon labels the rollout's first ticks
    m = tr.dagger_solver(1, n_envs=64, seed=3, update=False, horizon=12)[0]
    assert m["dagger_decisions"] <= 12 * 64 and abs(m["dagger_regret_mean"] - m["dagger_discounted_gap_mean"]) <= REGRET_TOL
    # training: the imitation step runs on the sets
    out = tr.dagger_solver(1, n_envs=64, beta=0.5, seed=4)
    for m in out:
        print("update", m)
        assert keys < set(m) and all(np.isfinite(float(v)) for v in m.values())
        assert m["imitation_samples"] == m["dagger_decisions"] and m["imitation_updates"] >= 1
        assert 0.0 <= m["imitation_agreement"] <= 1.0
    assert any(not torch.equal(a, b) for a, b in zip(solver0[0], tr.solver.network.parameters()))
    after = snapshot()
    for k in before:
        assert same(before[k], after[k]), k
    with pytest.raises(ValueError):
        tr.dagger_solver(1, n_envs=64, beta=1.5)
    out = tr.train_iteration()
    assert "layouts_scored" in out
    tr._pretrain_env.close()
    tr.env.close()
