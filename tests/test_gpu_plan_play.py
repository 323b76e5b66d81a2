"""heist_plan_play (HeistEnv.plan_play): episodes played from a planner's per-tick tables in one
read-only launch, and the consumers that train from them.  Every comparison of the kernel's
outputs is equality, float64 through its bits (int64).

Yardsticks, none of which uses the kernel under test: heist_amd.search.play_table (the contract in
torch, pinned to the C oracle by test_plan_play_cpu.py) on the same tensors copied to the CPU;
heist_amd.search.follow_value; the env kernels' own records, rewards and statuses of the played
actions (heist_step_multi_records on a twin handle); CPU fp32 torch for the supervised loss.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import field_ref as fr
from heist_amd import EnvironmentConfig, HeistEnv, PlanPlay, _native as nat
from heist_amd.layouts import synthetic_layouts
from heist_amd.obs_compact import record_words
from heist_amd.search import discounted_return, expert_rollout, follow_value, play_table

pytestmark = pytest.mark.gpu

HEIST_EINVAL = 100000
MC, MG, MP = 5, 3, 16
GAMMA = 0.99
SEED = 11
FIELDS = ("actions", "expert", "value", "records", "reward64", "done", "status", "length")


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


def _reference(env, table, vis, values=None, pos=None, **kw):
    """search.play_table on the launch's own inputs and the handle's exported state, on the CPU."""
    c = env.config
    x = {k: v.cpu() for k, v in env.export(grid=True).items()}
    if pos is None:
        pos = torch.stack([x["pos_r"], x["pos_c"]], 1)
    return play_table(table.cpu(), vis.cpu(), x["grid"], x["tick"], torch.as_tensor(pos).cpu(), c.max_steps,
                      x["initial_dist"], c.vault_pos, (c.reward_step, c.reward_detection, c.reward_vault),
                      values=None if values is None else values.cpu(), done=x["done"], **kw)


def _assert_same(got, want, what):
    assert isinstance(got, PlanPlay)
    for f in FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert (g is None) == (w is None), (what, f)
        if g is None:
            continue
        g = g.cpu()
        assert g.shape == w.shape and g.dtype == w.dtype, (what, f, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == torch.float64:
            g, w = g.contiguous().view(torch.int64), w.contiguous().view(torch.int64)
        bad = (g != w).nonzero()
        assert not len(bad), "%s: %s differs first at %s" % (what, f, bad[0].tolist())


def _bits(t):
    return t.contiguous().view(torch.int64)


# ---- 1. the kernel against the contract in torch, and against follow_value

@pytest.mark.parametrize("name", sorted(fr.SHAPES))
def test_kernel_equals_play_table(gpu_device, name):
    env, lays = _shape_env(name, gpu_device)
    n = len(lays)
    pv = env.plan_value(gamma=GAMMA, all_ticks=True)
    off, det = 0, 0
    for noise in (0.0, 0.25, 1.0):
        got = env.plan_play(pv.action_ticks, pv.vis, values=pv.value_ticks, noise=noise, seed=SEED)
        want = _reference(env, pv.action_ticks, pv.vis, pv.value_ticks, noise=noise, seed=SEED)
        _assert_same(got, want, "%s noise %r" % (name, noise))
        assert bool((got.length >= 1).all())
        if noise == 0.0:
            start = torch.ones(n, dtype=torch.int64, device=gpu_device)
            assert torch.equal(got.actions, follow_value(pv, start, start))
            assert torch.equal(got.expert.long()[got.expert >= 0], got.actions[got.expert >= 0])
        else:
            off += int((got.actions != got.expert.long().clamp(min=0)).sum())
            det += int((got.status == 1).sum())
    print("%s: %d noisy steps off the expert's action, %d plays detected" % (name, off, det))
    assert off >= 1
    env.close()


# ---- 2. the played actions through the env kernels

@pytest.mark.parametrize("name", sorted(fr.SHAPES))
def test_replay_through_env(gpu_device, name):
    R, C, max_steps, _ = fr.SHAPES[name]
    for noise in (0.0, 0.25):
        env, lays = _shape_env(name, gpu_device)
        pv = env.plan_value(gamma=GAMMA, all_ticks=True)
        p = env.plan_play(pv.action_ticks, pv.vis, values=pv.value_ticks, noise=noise, seed=SEED)
        twin, _ = _shape_env(name, gpu_device)
        records, _, done, status, r64 = twin.step_multi_records(p.actions, auto_reset=False, reward64=True)
        k = torch.arange(max_steps, device=gpu_device).reshape(-1, 1)
        played = k < p.length.reshape(1, -1)
        assert torch.equal(p.records[played], records[played]), (name, noise)
        # rewards, done and status on every row, the rows after the end included
        assert torch.equal(_bits(p.reward64), _bits(r64)), (name, noise)
        assert torch.equal(p.done, done) and torch.equal(p.status, status), (name, noise)
        if noise == 0.0:
            ret = discounted_return(p.reward64, p.done, GAMMA)
            assert torch.equal(_bits(ret), _bits(pv.value[:, 1, 1])), (ret.tolist(), pv.value[:, 1, 1].tolist())
            assert torch.equal(_bits(p.value[0]), _bits(pv.value[:, 1, 1]))
        env.close()
        twin.close()


# ---- 3. mid-episode: the same seed continues the same draws

def test_mid_episode(gpu_device):
    R, C, H, _ = fr.SHAPES["10x10"]
    env, lays = _shape_env("10x10", gpu_device)
    p0v = env.plan_value(gamma=GAMMA, all_ticks=True)
    p0 = env.plan_play(p0v.action_ticks, p0v.vis, values=p0v.value_ticks, noise=0.25, seed=SEED)
    played = 0
    for k in (3, 7):
        env.step_multi(p0.actions[played:k], auto_reset=False)
        played = k
        x = env.export()
        live = x["done"] == 0
        assert int(live.sum()) >= 2 and bool((p0.length[live] > k).all()) and bool((p0.length[~live] <= k).all())
        pv = env.plan_value(horizon=H - k, gamma=GAMMA, all_ticks=True)
        pk = env.plan_play(pv.action_ticks, pv.vis, values=pv.value_ticks, noise=0.25, seed=SEED)
        ref = _reference(env, pv.action_ticks, pv.vis, pv.value_ticks, noise=0.25, seed=SEED)
        _assert_same(pk, ref, "after %d" % k)
        assert torch.equal(pk.length[live], p0.length[live] - k)
        for f in ("actions", "expert", "records", "done", "status"):
            assert torch.equal(getattr(pk, f)[:, live], getattr(p0, f)[k:, live]), (k, f)
        for f in ("value", "reward64"):
            assert torch.equal(_bits(getattr(pk, f)[:, live]), _bits(getattr(p0, f)[k:, live])), (k, f)
        # another seed draws otherwise
        other = env.plan_play(pv.action_ticks, pv.vis, noise=0.25, seed=SEED + 1)
        assert not torch.equal(other.actions, pk.actions)
        # the envs already done play nothing
        assert bool((pk.length[~live] == 0).all()) and bool((pk.status[:, ~live] == 4).all())
        assert not pk.records[:, ~live].any() and bool((pk.expert[:, ~live] == -1).all())
    env.close()


# ---- 4. the launch only reads the env

def test_plan_play_reads_only(gpu_device, monkeypatch):
    monkeypatch.setenv("HEIST_MULTI_WAVES", "1")
    n, R, budget, K = 64, 20, 15, 20
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=R, max_steps=200)
    lays = synthetic_layouts(n, R, R, budget, seed=43)
    acts = torch.randint(0, 5, (4 + K, n), generator=torch.Generator().manual_seed(5)).to(gpu_device)
    envs = []
    for i in range(2):
        env = HeistEnv(n, cfg, max_cams=MC, max_guards=MG, max_path=MP, device=gpu_device, auto_reset=True)
        env.set_layouts(lays, budget=budget)
        env.reset()
        env.step_multi(acts[:4])
        envs.append(env)
    a, b = envs
    pv = a.plan_value(horizon=50, gamma=GAMMA, all_ticks=True)
    before = a.save_state().blobs.clone()
    p = a.plan_play(pv.action_ticks, pv.vis, values=pv.value_ticks, noise=0.25, seed=SEED)
    assert int(p.length.sum()) > n
    assert torch.equal(a.save_state().blobs, before)
    for u, v in zip(a.step_multi(acts[4:], reward64=True), b.step_multi(acts[4:], reward64=True)):
        assert torch.equal(u, v)
    assert torch.equal(a.save_state().blobs, b.save_state().blobs)
    a.close()
    b.close()


# ---- 5. arguments

def test_arguments(gpu_device):
    R, C, N, H = 13, 17, 3, 6
    env = _make(N, _cfg(R, C, 50), gpu_device)
    env.set_layouts([([], [], [])] * N, budget=10)
    env.reset()
    W, RC = record_words(R, C), R * C
    pv = env.plan_value(horizon=H, gamma=GAMMA, all_ticks=True)
    want = env.plan_play(pv.action_ticks, pv.vis, values=pv.value_ticks, noise=0.25, seed=SEED)
    _assert_same(want, _reference(env, pv.action_ticks, pv.vis, pv.value_ticks, noise=0.25, seed=SEED), "13x17")
    kw = dict(device=gpu_device)
    table, vis, vals = pv.action_ticks.contiguous(), pv.vis.contiguous(), pv.value_ticks.contiguous()
    acts = torch.empty(H * N + 1, dtype=torch.int64, **kw)
    expert = torch.empty(H * N, dtype=torch.int8, **kw)
    value = torch.empty(H * N + 1, dtype=torch.float64, **kw)
    rec = torch.empty(H * N * W + 4, dtype=torch.int32, **kw)
    r64 = torch.empty(H * N + 1, dtype=torch.float64, **kw)
    done = torch.empty(H * N, dtype=torch.uint8, **kw)
    status = torch.empty(H * N, dtype=torch.int8, **kw)
    length = torch.empty(N, dtype=torch.int32, **kw)
    lib, st, P = nat.lib(), env._stream(), nat.ptr
    q = int(round(0.25 * 2 ** 24))
    ins = [P(table), P(vis), P(vals), None]
    outs = [P(acts), P(expert), P(value), P(rec), P(r64), P(done), P(status), P(length)]

    def call(ins=ins, outs=outs, h=H, noise=q):
        return lib.heist_plan_play(env._h, h, *ins, noise, SEED, *outs, st)

    def check(which):
        torch.cuda.synchronize(gpu_device)
        got = {"actions": acts[:H * N], "expert": expert, "value": value[:H * N], "records": rec[:H * N * W],
               "reward64": r64[:H * N], "done": done.view(torch.bool), "status": status, "length": length}
        for f in which:
            g, w = got[f].reshape(getattr(want, f).shape), getattr(want, f)
            if g.dtype == torch.float64:
                g, w = _bits(g), _bits(w)
            assert torch.equal(g, w), f
    assert call() == 0
    check(FIELDS)
    # every optional argument alone left out
    for i, f in ((1, "expert"), (2, "value"), (3, "records"), (4, "reward64"), (7, "length")):
        for t in (acts, expert, value, rec, r64, done, status, length):
            t.zero_()
        o = list(outs)
        o[i] = None
        assert call(outs=o) == 0, f
        check([g for g in FIELDS if g != f])
    o = list(outs)
    o[2] = None
    assert call(ins=[ins[0], ins[1], None, None], outs=o) == 0  # no value table, no value output
    check([g for g in FIELDS if g != "value"])
    assert call(ins=[ins[0], ins[1], None, None]) == HEIST_EINVAL  # value_out without value_table
    for h in (0, 1025, -1):
        assert call(h=h) == HEIST_EINVAL
    assert call(noise=2 ** 24 + 1) == HEIST_EINVAL
    for i in (0, 1):
        bad = list(ins)
        bad[i] = None
        assert call(ins=bad) == HEIST_EINVAL
    for i in (0, 5, 6):
        bad = list(outs)
        bad[i] = None
        assert call(outs=bad) == HEIST_EINVAL
    assert vis.data_ptr() % 16 == 0 and rec.data_ptr() % 16 == 0
    assert call(ins=[ins[0], P(torch.cat([vis.reshape(-1), vis.reshape(-1)[:4]])[1:]), ins[2], None]) == HEIST_EINVAL
    o = list(outs)
    o[3] = P(rec[1:])
    assert call(outs=o) == HEIST_EINVAL
    for i, t in ((2, value), (4, r64)):
        o = list(outs)
        o[i] = P(t.view(torch.int32)[1:])
        assert call(outs=o) == HEIST_EINVAL
    odd = torch.cat([vals.reshape(-1), vals.reshape(-1)[:1]]).view(torch.int32)[1:]
    assert call(ins=[ins[0], ins[1], P(odd), None]) == HEIST_EINVAL
    assert lib.heist_plan_play(None, H, *ins, q, SEED, *outs, st) == HEIST_EINVAL
    # 8-byte alignment is enough for the float64 arrays, 16 for the records
    o = list(outs)
    o[2], o[4], o[3] = P(value[1:]), P(r64[1:]), P(rec[4:])
    assert call(outs=o) == 0
    torch.cuda.synchronize(gpu_device)
    assert torch.equal(_bits(value[1:]), _bits(want.value.reshape(-1)))
    assert torch.equal(rec[4:], want.records.reshape(-1))
    # start cells: an override, and cells outside the grid, found on the device
    pos = torch.tensor([[5, 5], [R, 0], [0, -1]], dtype=torch.int32)
    got = env.plan_play(pv.action_ticks, pv.vis, values=pv.value_ticks, pos=pos, noise=0.25, seed=SEED)
    _assert_same(got, _reference(env, pv.action_ticks, pv.vis, pv.value_ticks, pos=pos, noise=0.25, seed=SEED), "pos0")
    assert got.length.tolist()[1:] == [-1, -1] and int(got.length[0]) >= 1
    assert int(got.expert[0, 0]) == int(pv.action_ticks[0, 0, 5, 5])
    assert bool((got.status[:, 1:] == 4).all()) and not got.records[:, 1:].any() and bool(got.done[:, 1:].all())
    with pytest.raises(nat.HeistError):
        env.plan_play(pv.action_ticks[:0], pv.vis[:0])
    with pytest.raises(ValueError):
        env.plan_play(pv.action_ticks, pv.vis, noise=1.5)
    with pytest.raises(ValueError):
        env.plan_play(pv.action_ticks[:, :2], pv.vis)
    env.close()


# ---- 6. 64 x 64: served with a hand-made table (plan_value has no kernel there)

def test_64x64_hand_made_table(gpu_device):
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
    table = torch.randint(-1, 6, (H, N, R, C), generator=gen).to(torch.int8)
    table[:, :, :8, :8] = torch.where(torch.rand((H, N, 8, 8), generator=gen) < 0.5, 4, 2).to(torch.int8)
    values = torch.randn((H, N, R, C), dtype=torch.float64, generator=gen)
    pos = torch.tensor([[1, 1], [62, 60], [40, 63]], dtype=torch.int32)
    for noise, p0 in ((0.0, None), (0.25, None), (0.25, pos)):
        got = env.plan_play(table.to(gpu_device), vis, values=values.to(gpu_device), pos=p0, noise=noise, seed=SEED)
        _assert_same(got, _reference(env, table, vis, values, pos=p0, noise=noise, seed=SEED), "64x64 %r" % noise)
    assert int(got.length.max()) >= 2
    env.close()


# ---- 7. the supervised step on the fp32 MFMA backbone

def test_imitation_update_mfma(gpu_device):
    from heist_amd.agents.solver import SolverAgent
    torch.manual_seed(0)
    R, n = 20, 256
    env = _make(32, _cfg(R, R, 60), gpu_device)
    valid = env.set_layouts(synthetic_layouts(32, R, R, 15, seed=9), budget=15).bool()
    env.reset()
    data = expert_rollout(env, gamma=GAMMA, noise=0.25, seed=SEED)
    obs, expert, value, taken = data.flat(valid)
    assert len(obs) >= n and int(data.valid.sum()) == int(data.length.clamp(min=0).sum())
    idx = torch.arange(n, device=gpu_device)
    obs, expert, value = obs[idx], expert[:n], value[:n]
    assert bool((expert >= 0).all()) and len(set(expert.tolist())) >= 3
    agent = SolverAgent(grid_rows=R, grid_cols=R, device=gpu_device)
    x = obs.expand()
    assert agent.network._train_conv_ok(x), "the fp32 MFMA training backbone must serve this shape"
    twin = copy.deepcopy(agent.network).cpu().to(memory_format=torch.contiguous_format)
    twin.train()
    with torch.no_grad():
        logits, v, _ = twin(x.cpu().contiguous())
        ce = float(F.cross_entropy(logits.float(), expert.cpu()))
        mse = float(F.mse_loss(v.reshape(-1).float(), value.cpu()))
    m = agent.imitation_update(obs, expert, value, minibatch=n)
    print("imitation_ce %r (CPU fp32 %r), value loss %r (CPU %r)"
          % (m["imitation_ce"], ce, m["imitation_value_loss"], mse))
    assert m["imitation_updates"] == 1 and m["imitation_samples"] == n
    assert abs(m["imitation_ce"] - ce) < 1e-4
    env.close()


# ---- 8. the trainer's pre-training leaves the trainer's own state alone

def test_pretrain_solver(gpu_device, tmp_path):
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

    def same(u, v):
        if torch.is_tensor(u):
            return torch.equal(u, v)
        if isinstance(u, np.ndarray):
            return bool((u == v).all())
        if isinstance(u, (list, tuple)):
            return len(u) == len(v) and all(same(a, b) for a, b in zip(u, v))
        return u == v

    before = snapshot()
    assert len([k for k in before if k.startswith("b_")]) >= 10
    solver0 = [p.detach().clone() for p in tr.solver.network.parameters()]
    for layouts in ("architect", "empty"):
        out = tr.pretrain_solver(2, n_envs=32, noise=0.1, seed=1, layouts=layouts)
        assert len(out) == 2
        for m in out:
            print(layouts, m)
            assert all(np.isfinite(float(v)) for v in m.values())
            assert m["imitation_samples"] >= 1 and m["imitation_updates"] >= 1
            assert 0.0 <= m["imitation_agreement"] <= 1.0
    assert tr._pretrain_env.n_envs == 32 and tr._pretrain_env is not tr.env
    assert any(not torch.equal(a, b) for a, b in zip(solver0, tr.solver.network.parameters()))
    after = snapshot()
    for k in before:
        assert same(before[k], after[k]), k
    out = tr.train_iteration()
    assert "layouts_scored" in out
    tr._pretrain_env.close()
    tr.env.close()
