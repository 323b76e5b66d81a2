"""heist_plan (HeistEnv.plan): the fewest undetected ticks to the vault, the canonical plan and
the per-tick reach sets of every env, in one launch.

Yardsticks, none of which uses the planner: the 10 x 10 table of plan_ref.py (measured with the C
oracle); a search by forks on the env kernels themselves (fork_search: save_state, load_state x 5,
one heist_step with the five actions, export, one saved state per distinct live cell); replays of
the returned actions through heist_step_multi and the C oracle.  Every heist_create-able handle
has a planner kernel (heist_create falls back to waves for which the K-tick instance exists), so
the HEIST_EINVAL of an unsupported handle cannot be provoked from here; heist_plan_supported is
checked to be 1 on every shape and -1 on a bad handle (test_plan_ref_cpu.py).
"""
import numpy as np
import pytest
import torch

import plan_ref as pr
from heist_amd import EnvironmentConfig, HeistEnv, _native as nat
from heist_amd.layouts import synthetic_layout, synthetic_layouts
from heist_amd.obs_compact import record_words
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

HEIST_EINVAL = 100000
MC, MG, MP = 5, 3, 16


def _cfg(R, C, max_steps, start=(1, 1)):
    return EnvironmentConfig(grid_rows=R, grid_cols=C, max_steps=max_steps, start_pos=start, architect_budget=C + 10)


def _make(n, cfg, dev, cones=True):
    env = HeistEnv(n, cfg, max_cams=MC, max_guards=MG, max_path=MP, device=dev, auto_reset=False)
    env.set_guard_cones(cones)
    return env


def _make_scratch(cfg, dev, cones=True):
    """The fork search's handle: 5 R C envs (every cell of one planned env x the five actions),
    laid out empty so that the envs a tick does not load are ordinary ones."""
    n = 5 * cfg.grid_rows * cfg.grid_cols
    env = _make(n, cfg, dev, cones)
    env.set_layouts([([], [], [])] * n, budget=0)
    env.reset()
    return env


# ---- the yardstick: search by forks on the env kernels

def fork_search(env, scratch, e, horizon=None):
    """(T, reach) of env e of `env` as it stands, reach[k - 1] the bool [R, C] device mask of the
    distinct cells with done == 0 after k ticks (the list ends at the first clean vault arrival,
    when no cell is left, or at the horizon)."""
    R, C, dev = env.rows, env.cols, env.device
    x = env.export()
    tick0, done0 = int(x["tick"][e]), int(x["done"][e])
    H = env.config.max_steps if horizon is None else horizon
    H = min(H, env.config.max_steps - tick0)
    parents = env.save_state([e])
    F = 0 if done0 else 1
    five = torch.arange(5, device=dev)
    reach, T = [], -1
    for k in range(1, H + 1):
        if F == 0:
            break
        assert 5 * F <= scratch.n_envs
        ok = scratch.load_state(parents, index=torch.arange(F, device=dev).repeat_interleave(5))
        acts = torch.zeros(scratch.n_envs, dtype=torch.int64, device=dev)
        acts[:5 * F] = five.repeat(F)
        scratch.step(acts, auto_reset=False)
        y = scratch.export()
        done, det, vault = (y[key][:5 * F] for key in ("done", "detected", "vault_reached"))
        assert bool(ok.all()) and bool((y["tick"][:5 * F] == tick0 + k).all())
        if bool(((vault == 1) & (det == 0)).any()):
            T = k
            break
        live = done == 0
        cell = (y["pos_r"][:5 * F] * C + y["pos_c"][:5 * F]).long()
        first = torch.full((R * C,), 5 * F, dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, cell[live], torch.arange(5 * F, device=dev)[live], "amin")
        reach.append((first < 5 * F).reshape(R, C))
        reps = first[first < 5 * F]
        F = int(reps.numel())
        if F:
            parents = scratch.save_state(reps)
    return T, reach


def _check_against_forks(env, scratch, res, horizon=None, envs=None):
    """Every tick's reach set, the tick count and the canonical plan of res against fork_search;
    returns {env: T} from the yardstick."""
    H, N = res.actions.shape
    R, C = env.rows, env.cols
    masks = torch.stack([res.reach_mask(k) for k in range(1, H + 1)])  # [H, N, R, C]
    ticks, actions = res.ticks.cpu().numpy(), res.actions.cpu().numpy()
    x = env.export()
    pos = torch.stack([x["pos_r"], x["pos_c"], x["done"]], 1).cpu().numpy()
    words = res.reach.cpu().numpy().view(np.uint32)
    nvis = (R * C + 31) // 32
    assert not words[:, :, nvis:].any(), "words past ceil(RC/32) must be 0"
    if R * C % 32:
        assert not (words[:, :, nvis - 1] >> (R * C % 32)).any(), "bits past RC must be 0"
    out = {}
    for e in (range(N) if envs is None else envs):
        T, reach = fork_search(env, scratch, e, horizon)
        out[e] = T
        print("env %d: yardstick T = %d, planner T = %d, %d reach rows" % (e, T, ticks[e], len(reach)))
        want = torch.zeros((H, R, C), dtype=torch.bool, device=env.device)
        if reach:
            want[:len(reach)] = torch.stack(reach)[:H]
        diff = (masks[:, e] != want).flatten(1).any(1).nonzero()
        assert diff.numel() == 0, "env %d: reach set differs first at tick %d" % (e, int(diff[0]) + 1)
        assert ticks[e] == T, "env %d" % e
        r0 = np.zeros((R, C), bool)
        if not pos[e, 2]:
            r0[pos[e, 0], pos[e, 1]] = True
        plan = pr.backtrack([r0] + [m.cpu().numpy() for m in reach], T, env.config.vault_pos)
        np.testing.assert_array_equal(actions[:, e], plan + [0] * (H - len(plan)), "env %d" % e)
    return out


# ---- 1. the 10 x 10 fixtures

def _table_env(dev):
    """The seven cases of plan_ref.CASES in one handle.  The handle's start is (1, 1); the env of
    start_on_vault gets its solver's cell by a saved state whose scalars name the vault."""
    cfg = _cfg(pr.GRID, pr.GRID, pr.MAX_STEPS)
    names = list(pr.CASES)
    env = _make(len(names), cfg, dev)
    valid = env.set_layouts([pr.CASES[n][0] for n in names], budget=pr.BUDGET).cpu().numpy()
    env.reset()
    i = names.index("start_on_vault")
    st = env.save_state([i])
    scal = st.blobs[0, 64:72].view(torch.int32)  # EnvScalars follow the 64-byte header: pos_r, pos_c
    scal[0], scal[1] = pr.VAULT
    assert bool(env.load_state(st, env_ids=[i]).all())
    return env, names, valid


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_fixture_table(gpu_device, monkeypatch, waves):
    monkeypatch.setenv("HEIST_MULTI_WAVES", str(waves))
    env, names, valid = _table_env(gpu_device)
    assert env.kernel_config()["multi_waves"] == waves and env.plan_supported == 1
    assert [bool(v) for v in valid] == [n != "full_wallrow" for n in names]
    res = env.plan()
    H = pr.MAX_STEPS
    assert res.actions.shape == (H, len(names)) and res.actions.dtype == torch.int64
    assert res.reach.shape == (H, len(names), record_words(pr.GRID, pr.GRID)) and res.ticks.dtype == torch.int32
    ticks, actions = res.ticks.cpu().numpy(), res.actions.cpu().numpy()
    sizes = torch.stack([res.reach_mask(k).flatten(1).sum(1) for k in range(1, H + 1)]).cpu().numpy()  # [H, N]
    for i, n in enumerate(names):
        _, _, T, plan = pr.CASES[n]
        assert ticks[i] == T, n
        assert list(actions[:, i]) == plan + [0] * (H - len(plan)), n
    b = names.index("wallrow_both")
    assert list(sizes[:, b]) == pr.BOTH_SIZES[1:] + [0] * (H - len(pr.BOTH_SIZES) + 1)
    f = names.index("wallrow_fixed_cam")
    assert list(sizes[8:, f]) == [9] * (H - 9) + [0]
    env.close()


# ---- 2. against the env itself

def _wallrow(R, C):
    rw, g = R // 2 - 1, C // 2
    return [(rw, c) for c in range(1, C - 1) if c != g], rw, g


def shape_layouts(R, C, seed):
    """Layouts with a wall row and its one gap watched by a turning camera (a wait: T above the
    Manhattan distance), by a camera that never turns (BFS-valid, never clean), by a guard whose
    range of 8 keeps it off the cone cache (raycast live every tick), plus empty and random ones
    (the last a C2-style 5 cameras + 3 guards)."""
    walls, rw, g = _wallrow(R, C)

    def cam(h, s):
        return {"row": rw + 2, "col": g, "fov_angle": 60.0, "vision_range": 6, "heading": float(h),
                "rotation_speed": float(s)}

    lo, hi = max(1, g - 3), min(C - 2, g + 3)
    guard = {"patrol_path": [(rw + 1, c) for c in range(lo, hi + 1)], "speed": 1, "vision_range": 8, "fov_angle": 90.0}
    rng = np.random.Generator(np.random.PCG64(seed))
    return [([], [], []), (walls, [cam(270, 30)], []), (walls, [cam(90, 0)], []), (walls, [], [guard]),
            (walls, [cam(270, 30)], [dict(guard, vision_range=4)]),
            synthetic_layout(rng, R, C, C + 10, n_cams=2, n_guards=1),
            synthetic_layout(rng, R, C, 30, n_cams=5, n_guards=3)]


SHAPES = {"10x10": (10, 10, 40, True), "10x10_live_guards": (10, 10, 40, False), "13x17": (13, 17, 50, True),
          "20x20": (20, 20, 60, True), "32x32": (32, 32, 80, True)}


def _shape_envs(name, dev):
    R, C, max_steps, cones = SHAPES[name]
    cfg = _cfg(R, C, max_steps)
    lays = shape_layouts(R, C, seed=R * 100 + C)
    env, scratch = _make(len(lays), cfg, dev, cones), _make_scratch(cfg, dev, cones)
    valid = env.set_layouts(lays, budget=C + 10).cpu().numpy()
    env.reset()
    return env, scratch, lays, valid


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_reach_sets_equal_fork_search(gpu_device, name):
    env, scratch, lays, valid = _shape_envs(name, gpu_device)
    R, C, max_steps, cones = SHAPES[name]
    assert env.plan_supported == 1
    res = env.plan()
    T = _check_against_forks(env, scratch, res)
    manhattan = abs(env.config.vault_pos[0] - 1) + abs(env.config.vault_pos[1] - 1)
    # what the planned envs must contain, found by the yardstick
    assert any(t > manhattan for t in T.values()), T
    assert any(valid[e] and t == -1 for e, t in T.items()), (T, valid)
    x = env.export()
    assert int(x["n_guards"].max()) >= 1 and any(g["vision_range"] > 7 for lay in lays for g in lay[2])
    assert env.kernel_config()["guard_cones"] == (1 if cones else 0)
    env.close()
    scratch.close()


# ---- 3. mid-episode state, done envs, horizons

def test_mid_episode_and_horizons(gpu_device):
    R = C = pr.GRID
    cfg = _cfg(R, C, pr.MAX_STEPS)
    lays = shape_layouts(R, C, seed=7)
    # a camera that never turns and looks along row 1 at the start cell: detected on tick 1
    lays.append(([], [{"row": 1, "col": 4, "fov_angle": 60.0, "vision_range": 6, "heading": 180.0,
                       "rotation_speed": 0.0}], []))
    env, scratch = _make(len(lays), cfg, gpu_device), _make_scratch(cfg, gpu_device)
    env.set_layouts(lays, budget=C + 10)
    env.reset()
    for a in (4, 4, 0, 0, 0, 0, 0):  # to (1, 3), out of the gap's sight; cameras have turned, guards are mid-patrol
        env.step(torch.full((len(lays),), a, dtype=torch.int64), auto_reset=False)
    x = env.export()
    done = x["done"].cpu().numpy()
    print("done after 7 ticks:", done, "ticks:", x["tick"].cpu().numpy())
    assert done[-1] == 1 and not done[0] and int(x["tick"][0]) == 7
    state0 = env.save_state()
    res = env.plan()  # horizon max_steps: clipped to max_steps - tick for the live envs
    H = pr.MAX_STEPS
    T = _check_against_forks(env, scratch, res)
    assert torch.equal(env.save_state().blobs, state0.blobs)
    for e in np.nonzero(done)[0]:  # an env already done: -1, no actions, no cells
        assert T[int(e)] == -1 and int(res.ticks[e]) == -1
        assert not res.actions[:, e].any() and not res.reach[:, e].any()
    assert not res.reach[H - 7:].any(), "rows past max_steps - tick"
    never = [e for e, t in T.items() if t == -1 and not done[e]]
    assert never and all(bool(res.reach[H - 7 - 2, e].any()) for e in never[:1])  # alive up to the timeout
    # a horizon one short of T gives -1 and the same sets up to it
    e, t = max(T.items(), key=lambda kv: kv[1])
    assert t > 2
    short = env.plan(horizon=t - 1)
    assert int(short.ticks[e]) == -1 and not short.actions[:, e].any()
    assert torch.equal(short.reach[:, e], res.reach[:t - 1, e])
    _check_against_forks(env, scratch, short, horizon=t - 1, envs=[e, 0])
    env.close()
    scratch.close()


# ---- 4. replay

def test_replay_through_step_multi_and_oracle(gpu_device):
    n, R, max_steps, budget = 64, 20, 200, 15
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=R, max_steps=max_steps)
    lays = synthetic_layouts(n, R, R, budget, seed=41)
    env = _make(n, cfg, gpu_device)
    valid = env.set_layouts(lays, budget=budget).cpu().numpy()
    env.reset()
    res = env.plan()
    ticks, actions = res.ticks.cpu().numpy(), res.actions.cpu().numpy()
    assert (ticks > 0).sum() >= 16 and not (ticks[~valid] > 0).any()
    _, _, done, status, _ = env.step_multi(res.actions, auto_reset=False)
    x = {k: v.cpu().numpy() for k, v in env.export().items()}
    done = done.cpu().numpy()
    clean = (x["vault_reached"] == 1) & (x["detected"] == 0)
    for e in range(n):
        if ticks[e] > 0:
            assert clean[e] and x["tick"][e] == ticks[e], e
            assert int(np.argmax(done[:, e])) == ticks[e] - 1 and done[ticks[e] - 1, e], e
        else:
            assert ticks[e] == -1 and not clean[e], e
    for e in range(32):
        o = po.OracleEnv(R, R, max_steps, (1, 1), (R - 2, R - 2), budget)
        assert o.set_layout(*lays[e]) == bool(valid[e])
        o.reset()
        first = -1
        for k in range(max_steps):
            _, d, _ = o.step(int(actions[k, e]))
            if d and first < 0:
                first = k
        i = o.info()
        if ticks[e] > 0:
            assert (i["vault_reached"], i["detected"], i["tick"], first) == (1, 0, ticks[e], ticks[e] - 1), e
        else:
            assert not (i["vault_reached"] and not i["detected"]), e
    env.close()


# ---- 5. the launch only reads the env

def test_plan_reads_only(gpu_device, monkeypatch):
    """4,096 lean-served 20 x 20 envs with the shared fan table in use: the saved state is equal
    before and after plan(), and the next heist_step_multi launch is bit-identical to a twin's
    that never planned."""
    monkeypatch.setenv("HEIST_MULTI_WAVES", "1")
    n, R, budget, K = 4096, 20, 15, 4
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=R, max_steps=200)
    lays = synthetic_layouts(64, R, R, budget, seed=43) * (n // 64)
    gen = torch.Generator().manual_seed(5)
    acts = torch.randint(0, 5, (2 * K, n), generator=gen).to(gpu_device)
    envs = []
    for i in range(2):
        env = HeistEnv(n, cfg, max_cams=MC, max_guards=MG, max_path=MP, device=gpu_device, auto_reset=True)
        kc = env.kernel_config()
        assert kc["lean"] == 1 and kc["multi_waves"] == 1 and kc["fan_on"] == 1, kc
        env.set_layouts(lays, budget=budget)
        env.reset()
        env.step_multi(acts[:K])  # fills the fan table and leaves its position mid-table
        envs.append(env)
    a, b = envs
    before = a.save_state().blobs.clone()
    res = a.plan(horizon=50)
    assert int((res.ticks > 0).sum()) > 0
    assert torch.equal(a.save_state().blobs, before)
    out_a = a.step_multi(acts[K:], reward64=True)
    out_b = b.step_multi(acts[K:], reward64=True)
    for u, v in zip(out_a, out_b):
        assert torch.equal(u, v)
    assert torch.equal(a.save_state().blobs, b.save_state().blobs)
    a.close()
    b.close()


# ---- 6. arguments

def _einval(fn):
    with pytest.raises(nat.HeistError) as ei:
        fn()
    assert "code %d" % HEIST_EINVAL in str(ei.value)


def test_arguments(gpu_device, monkeypatch):
    cfg = _cfg(13, 17, 50)
    env = _make(3, cfg, gpu_device)
    env.set_layouts([([], [], [])] * 3, budget=10)
    env.reset()
    assert env.plan_supported == 1
    assert env.plan(horizon=1024).actions.shape == (1024, 3)
    _einval(lambda: env.plan(horizon=0))
    _einval(lambda: env.plan(horizon=1025))
    H, W = 4, record_words(13, 17)
    kw = dict(device=gpu_device)
    ticks = torch.empty(3, dtype=torch.int32, **kw)
    actions = torch.empty((H, 3), dtype=torch.int64, **kw)
    reach = torch.empty(H * 3 * W + 4, dtype=torch.int32, **kw)
    lib, st = nat.lib(), env._stream()
    good = [nat.ptr(ticks), nat.ptr(actions), nat.ptr(reach)]
    assert lib.heist_plan(env._h, H, *good, st) == 0
    for i in range(3):
        args = list(good)
        args[i] = None
        assert lib.heist_plan(env._h, H, *args, st) == HEIST_EINVAL
    assert reach.data_ptr() % 16 == 0
    assert lib.heist_plan(env._h, H, good[0], good[1], nat.ptr(reach[1:]), st) == HEIST_EINVAL
    assert lib.heist_plan(None, H, *good, st) == HEIST_EINVAL and lib.heist_plan_supported(None) == -1
    torch.cuda.synchronize(gpu_device)
    env.close()
    monkeypatch.setenv("HEIST_PROBE_MODE", "1")
    probe = _make(3, _cfg(20, 20, 60), gpu_device)
    assert probe.kernel_config()["probe_mode"] == 1
    _einval(lambda: probe.plan())
    probe.close()


# ---- 7. trainer

def test_trainer_track_optimal(gpu_device, tmp_path):
    from heist_amd.training import AdversarialTrainer
    outs = {}
    for track in (False, True):
        cfg = EnvironmentConfig(grid_rows=20, grid_cols=20, max_steps=200)
        d = tmp_path / str(track)
        tr = AdversarialTrainer(cfg, solver_episodes_per_layout=1, total_episodes=10 ** 6, save_dir=str(d / "ck"),
                                log_dir=str(d / "logs"), n_envs=16, rollout_len=16, device=gpu_device, seed=0,
                                minibatch=256, track_optimal=track)
        tr.global_episode = 200  # curriculum phase with cameras and guards
        tr._assign_layouts(np.arange(16))
        outs[track] = tr.train_iteration()
        tr.env.close()
    assert set(outs[True]) == set(outs[False]) | {"solvable_frac", "optimal_ticks_mean"}
    assert "solvable_frac" not in outs[False]
    assert 0.0 <= outs[True]["solvable_frac"] <= 1.0
    if outs[True]["solvable_frac"] > 0:
        assert 34 <= outs[True]["optimal_ticks_mean"] <= 200  # the Manhattan distance .. max_steps
