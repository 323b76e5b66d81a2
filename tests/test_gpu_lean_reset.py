"""Auto-reset inside the lean K-tick kernel (step_lean_kernel): a finishing env whose guards
stand off their patrol start keeps the cameras' share of the tick's visibility and restamps
the guards' cones alone, from cone entries staged a tick ahead.  Every case runs 64 envs for
at most 60 ticks and compares heist_step_multi on the lean kernel, bit for bit, with one
heist_step per tick on the single-tick step kernel (HEIST_STEP_LEAN=0), with the C oracle for
16 envs (every tick's observation bytes, float64 reward, done, status) and with the exported
end state.

A case must meet the situation it names: a CPU replay through the oracle (all valid envs)
counts the env-ticks that end an episode with a guard off its patrol start
  * at the first tick of a launch, * at the last tick of a launch, * on two consecutive ticks
    of one env, * in an env with at least 4 cameras,
and each count must be at least 1 with auto-reset on.  The 4-camera count is asked where the
budget allows 4 cameras beside a guard (3 x 4 + 5 = 17 <= budget: components/budget.py); at
budget 15 an env with 4 cameras has no guard, so no reset of it can find a guard off its start.
With auto-reset off no env resets; those cases must instead freeze an env before the last
launch (the frozen env keeps both planes).  The counts need no GPU: _plan() is the replay.
"""
import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from heist_amd import EnvironmentConfig
from heist_amd.layouts import architect_patrol, synthetic_layouts
from test_gpu_env import _interval_fan_layouts, _shared_camera_layouts, _twin_envs

pytestmark = pytest.mark.gpu

LAUNCHES = (1, 2, 20, 7)
N_ENVS = 64
N_ORACLE = 16


def _f32(x):
    return float(np.float32(x))


def _actions(n, ticks, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, 5, (ticks, n), generator=g)


def _plan(cfg, lays, budget, acts, launches, auto_reset):
    """The oracle's replay of every env: (valid mask, picked envs, their expected rows per tick,
    the situation counts).  A row is (observation bytes, float64 reward, done, status)."""
    n, ticks = len(lays), sum(launches)
    acts = acts.numpy()
    oracles, valid = [], np.zeros(n, bool)
    for i, lay in enumerate(lays):
        o = po.OracleEnv(cfg.grid_rows, cfg.grid_cols, cfg.max_steps, cfg.start_pos, cfg.vault_pos, budget)
        valid[i] = o.set_layout(*lay)
        o.reset()
        oracles.append(o)
    pick = np.nonzero(valid)[0][:N_ORACLE]
    assert len(pick) == N_ORACLE
    picked = set(int(i) for i in pick)
    # guards the oracle accepted as listed: their patrol index names a point of the listed path
    tracked = [valid[i] and oracles[i].info()["n_guards"] == len(lays[i][2]) for i in range(n)]
    cams4 = [oracles[i].info()["n_cams"] >= 4 for i in range(n)]
    ends = np.zeros((ticks, n), bool)  # env-ticks that end an episode with a guard off its patrol start
    frozen_at = np.full(n, ticks, np.int64)
    rows = {int(i): [] for i in pick}
    for t in range(ticks):
        for i, o in enumerate(oracles):
            if not valid[i]:
                continue
            r, d, s = o.step(int(acts[t, i]))
            if d and tracked[i] and frozen_at[i] == ticks:
                _, gi, _ = o.headings()
                paths = [g["patrol_path"] for g in lays[i][2]]
                ends[t, i] = any(tuple(p[int(j)]) != tuple(p[0]) for p, j in zip(paths, gi))
            if d and auto_reset:
                o.reset()
            elif d:
                frozen_at[i] = min(frozen_at[i], t)
            if i in picked:
                rows[i].append((o.state_tensor().tobytes(), r, d, s))
    firsts = np.cumsum((0,) + tuple(launches[:-1]))
    lasts = np.cumsum(launches) - 1
    counts = {"first_tick": int(ends[firsts].sum()), "last_tick": int(ends[lasts].sum()),
              "consecutive": int((ends[1:] & ends[:-1]).sum()),
              "four_cameras": int(ends[:, np.nonzero(cams4)[0]].sum()),
              "frozen_before_last_launch": int((frozen_at < firsts[-1]).sum())}
    return valid, pick, rows, counts


def _check_counts(counts, budget, auto_reset):
    if auto_reset:
        need = ["first_tick", "last_tick", "consecutive"] + (["four_cameras"] if budget >= 17 else [])
    else:
        need = ["frozen_before_last_launch"]
    for key in need:
        assert counts[key] >= 1, (key, counts)


def _run(gpu_device, monkeypatch, cfg, lays, budget, max_cams, max_guards, seed, auto_reset=True, lean_waves=None,
         launches=LAUNCHES):
    n = len(lays)
    acts = _actions(n, sum(launches), seed)
    valid, pick, rows, counts = _plan(cfg, lays, budget, acts, launches, auto_reset)
    print("situation counts:", counts)
    _check_counts(counts, budget, auto_reset)
    monkeypatch.setenv("HEIST_MULTI_WAVES", "1")  # one wave per env at this small batch, as at the bench's 4,096
    if lean_waves is not None:
        monkeypatch.setenv("HEIST_LEAN_WAVES", str(lean_waves))
    a, b = _twin_envs(n, cfg, lays, budget, gpu_device, max_cams=max_cams, max_guards=max_guards, max_path=16)
    kc = a.kernel_config()
    assert kc["lean"] == 1 and kc["multi_waves"] == 1, kc
    if lean_waves is not None and torch.cuda.get_device_properties(gpu_device).multi_processor_count >= 256:
        assert kc["lean_waves"] == lean_waves, kc
    acts_d = acts.to(gpu_device)
    pick_t = torch.from_numpy(pick).to(gpu_device)
    k0 = 0
    for K in launches:
        obs, rew, done, status, r64 = a.step_multi(acts_d[k0:k0 + K], auto_reset=auto_reset, reward64=True)
        obs_p = obs[:, pick_t].cpu().numpy()
        r64_p, done_p, st_p = (x[:, pick_t].cpu().numpy() for x in (r64, done, status))
        for k in range(K):
            o, r, d, s = b.step(acts_d[k0 + k], auto_reset=auto_reset)
            ctx = "tick %d" % (k0 + k)
            assert torch.equal(obs[k], o), ctx
            assert torch.equal(r64[k], b.reward64) and torch.equal(rew[k], r), ctx
            assert torch.equal(done[k], d) and torch.equal(status[k], s), ctx
            for j, i in enumerate(pick):
                ob_, r_, d_, s_ = rows[int(i)][k0 + k]
                assert (float(r64_p[k, j]), bool(done_p[k, j]), int(st_p[k, j])) == (r_, d_, s_), "env %d %s" % (i, ctx)
                assert obs_p[k, j].tobytes() == ob_, "env %d %s" % (i, ctx)
        k0 += K
    sa, sb = a.export(grid=True), b.export(grid=True)
    for key in sb:
        assert torch.equal(sa[key], sb[key]), key


# ---- the cases' layouts (plain functions: the replay above runs on them without a GPU)

def fan20_case(max_steps):
    cfg = EnvironmentConfig(max_steps=max_steps)
    lays = _shared_camera_layouts(N_ENVS, 20, 15, 411 + max_steps, _f32(96.5), _f32(23.7), _f32(301.3))
    return cfg, lays, 15, 5, 3


WIDE = {"fov126": (126.5, 23.7, 301.3, 40), "fov151": (151.25, 23.7, 301.3, 40), "default_camera": (60.0, 15.0, 0.0, 40)}


def wide20_case(name):
    fov, speed, heading, budget = WIDE[name]
    cfg = EnvironmentConfig(max_steps=2, architect_budget=budget)
    lays = _shared_camera_layouts(N_ENVS, 20, budget, 520, _f32(fov), _f32(speed), _f32(heading))
    return cfg, lays, budget, 13, 8


def ivl20_case(max_steps):
    cfg = EnvironmentConfig(max_steps=max_steps)
    seed = {1: 631, 2: 633, 5: 635}[max_steps]  # chosen on the CPU replay: every situation count >= 1
    return cfg, _interval_fan_layouts(N_ENVS, 20, 15, seed), 15, 5, 3


def mix32_case():
    """4 cameras and 3 guards in every env: half the envs the shared fan's (every camera the
    batch's first camera's twin), a few with a 4-degree fov (the generic body), the rest
    interval fans."""
    budget = 40
    cfg = EnvironmentConfig(grid_rows=32, grid_cols=32, max_steps=2, architect_budget=budget)
    rng = np.random.default_rng(31)
    lays = []
    for walls, cams, guards in synthetic_layouts(N_ENVS, 32, 32, budget, seed=731, n_cams=4, n_guards=3):
        cams = [dict(c) for c in cams]
        u = rng.random()
        for c in cams:
            if u < 0.5:
                c.update(fov_angle=60.0, heading=30.0, rotation_speed=15.0)
            elif u < 0.6:
                c.update(fov_angle=4.0)
        lays.append((walls, cams, guards))
    lays[0][1][0].update(fov_angle=60.0, heading=30.0, rotation_speed=15.0)
    return cfg, lays, budget, 13, 8


def edge20_case():
    """Cameras without guards; guards only, each on a one-point patrol (never off its start);
    one static guard beside one moving guard, with 4 cameras.  Even envs carry the shared
    fan's camera, odd envs cameras of their own (interval fans)."""
    budget = 25
    cfg = EnvironmentConfig(max_steps=2, architect_budget=budget)
    rng = np.random.default_rng(841)
    twin = dict(fov_angle=_f32(75.5), heading=_f32(12.25), rotation_speed=_f32(17.5))
    lays = []
    for i, (walls, cams, _) in enumerate(synthetic_layouts(N_ENVS, 20, 20, budget, seed=842, n_cams=4, n_guards=2)):
        cams = [dict(c, **twin) if i % 2 == 0 else dict(c) for c in cams]
        spots = [(int(r), int(c)) for r, c in rng.integers(3, 17, (2, 2))]
        kind = i % 4
        if kind == 0 and i > 0:
            guards = []
        elif kind == 1:
            cams = []
            guards = [{"patrol_path": [p], "speed": 1, "vision_range": 4, "fov_angle": 90.0} for p in spots]
        else:
            guards = [{"patrol_path": [spots[0]], "speed": 1, "vision_range": 4, "fov_angle": 90.0},
                      {"patrol_path": architect_patrol(spots[1][0], spots[1][1], 20, 20), "speed": 1, "vision_range": 4,
                       "fov_angle": 90.0}]
        lays.append((walls, cams, guards))
    return cfg, lays, budget, 8, 5


# ---- the tests

@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto_reset", "no_reset"])
@pytest.mark.parametrize("max_steps", [1, 2, 5])
def test_fan20_heavy_resets(gpu_device, monkeypatch, max_steps, auto_reset):
    """20 x 20, shared fan (every camera one fov, speed and heading), budget 15, 5 cameras and
    3 guards at most; max_steps 1 resets every env on every tick (consecutive resets, the
    staged entries re-issued from the reset pose each time)."""
    cfg, lays, budget, mc, mg = fan20_case(max_steps)
    _run(gpu_device, monkeypatch, cfg, lays, budget, mc, mg, 900 + max_steps, auto_reset=auto_reset)


@pytest.mark.parametrize("name", list(WIDE))
def test_fan20_wide_fans_with_tie_rays(gpu_device, monkeypatch, name):
    """20 x 20, budget 40 (two cone-stamp passes): fov 126.5 (more than 64 unique directions),
    fov 151.25 (more than 128) and the reference's default camera (heading 0, fov 60, speed 15:
    rays on whole degrees, tie rays on the exact path): the tie rays' tiles are the cameras'
    share and survive the reset."""
    cfg, lays, budget, mc, mg = wide20_case(name)
    _run(gpu_device, monkeypatch, cfg, lays, budget, mc, mg, 910)


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto_reset", "no_reset"])
@pytest.mark.parametrize("max_steps", [1, 2, 5])
def test_ivl20_interval_fans(gpu_device, monkeypatch, max_steps, auto_reset):
    """20 x 20, per-camera fov, heading and speed (the interval fans' pair chunks and their
    exact-path rays are the cameras' share)."""
    cfg, lays, budget, mc, mg = ivl20_case(max_steps)
    _run(gpu_device, monkeypatch, cfg, lays, budget, mc, mg, 920 + max_steps, auto_reset=auto_reset)


@pytest.mark.parametrize("waves", [1, 2])
def test_mix32_one_and_two_waves(gpu_device, monkeypatch, waves):
    """32 x 32 with one and two waves per env (HEIST_LEAN_WAVES; two fit the chip at 64 envs):
    shared-fan, interval-fan and generic envs in one batch; with two waves wave 0 restamps the
    guard plane between two joins and both waves re-read their quads."""
    cfg, lays, budget, mc, mg = mix32_case()
    _run(gpu_device, monkeypatch, cfg, lays, budget, mc, mg, 930, lean_waves=waves)


def test_edge20_layouts(gpu_device, monkeypatch):
    """Cameras without guards, guards that never move (one-point patrols), one static guard
    beside a moving one."""
    cfg, lays, budget, mc, mg = edge20_case()
    _run(gpu_device, monkeypatch, cfg, lays, budget, mc, mg, 940)
