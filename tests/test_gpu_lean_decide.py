"""The lean K-tick kernel (step_lean_kernel) decides the episode's end before it stamps any
guard plane: "some cached guard sees the solver's tile" is one bit of a staged cone row per
guard (the row and column the solver's offset from the guard's pose after the move names, inside
the 15 x 15 window only), "some camera sees it" one byte of the visibility plane after the
marches; the tick then stamps the one guard plane its row shows (the reset poses' when the tick
ends the episode with a guard off its patrol start) and reads the channel-1 quads once.

Pure parity: every case runs 64 envs for 30 ticks in launches of 1, 2, 20 and 7 ticks and
compares heist_step_multi on the lean kernel, bit for bit, with one heist_step per tick on the
single-tick step kernel, with the C oracle for 16 envs (every tick's observation bytes, float64
reward, done, status) and with the exported end state (test_gpu_lean_reset._run).  The cases
also pass on the kernel as it was before the decision moved (checked once when this file was
written): they pin what the tick computes, not how.

A case must exercise the classes of detection it names: a CPU replay through the oracle
(_classes) sorts every env-tick that detects the solver by who sees the solver's tile (guards
only, cameras only, both) and by whether a guard then stands off its patrol start (moved, none
moved), and each named class must occur at the first tick of a launch, at the last tick of a
launch and on two consecutive ticks of one env.  The counts need no GPU.
"""
import functools

import numpy as np
import pytest

import test_gpu_lean_reset as lr
from oracle import pyoracle as po
from heist_amd import EnvironmentConfig
from heist_amd.layouts import architect_patrol, synthetic_layouts
from test_gpu_env import _interval_fan_layouts, _shared_camera_layouts, _twin_envs
from test_gpu_lean_reset import LAUNCHES, N_ENVS, _actions, _f32, _plan, _run
from test_gpu_step_records import _compare, _numpy_record

pytestmark = pytest.mark.gpu

T_WALL = 1
DETECT_CLASSES = ("guard_only", "camera_only", "both", "moved", "none_moved")
MID = (10, 10)  # a start cell with every window offset -8 .. 9 inside the 20 x 20 interior


def _oracle(cfg, lay, budget):
    o = po.OracleEnv(cfg.grid_rows, cfg.grid_cols, cfg.max_steps, cfg.start_pos, cfg.vault_pos, budget)
    ok = o.set_layout(*lay)
    o.reset()
    return o, ok


def _who_sees(o, lay, pos, reset_pose=False):
    """(a camera sees tile pos, a guard sees it) in the oracle's present state; reset_pose: the
    guards stand on patrol point 0 with the headings they have (what a reset leaves)."""
    walls = o.grid() == T_WALL
    ch, gi, gh = o.headings()
    cam = any(po.cone(0, walls, c["row"], c["col"], c["fov_angle"], float(h), c.get("vision_range", 6))[pos]
              for c, h in zip(lay[1], ch))
    guard = False
    for g, j, h in zip(lay[2], gi, gh):
        r, c = g["patrol_path"][0 if reset_pose else int(j)]
        guard = guard or (r, c) == tuple(pos) or bool(
            po.cone(1, walls, int(r), int(c), g["fov_angle"], float(h), g["vision_range"])[pos])
    return cam, guard


def _classes(cfg, lays, budget, acts, launches, auto_reset=True):
    """The oracle's replay of every valid env whose components were all accepted: per class a
    [ticks, envs] mask of the env-ticks that belong to it."""
    n, ticks = len(lays), sum(launches)
    acts = acts.numpy()
    names = DETECT_CLASSES + ("moved_pose_only", "reset_pose_only", "detected_on_vault", "detected_at_timeout")
    m = {k: np.zeros((ticks, n), bool) for k in names}
    for i, lay in enumerate(lays):
        o, ok = _oracle(cfg, lay, budget)
        inf = o.info()
        if not ok or inf["n_cams"] != len(lay[1]) or inf["n_guards"] != len(lay[2]):
            continue
        for t in range(ticks):
            _, d, s = o.step(int(acts[t, i]))
            if s == 4:  # frozen
                break
            inf = o.info()
            pos = (inf["pos_r"], inf["pos_c"])
            if inf["detected"]:
                cam, guard = _who_sees(o, lay, pos)
                assert cam or guard
                _, gi, _ = o.headings()
                off = any(tuple(g["patrol_path"][int(j)]) != tuple(g["patrol_path"][0]) for g, j in zip(lay[2], gi))
                m["guard_only"][t, i] = guard and not cam
                m["camera_only"][t, i] = cam and not guard
                m["both"][t, i] = cam and guard
                m["moved"][t, i] = off
                m["none_moved"][t, i] = not off
                m["detected_on_vault"][t, i] = bool(inf["vault_reached"])
                m["detected_at_timeout"][t, i] = s == 3
            if d and lay[2] and not lay[1]:  # guards alone: the pose that decides against the pose the row shows
                seen = bool(inf["detected"])
                _, at_reset = _who_sees(o, lay, pos, reset_pose=True)
                m["moved_pose_only"][t, i] = seen and not at_reset
                m["reset_pose_only"][t, i] = at_reset and not seen
            if d and auto_reset:
                o.reset()
    return m


def _situations(mask, launches):
    firsts = np.cumsum((0,) + tuple(launches[:-1]))
    lasts = np.cumsum(launches) - 1
    return {"first_tick": int(mask[firsts].sum()), "last_tick": int(mask[lasts].sum()),
            "consecutive": int((mask[1:] & mask[:-1]).sum())}


def _check_classes(cfg, lays, budget, seed, need, once=(), auto_reset=True, launches=LAUNCHES):
    """Each class of `need` at the first tick of a launch, at the last tick of a launch and on two
    consecutive ticks of one env; each class of `once` on some tick."""
    m = _classes(cfg, lays, budget, _actions(len(lays), sum(launches), seed), launches, auto_reset)
    for key in need:
        sit = _situations(m[key], launches)
        print(key, sit)
        for name, cnt in sit.items():
            assert cnt >= 1, (key, name, sit)
    for key in once:
        print(key, int(m[key].sum()))
        assert m[key].any(), key


def _guard(path, rng_=4, fov=90.0):
    return {"patrol_path": [tuple(int(x) for x in p) for p in path], "speed": 1, "vision_range": int(rng_), "fov_angle": fov}


# ---- the cases' layouts (plain functions: the replays above run on them without a GPU)

# the solver's start cell minus the guard's pose after its first move: the 15 x 15 window is
# -7 .. 7 on both axes, so -9 .. 9 reaches two tiles past it on each side
SWEEP = [(dr, dc) for dr in range(-9, 10) for dc in range(-9, 10)]
_STEPS = [(0, 1), (1, 0), (0, -1), (-1, 0)]


def _inside(p):
    return 1 <= p[0] <= 18 and 1 <= p[1] <= 18


def _patrol_through(p1, kind, start, vault):
    """A patrol whose point 1 is p1: two points (kind even) or a longer loop (kind odd), entered
    from a neighbour the kind picks (so the heading slot differs between envs); point 0 avoids the
    start and the vault cell."""
    for turn in range(4):
        dr, dc = _STEPS[(kind // 2 + turn) % 4]
        p0 = (p1[0] - dr, p1[1] - dc)
        if _inside(p0) and p0 not in (start, vault):
            break
    else:
        raise AssertionError(p1)
    if kind % 2 == 0:
        return [p0, p1]
    path = [p0, p1]
    for s in range(1, 5):  # onward with right turns where the grid allows, 6 points
        ndr, ndc = _STEPS[(kind // 2 + turn + (s + 1) // 2) % 4]
        q = (path[-1][0] + ndr, path[-1][1] + ndc)
        path.append(q if _inside(q) else path[-2])
    return path


def sweep20_case(block):
    """Guards only.  Env i of block b puts the pose after the first move of one guard at the start
    cell minus SWEEP[64 b + i]: blocks 0-4 from start (10, 10) (offsets -8 .. 9, the guard on
    every interior cell: windows clipped by all four edges and the corners), block 5 from start
    (9, 9) (the offsets with a -9, then offsets of the earlier blocks again in other variants).
    One guard or three (the swept one in any slot), two-point and longer patrols, vision ranges
    4 .. 7, fovs 90 and 120 degrees."""
    start = MID if block < 5 else (9, 9)
    vault = (18, 18) if block % 2 == 0 else (1, 18)
    cfg = EnvironmentConfig(max_steps=2, start_pos=start, vault_pos=vault)
    reach = [o for o in SWEEP if _inside((start[0] - o[0], start[1] - o[1]))]
    if block < 5:
        offs = reach[64 * block:64 * block + 64]
    else:
        first = [o for o in SWEEP if _inside((9 - o[0], 9 - o[1])) and not _inside((10 - o[0], 10 - o[1]))]
        offs = first + [o for o in SWEEP if max(abs(o[0]), abs(o[1])) <= 8][::5]
    rng = np.random.default_rng(1200 + block)
    lays = []
    for i in range(N_ENVS):
        dr, dc = offs[i % len(offs)]
        p1 = (start[0] - dr, start[1] - dc)
        swept = _guard(_patrol_through(p1, i + block, start, vault), 4 + (i + block) % 4, 90.0 if i % 3 else 120.0)
        guards = [swept]
        if i % 2:  # two more guards elsewhere, the swept one in slot i % 3
            others = []
            while len(others) < 2:
                q = tuple(int(x) for x in rng.integers(1, 19, 2))
                if q not in (start, vault):
                    others.append(_guard(_patrol_through(q, int(rng.integers(0, 8)), start, vault), 4, 90.0))
            guards = others[:i % 3] + [swept] + others[i % 3:]
        lays.append(([], [], guards))
    return cfg, lays, 15, 5, 3


def cams20_case(kind):
    """Cameras only, the start cell in the middle of the grid: the shared fan (every camera one
    fov, speed and heading) or interval fans (each camera its own)."""
    cfg = EnvironmentConfig(max_steps=2, start_pos=MID)
    if kind == "fan":
        lays = _shared_camera_layouts(N_ENVS, 20, 15, 1301, _f32(96.5), _f32(23.7), _f32(301.3), n_guards=0, start=MID)
    else:
        lays = _interval_fan_layouts(N_ENVS, 20, 15, 1302, n_guards=0, start=MID)
    return cfg, lays, 15, 5, 3


def both20_case(max_steps=2, vault=(18, 18)):
    """Cameras and guards around a start cell in the middle of the grid: even envs the shared fan's
    camera, odd envs cameras of their own; one or two guards whose patrol passes within two tiles
    of the start cell."""
    cfg = EnvironmentConfig(max_steps=max_steps, start_pos=MID, vault_pos=vault, architect_budget=25)
    rng = np.random.default_rng(1400)
    twin = dict(fov_angle=_f32(110.5), heading=_f32(40.25), rotation_speed=_f32(21.5))
    lays = []
    for i, (walls, cams, _) in enumerate(synthetic_layouts(N_ENVS, 20, 20, 25, seed=1401, n_cams=4, n_guards=2,
                                                           start=MID, vault=vault)):
        cams = [dict(c, row=int(MID[0] + rng.integers(-4, 5)), col=int(MID[1] + rng.integers(-4, 5))) for c in cams]
        cams = [c for j, c in enumerate(cams) if (c["row"], c["col"]) not in (MID, vault)
                and (c["row"], c["col"]) not in [(d["row"], d["col"]) for d in cams[:j]]]
        walls = [w for w in walls if w not in [(c["row"], c["col"]) for c in cams]]
        cams = [dict(c, **twin) if i % 2 == 0 else c for c in cams]
        guards = []
        for _ in range(1 + i % 2):
            p1 = (int(MID[0] + rng.integers(-2, 3)), int(MID[1] + rng.integers(-2, 3)))
            guards.append(_guard(_patrol_through(p1, int(rng.integers(0, 8)), MID, vault), 4 + int(rng.integers(0, 4))))
        lays.append((walls, cams, guards))
    return cfg, lays, 25, 8, 5


def disagree20_case():
    """Guards only, max_steps 1 (every tick ends the episode, so every row shows the reset pose):
    two-point patrols beside the start cell, so that the solver's tile after its move lies in the
    cone of the pose after the move and not in the reset pose's, or the reverse."""
    cfg = EnvironmentConfig(max_steps=1, start_pos=MID)
    rng = np.random.default_rng(1500)
    lays = []
    for i in range(N_ENVS):
        p1 = (int(MID[0] + rng.integers(-3, 4)), int(MID[1] + rng.integers(-3, 4)))
        lays.append(([], [], [_guard(_patrol_through(p1, 2 * (i % 4), MID, (18, 18)), 4 + i % 2)]))
    return cfg, lays, 15, 5, 3


def still20_case():
    """No guard off its start when the episode ends: one-point patrols (heading 0 for ever, so the
    guard stands west of the start cell), alone, in pairs and beside cameras; every fourth env a
    static guard beside a moving one."""
    cfg = EnvironmentConfig(max_steps=2, start_pos=MID, architect_budget=25)
    rng = np.random.default_rng(1600)
    lays = []
    for i, (walls, cams, _) in enumerate(synthetic_layouts(N_ENVS, 20, 20, 25, seed=1601, n_cams=2, n_guards=2,
                                                           start=MID)):
        spot = lambda: (int(MID[0] + rng.integers(-2, 3)), int(MID[1] - rng.integers(1, 5)))  # noqa: E731
        guards = [_guard([spot()], 4 + i % 4)]
        if i % 4 == 1:
            guards.append(_guard([spot()], 5))
        if i % 4 == 3:
            guards.append(_guard(architect_patrol(int(rng.integers(3, 17)), int(rng.integers(3, 17)), 20, 20)))
        if i % 4 != 2:
            cams = []
        taken = [g["patrol_path"][0] for g in guards]
        cams = [c for c in cams if (c["row"], c["col"]) not in taken]
        walls = [w for w in walls if w not in taken]
        lays.append((walls, cams, guards))
    return cfg, lays, 25, 8, 5


def mix32_case():
    """32 x 32, 4 cameras and 3 guards around a start cell in the middle: half the envs the shared
    fan's (every camera the batch's first camera's twin), a few with a 4-degree fov (the generic
    body), the rest interval fans."""
    budget, mid = 40, (16, 16)
    cfg = EnvironmentConfig(grid_rows=32, grid_cols=32, max_steps=2, architect_budget=budget, start_pos=mid)
    rng = np.random.default_rng(1700)
    lays = []
    for walls, cams, guards in synthetic_layouts(N_ENVS, 32, 32, budget, seed=1701, n_cams=4, n_guards=3, start=mid):
        u = rng.random()
        cams = [dict(c) for c in cams]
        for c in cams:
            if u < 0.5:
                c.update(fov_angle=60.0, heading=30.0, rotation_speed=15.0)
            elif u < 0.6:
                c.update(fov_angle=4.0)
        g0 = (int(mid[0] + rng.integers(-3, 4)), int(mid[1] + rng.integers(-3, 4)))
        guards = [dict(guards[0], patrol_path=architect_patrol(g0[0], g0[1], 32, 32))] + list(guards[1:])
        lays.append((walls, cams, guards))
    lays[0][1][0].update(fov_angle=60.0, heading=30.0, rotation_speed=15.0)
    return cfg, lays, budget, 13, 8


def _go(gpu_device, monkeypatch, case, seed, need, once=(), auto_reset=True, reset_counts=True, **kw):
    """The classes on the CPU, then test_gpu_lean_reset._run on the GPU.  reset_counts False: the
    case cannot meet that file's own situation counts (episodes that end with a guard off its
    start; with no guard, or none that moves, there is none): this file's classes stand for them."""
    cfg, lays, budget, mc, mg = case
    _check_classes(cfg, lays, budget, seed, need, once, auto_reset)
    if not reset_counts:
        monkeypatch.setattr(lr, "_check_counts", lambda *a: None)
    _run(gpu_device, monkeypatch, cfg, lays, budget, mc, mg, seed, auto_reset=auto_reset, **kw)


# ---- the tests

@pytest.mark.parametrize("block", range(6))
def test_guard_window_sweep(gpu_device, monkeypatch, block):
    """Detection rests on the cone row's bit alone: the start cell over the whole window of the
    pose after the first move and one and two tiles past each side (not seen, not a wrapped
    index), the window clipped by every grid edge and corner."""
    _go(gpu_device, monkeypatch, sweep20_case(block), 1210 + block, ("guard_only", "moved"))


@pytest.mark.parametrize("kind", ["fan", "ivl"])
def test_cameras_only(gpu_device, monkeypatch, kind):
    """Detection rests on the visibility plane's byte alone."""
    _go(gpu_device, monkeypatch, cams20_case(kind), 1310, ("camera_only", "none_moved"), reset_counts=False)


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto_reset", "no_reset"])
def test_cameras_and_guards(gpu_device, monkeypatch, auto_reset):
    """Both a camera and a guard see the cell; without auto-reset the frozen rows repeat the
    planes of the tick that ended the episode."""
    need = ("guard_only", "camera_only", "both", "moved") if auto_reset else ()
    _go(gpu_device, monkeypatch, both20_case(), 1410, need, once=("both", "guard_only", "camera_only"),
        auto_reset=auto_reset)


def test_poses_that_disagree(gpu_device, monkeypatch):
    """The moved pose decides, the row shows the reset pose."""
    _go(gpu_device, monkeypatch, disagree20_case(), 1510, ("moved_pose_only", "reset_pose_only", "guard_only"))


def test_no_moved_guard_on_reset(gpu_device, monkeypatch):
    _go(gpu_device, monkeypatch, still20_case(), 1610, ("none_moved", "guard_only"), once=("moved", "camera_only"),
        reset_counts=False)


@pytest.mark.parametrize("max_steps", [1, 2])
def test_vault_and_timeout_on_a_detection(gpu_device, monkeypatch, max_steps):
    """The vault beside the start cell, inside the cones: status and reward take the reference's
    order (detected, then vault, then timeout on one tick)."""
    case = both20_case(max_steps, vault=(10, 11))
    _go(gpu_device, monkeypatch, case, 1420 + max_steps, ("moved",), once=("detected_on_vault", "detected_at_timeout"))


@pytest.mark.parametrize("waves", [1, 2])
def test_mix32_one_and_two_waves(gpu_device, monkeypatch, waves):
    """32 x 32 with one and two waves per env: both waves decide alike from the plane's byte and
    the cone rows wave 0 staged."""
    _go(gpu_device, monkeypatch, mix32_case(), 1710, ("guard_only", "camera_only", "moved"), lean_waves=waves)


@functools.lru_cache(maxsize=None)
def _records_case():
    cfg, lays, budget, mc, mg = both20_case()
    acts = _actions(len(lays), sum(LAUNCHES), 1410)
    _, pick, rows, _ = _plan(cfg, lays, budget, acts, LAUNCHES, True)
    want = {int(i): np.stack([_numpy_record(r[0], 20, 20, cfg.vault_pos) for r in rows[int(i)]]) for i in pick}
    return cfg, lays, budget, mc, mg, acts, pick, rows, want


def test_records_form(gpu_device, monkeypatch):
    """step_multi_records on the cameras-and-guards case: the record equals the packed observation
    of the same ticks (heist_step, pack_obs) and the record built from the oracle's."""
    cfg, lays, budget, mc, mg, acts, pick, rows, want = _records_case()
    monkeypatch.setenv("HEIST_MULTI_WAVES", "1")
    a, b = _twin_envs(len(lays), cfg, lays, budget, gpu_device, max_cams=mc, max_guards=mg, max_path=16)
    assert a.records_direct == 1 and a.kernel_config()["lean"] == 1
    _compare(a, b, acts.to(gpu_device), True, pick, rows, want)
    a.close()
    b.close()
