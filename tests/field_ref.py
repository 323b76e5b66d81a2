"""References for heist_plan_field (HeistEnv.plan_field): the fewest undetected ticks to the vault
from every cell, none of which uses the kernel under test.

* field_from_planes: the backward recurrence of include/heist.h in NumPy, on boolean [R, C]
  planes, given the visibility plane of every tick.
* witness_planes: those planes from the C oracle (oracle.pyoracle.OracleEnv).  The visibility of
  tick k does not depend on the Solver, and an env that was still running before tick k shows
  vis_k after it, so one WAITing witness env is parked on every cell it can be parked on and each
  tick's plane is taken from the witnesses still running, which must all agree.  An OracleEnv's
  Solver starts where the env's start tile is, and a start tile refuses a wall or a camera
  (environment.py:160-167), so the oracle's witnesses stand on the tiles the layout leaves empty
  (and on the start and the vault); the GPU's witnesses, parked by a state edit, stand on every
  non-wall cell.
* bfs_dist: ticks to the vault with nobody watching.
* the test layouts: plan_ref.CASES (10 x 10) and shape_layouts for the larger grids.
"""
import functools

import numpy as np

import plan_ref as pr
from heist_amd.layouts import synthetic_layout
from oracle import pyoracle as po

DELTA = pr.DELTA
NONE = -1


def moves(walls):
    """[5, R, C] flat index of move(x, a) for every cell x: x + delta(a) if inside the grid and
    not a wall, else x."""
    R, C = walls.shape
    rr, cc = np.meshgrid(np.arange(R), np.arange(C), indexing="ij")
    out = np.empty((5, R, C), np.int64)
    for a, (dr, dc) in enumerate(DELTA):
        yr, yc = rr + dr, cc + dc
        ok = (yr >= 0) & (yr < R) & (yc >= 0) & (yc < C)
        ok &= ~walls[np.clip(yr, 0, R - 1), np.clip(yc, 0, C - 1)]
        out[a] = np.where(ok, yr * C + yc, rr * C + cc)
    return out


def field_from_planes(walls, vault, planes, tick0=0, max_steps=200, done=False):
    """(togo [R, C] int16, action [R, C] int8, ticks [HK, R, C] int16) for the ticks planes[0],
    planes[1], ... gives the visibility of (planes[k] is vis_{k+1}); HK = min(len(planes),
    max_steps - tick0), 0 when done.  ticks[k] is togo_k, togo = ticks[0] (all -1 when HK is 0),
    action the lowest action that attains it."""
    walls = np.asarray(walls, bool)
    R, C = walls.shape
    HK = 0 if done else max(0, min(len(planes), max_steps - tick0))
    mv = moves(walls).reshape(5, -1)
    vcell = vault[0] * C + vault[1]
    big = np.int64(1 << 20)
    nxt = np.full(R * C, big)  # togo_HK: none
    ticks = np.full((HK, R, C), NONE, np.int16)
    action = np.full(R * C, NONE, np.int8)
    for k in range(HK - 1, -1, -1):
        seen = np.asarray(planes[k], bool).reshape(-1)
        best = np.full(R * C, big)
        act = np.full(R * C, NONE, np.int8)
        for a in range(5):
            y = mv[a]
            val = np.where(seen[y], big, np.where(y == vcell, 1, np.where(nxt[y] >= big, big, nxt[y] + 1)))
            better = val < best  # strict: the first minimum stays
            best = np.where(better, val, best)
            act = np.where(better, a, act).astype(np.int8)
        best[walls.reshape(-1)] = big
        act[best >= big] = NONE
        ticks[k] = np.where(best >= big, NONE, best).astype(np.int16).reshape(R, C)
        nxt, action = best, act
    togo = ticks[0] if HK else np.full((R, C), NONE, np.int16)
    if not HK:
        action = np.full(R * C, NONE, np.int8)
    return togo, action.reshape(R, C), ticks


def bfs_dist(walls, vault):
    """[R, C] int: moves to the vault over non-wall cells, -1 where there is no path."""
    walls = np.asarray(walls, bool)
    R, C = walls.shape
    dist = np.full((R, C), -1, np.int64)
    dist[vault] = 0
    frontier = [tuple(vault)]
    while frontier:
        nxt = []
        for r, c in frontier:
            for dr, dc in DELTA[1:]:
                y = (r + dr, c + dc)
                if 0 <= y[0] < R and 0 <= y[1] < C and not walls[y] and dist[y] < 0:
                    dist[y] = dist[r, c] + 1
                    nxt.append(y)
        frontier = nxt
    return dist


def oracle_env(R, C, max_steps, start, vault, layout, budget):
    o = po.OracleEnv(R, C, max_steps, start, vault, budget)
    valid = o.set_layout(*layout)
    o.reset()
    return o, valid


def witness_planes(R, C, max_steps, start, vault, layout, budget, horizon=None):
    """(planes, walls, counts): planes[k - 1] the bool [R, C] visibility of tick k = 1 .. horizon
    of the layout played from reset, walls the bool wall plane (the layout's and the border),
    counts[k - 1] the number of witnesses that showed tick k.  AssertionError if two witnesses of
    a tick disagree, if a witness's grid differs from the env's own outside its start tile, or if
    a tick has no witness."""
    horizon = max_steps if horizon is None else min(horizon, max_steps)
    base, _ = oracle_env(R, C, max_steps, start, vault, layout, budget)
    grid = base.grid()
    walls = grid == 1
    cells = [(r, c) for r in range(R) for c in range(C) if grid[r, c] in (0, 2, 3)]  # empty, start, vault
    wit = []
    for cell in cells:
        o, _ = oracle_env(R, C, max_steps, cell, vault, layout, budget)
        g = o.grid()
        same = (g == grid) | (g == 2) | (grid == 2)  # the start tile is the witness's own
        assert same.all() and ((g == 1) == walls).all(), "witness %s changes the layout" % (cell,)
        wit.append(o)
    planes, counts = [], []
    for k in range(1, horizon + 1):
        plane, n = None, 0
        for cell, o in zip(cells, wit):
            if o.info()["done"]:
                continue
            o.step(0)
            v = o.visibility().astype(bool)
            if plane is None:
                plane = v
            else:
                assert (plane == v).all(), "tick %d: witness %s disagrees" % (k, cell)
            n += 1
        assert plane is not None, "tick %d has no witness left" % k
        planes.append(plane)
        counts.append(n)
    return planes, walls, counts


def pack_planes(planes, W):
    """[len(planes), W] uint32: the planes in the record's bit order (bit i of word j is cell
    32 j + i), zero padded."""
    out = np.zeros((len(planes), W), np.uint32)
    for k, p in enumerate(planes):
        bits = np.zeros(32 * W, np.uint64)
        flat = np.asarray(p, bool).reshape(-1)
        bits[:flat.size] = flat
        out[k] = (bits.reshape(W, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """A plan_ref.CASES fixture from reset, all 40 ticks: (planes, walls, counts, togo, action,
    ticks) -- the oracle's witness planes and field_from_planes on them.  Computed once; callers
    must not modify it.  The witnesses all start at the handle's start (1, 1) in the planes'
    sense: start_on_vault differs from empty only in the cell the Solver stands on."""
    layout, _, _, _ = pr.CASES[name]
    planes, walls, counts = witness_planes(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, layout, pr.BUDGET)
    togo, action, ticks = field_from_planes(walls, pr.VAULT, planes, 0, pr.MAX_STEPS)
    return planes, walls, counts, togo, action, ticks


def cases_field(names, W):
    """The reference fields of the named fixtures as a CPU heist_amd.PlanField (H = 40)."""
    import torch
    from heist_amd import PlanField
    refs = [case_reference(n) for n in names]
    vis = np.stack([pack_planes(r[0], W) for r in refs], 1)  # [H, N, W]
    ticks = np.stack([r[5] for r in refs], 1)                # [H, N, R, C]
    return PlanField(torch.from_numpy(np.stack([r[3] for r in refs])), torch.from_numpy(np.stack([r[4] for r in refs])),
                     torch.from_numpy(vis.view(np.int32)), torch.from_numpy(ticks), pr.GRID, pr.GRID, pr.VAULT)


# ---- layouts for the larger grids (start (1, 1), vault (R - 2, C - 2))

def wallrow(R, C):
    """A wall row above the middle with one gap: (walls, its row, the gap's column)."""
    rw, g = R // 2 - 1, C // 2
    return [(rw, c) for c in range(1, C - 1) if c != g], rw, g


def shape_layouts(R, C, seed):
    """Empty; a wall row whose gap is watched by a turning camera (forced waits), by a camera that
    never turns (BFS-valid, the start's side never clean), by a guard of range 8 (off the cone
    cache: raycast live every tick), by camera and a cached guard; two random layouts, the last
    with 5 cameras and 3 guards."""
    walls, rw, g = wallrow(R, C)

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


# name -> (R, C, max_steps, guard cone cache on)
SHAPES = {"10x10": (10, 10, 40, True), "10x10_live_guards": (10, 10, 40, False), "13x17": (13, 17, 50, True),
          "20x20": (20, 20, 60, True), "32x32": (32, 32, 80, True)}

# shape -> how many of shape_layouts' layouts the witness test uses: those that keep a witness
# through every tick of max_steps.  Counted with the oracle's witnesses (a subset of the GPU's),
# fewest per tick: 10 x 10: 63, 15, 42, 31, 14, 1; 13 x 17: 164, 63, 133, 81, 56, 29; 20 x 20: 323,
# 205, 289, 211, 198, 108, 27.  The 5-camera 3-guard layout sees every witness of the 10 x 10 grid
# by tick 7 and of the 13 x 17 grid by tick 20, so it is witnessed at 20 x 20 only.
WITNESS_LAYOUTS = {"10x10_live_guards": 6, "13x17": 6, "20x20": 7}
