"""Reference for heist_plan_place_guard (HeistEnv.plan_place_guard): the planner's answers with one
more guard, without the kernel under test and without any notion of a candidate.

A variant's reference is BASE with the candidate APPENDED TO ITS GUARD LIST, handed to what the other
planner tests already trust: plan_ref.oracle_search for the fewest ticks, field_ref.witness_planes
for the visibility of every tick, field_ref.field_from_planes / value_ref.value_from_planes on those
planes for the tables -- what place_ref does for cameras.

One trap: witness_planes needs a cell that stays unseen, and under BASE plus the rectangle or the
border candidate every waiting witness is detected by tick 11, so the plus-layout shows 10 ticks
only.  A variant's planes are therefore built as base | alone -- the candidate alone over BASE's
walls always has witnesses -- and test_plan_place_guard_cpu.py holds plus == base | alone wherever
plus has a witness.

BASE: the plan_ref 10 x 10 set-up (start (1, 1), vault (8, 8), max_steps 40) with WALLROW, cam(270,
30) and GUARD.  BUDGET = 60 buys the base layout and any candidate.

A candidate is a tuple (path, speed, vision_range, fov): path a tuple of (row, col), the guard as
heist_set_layout leaves it (patrol index 0, heading 0.0).
"""
import functools
import math

import numpy as np

import field_ref as fr
import plan_ref as pr
import value_ref as vr

BUDGET = 60
BASE = (pr.WALLROW, [pr.cam(270, 30)], [pr.GUARD])
D0 = abs(pr.START[0] - pr.VAULT[0]) + abs(pr.START[1] - pr.VAULT[1])
CAM_TILE = (6, 5)
GUARD_START = pr.GUARD["patrol_path"][0]
P = 8  # the patrol array's width in the tests: every candidate is shorter (len < P, garbage behind)


def cand(path, speed=1, rng=4, fov=90.0):
    return (tuple((int(r), int(c)) for r, c in path), int(speed), int(rng), float(fov))


RECT = [(2, 2), (2, 3), (2, 4), (3, 4), (3, 3), (3, 2)]
# the candidates of the union premise (test_plan_place_guard_cpu.py), all valid
PREMISE = {
    "through_wall": cand([(3, 3), (4, 3), (5, 3), (6, 3)]),
    "still": cand([(7, 2)]),
    "jump": cand([(2, 6), (6, 2), (7, 7)], speed=2, rng=8, fov=200.0),   # 400 rays: more than 64 unique directions
    "range0": cand([(2, 7), (2, 8)], rng=0),
    "rectangle": cand(RECT),
    "border": cand([(1, 5), (0, 5), (1, 6)]),
    "negative_speed": cand(RECT, speed=-1),              # Python's %: step 5, the rectangle walked backwards
    "speed_multiple_of_len": cand(RECT, speed=12),       # step 0: never moves
    "repeated_point": cand([(7, 3), (7, 3), (7, 4), (7, 4), (6, 4)]),   # a move onto the same tile keeps the heading
}
# the two whose plus-layout runs out of witnesses (every waiting witness detected by tick 11)
SHORT_WITNESS = ("rectangle", "border")
FULL_WITNESS = ("through_wall", "still", "jump", "range0")   # all 40 ticks witnessed
# a moving guard that leaves BASE solvable (oracle_search: 22 ticks, by another plan than BASE's): the mid-episode test's
CORNER = cand([(1, 7), (1, 8), (2, 8), (2, 7)], rng=2)
# name -> a candidate that is not valid because of its path; START_ON_WALL breaks the premise itself
START_ON_WALL = cand([(4, 2), (3, 2)])
INVALID = {
    "start_on_wall": START_ON_WALL,
    "start_on_border": cand([(0, 5), (1, 5)]),
    "start_on_camera": cand([CAM_TILE, (6, 6)]),
    "start_on_guard": cand([GUARD_START, (5, 3)]),
    "start_on_start": cand([pr.START, (1, 2)]),
    "start_on_vault": cand([pr.VAULT, (8, 7)]),
    "point_past_grid": cand([(2, 2), (2, pr.GRID)]),
    "negative_point": cand([(2, 2), (-1, 2)]),
    "zero_fov": cand([(2, 2)], fov=0.0),
    "nan_fov": cand([(2, 2)], fov=float("nan")),
    "negative_range": cand([(2, 2)], rng=-1),
    "range_past_int16": cand([(2, 2)], rng=32768),
    "empty_path": cand([]),
}


def guard_dict(c):
    return {"patrol_path": list(c[0]), "speed": c[1], "vision_range": c[2], "fov_angle": c[3]}


def with_cand(layout, c):
    """The layout with candidate c appended to its guard list (c None: the layout itself)."""
    walls, cams, guards = layout
    return (walls, cams, list(guards) + ([] if c is None else [guard_dict(c)]))


def alone(c):
    """The base layout's walls with the candidate as the only emitter."""
    return (BASE[0], [], [guard_dict(c)])


@functools.lru_cache(maxsize=None)
def base_grid():
    o, _ = fr.oracle_env(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, BASE, BUDGET)
    return o.grid()


def expect_valid(c, idx=0, heading=0.0, p=P):
    """The contract's validity (include/heist.h, 1 - 6) of candidate c on BASE, restated."""
    path, speed, rng, fov = c
    n, R, C = len(path), pr.GRID, pr.GRID
    if not (1 <= n <= p and 0 <= idx < n):
        return False
    if not all(0 <= r < R and 0 <= q < C for r, q in path):
        return False
    r0, c0 = path[0]
    if not (0 < r0 < R - 1 and 0 < c0 < C - 1 and base_grid()[r0, c0] == 0):
        return False
    if not (0.0 < fov <= 16000.0):
        return False
    if not (abs(heading) <= 1e300):
        return False
    return 0 <= rng < 32768


def bought(layout):
    """(n_cams, n_guards) the oracle's purchase keeps of a layout at BUDGET."""
    o = pr.po.OracleEnv(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, BUDGET)
    o.set_layout(*layout)
    i = o.info()
    return i["n_cams"], i["n_guards"]


def witnessed(layout):
    """(planes, walls) of a layout from reset for as many ticks as it has a witness (at most 40)."""
    args = (pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, layout, BUDGET)
    o, _ = fr.oracle_env(*args)
    walls = o.grid() == 1
    h = pr.MAX_STEPS
    while h > 0:
        try:
            p, w, _ = fr.witness_planes(*args, horizon=h)
            assert (w == walls).all()
            return p, walls
        except AssertionError as ex:
            msg = str(ex)
            if "has no witness left" not in msg:
                raise
            h = int(msg.split()[1]) - 1  # "tick K has no witness left"
    return [], walls


@functools.lru_cache(maxsize=None)
def planes_of(layout_key):
    """(planes, walls): layout_key "base" or ("alone", c): all 40 ticks; ("plus", c): the ticks the
    plus-layout has a witness for.  Computed once; callers must not modify it."""
    if layout_key == "base" or layout_key[0] == "alone":
        lay = BASE if layout_key == "base" else alone(layout_key[1])
        p, walls, _ = fr.witness_planes(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, lay, BUDGET)
        return p, walls
    return witnessed(with_cand(BASE, layout_key[1]))


def search(c, prefix=(), horizon=None):
    """plan_ref.oracle_search of BASE plus candidate c after `prefix` actions."""
    return pr.oracle_search(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, with_cand(BASE, c), BUDGET,
                            horizon=horizon, prefix=prefix)


@functools.lru_cache(maxsize=None)
def reference(c, gamma):
    """Variant c (None: the baseline) from reset: dict(valid, ticks -- togo at the start cell; togo
    [R, C] int16; value [R, C] float64, action [R, C] int8; planes, walls).  The planes are base |
    alone.  Computed once; callers must not modify it."""
    ok = c is not None and expect_valid(c)
    p, walls = planes_of("base")
    if ok:
        own, walls_own = planes_of(("alone", c))
        assert (walls == walls_own).all()
        p = [a | b for a, b in zip(p, own)]
    togo = fr.field_from_planes(walls, pr.VAULT, p, 0, pr.MAX_STEPS)[0]
    value, action = vr.value_from_planes(walls, pr.VAULT, p, D0, 0, pr.MAX_STEPS, gamma)[:2]
    return {"valid": ok, "ticks": int(togo[pr.START]), "togo": togo, "value": value, "action": action, "planes": p,
            "walls": walls}


def arrays(cands, p=P, garbage=True):
    """The kernel's three arrays for a list of candidates: (paths int32 [M, p, 2], meta int32 [M, 4],
    fov float64 [M, 2]) as NumPy, patrol index 0 and heading 0.0; the unused points hold garbage
    (values outside the grid, INT32_MIN among them) when asked."""
    M = len(cands)
    fill = np.array([-(2 ** 31), 2 ** 31 - 1, 1000, -7], np.int64)
    paths = np.zeros((M, p, 2), np.int32)
    if garbage:
        paths[:] = fill[np.arange(M * p * 2) % 4].reshape(M, p, 2).astype(np.int32)
    meta = np.zeros((M, 4), np.int32)
    fov = np.zeros((M, 2), np.float64)
    for m, (path, speed, rng, f) in enumerate(cands):
        assert len(path) <= p
        for j, (r, c) in enumerate(path):
            paths[m, j] = (r, c)
        meta[m] = (len(path), speed, rng, 0)
        fov[m] = (f, 0.0)
    return paths, meta, fov


assert all(math.isfinite(c[3]) for c in PREMISE.values())
