"""Reference for heist_plan_place (HeistEnv.plan_place): the planner's answers with one more camera,
without the kernel under test and without any notion of a candidate.

A variant's reference is the layout with the candidate APPENDED TO ITS CAMERA LIST, handed to what
the other planner tests already trust: plan_ref.oracle_search (the C oracle expanded level by level)
for the fewest ticks, field_ref.witness_planes for the visibility of every tick, and
field_ref.field_from_planes / value_ref.value_from_planes on those planes for the tables -- what
masked_ref does for removed emitters.

BASE: the plan_ref 10 x 10 set-up (start (1, 1), vault (8, 8), max_steps 40) with WALLROW, cam(270,
30) and GUARD.  BUDGET = 40 buys the base layout (7 walls, a camera, a guard: 15) and any candidate.

A candidate is a tuple (row, col, fov, heading, speed, range), the kernel's cand row.  The oracle's
purchase decides whether it is placeable -- except on the guard's start tile, the one divergence the
contract names (a rebuilt layout places cameras before guards and would accept it), and for rows the
oracle is never shown (a NaN, a tile outside the grid): there the reference is the base layout's.
"""
import functools
import math

import field_ref as fr
import plan_ref as pr
import value_ref as vr

BUDGET = 40
BASE = (pr.WALLROW, [pr.cam(270, 30)], [pr.GUARD])
D0 = abs(pr.START[0] - pr.VAULT[0]) + abs(pr.START[1] - pr.VAULT[1])
GUARD_START = pr.GUARD["patrol_path"][0]


def cand(row, col, heading, speed, fov=60.0, rng=6):
    return (float(row), float(col), float(fov), float(heading), float(speed), float(rng))


# the candidates of the union premise (test_plan_place_cpu.py), all placeable
PREMISE = [cand(2, 2, 0, 0), cand(7, 3, 90, 15), cand(3, 8, 200, -20), cand(8, 1, 45, 7), cand(5, 5, 0, 0),
           cand(4, 5, 180, 30)]
SAME_FAN = cand(6, 3, 270, 30)        # the existing camera's heading, speed, fov and range on another tile
BLIND = cand(2, 6, 0, 0, rng=0)       # range 0: sees nothing
VALID = PREMISE + [SAME_FAN, BLIND]
# name -> a candidate that is not valid
INVALID = {
    "camera_tile": cand(6, 5, 0, 0), "wall": cand(4, 2, 0, 0), "border": cand(0, 4, 0, 0),
    "negative_row": cand(-3, 4, 0, 0), "col_past_grid": cand(4, pr.GRID, 0, 0), "row_past_grid": cand(pr.GRID + 7, 4, 0, 0),
    "start": cand(pr.START[0], pr.START[1], 0, 0), "vault": cand(pr.VAULT[0], pr.VAULT[1], 0, 0),
    "guard_start": cand(GUARD_START[0], GUARD_START[1], 0, 0), "nan_fov": cand(2, 2, 0, 0, fov=float("nan")),
}


def cam_dict(c):
    return {"row": int(c[0]), "col": int(c[1]), "fov_angle": c[2], "heading": c[3], "rotation_speed": c[4],
            "vision_range": int(c[5])}


def with_cand(layout, c):
    """The layout with candidate c appended to its camera list (c None: the layout itself)."""
    walls, cams, guards = layout
    return (walls, list(cams) + ([] if c is None else [cam_dict(c)]), guards)


def alone(c):
    """The base layout's walls with the candidate as the only emitter."""
    return (BASE[0], [cam_dict(c)], [])


def oracle_shown(c):
    """The oracle is shown a candidate only if its row is finite and its tile lies in the grid."""
    return all(math.isfinite(v) for v in c) and 0 <= c[0] < pr.GRID and 0 <= c[1] < pr.GRID


def bought(layout):
    """(n_cams, n_guards) the oracle's purchase keeps of a layout at BUDGET."""
    o = pr.po.OracleEnv(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, BUDGET)
    o.set_layout(*layout)
    i = o.info()
    return i["n_cams"], i["n_guards"]


def expect_valid(c):
    """The contract's validity of candidate c on BASE: the oracle's purchase takes it, and it does
    not stand on the guard's start tile."""
    if not oracle_shown(c) or (int(c[0]), int(c[1])) == GUARD_START:
        return False
    return bought(with_cand(BASE, c)) == (len(BASE[1]) + 1, len(BASE[2]))


def layout_of(c):
    """The layout whose plan is variant c's reference: BASE plus c when c is valid, else BASE."""
    return with_cand(BASE, c if c is not None and expect_valid(c) else None)


@functools.lru_cache(maxsize=None)
def planes_of(layout_key):
    """(planes, walls) of a layout from reset, all 40 ticks (field_ref.witness_planes); layout_key:
    "base", ("plus", c) or ("alone", c).  Computed once; callers must not modify it."""
    lay = BASE if layout_key == "base" else (with_cand(BASE, layout_key[1]) if layout_key[0] == "plus"
                                             else alone(layout_key[1]))
    p, walls, _ = fr.witness_planes(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, lay, BUDGET)
    return p, walls


def search(c, prefix=(), horizon=None):
    """plan_ref.oracle_search of BASE plus candidate c after `prefix` actions."""
    return pr.oracle_search(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, with_cand(BASE, c), BUDGET,
                            horizon=horizon, prefix=prefix)


@functools.lru_cache(maxsize=None)
def reference(c, gamma):
    """Variant c (None: the baseline) from reset: dict(valid, ticks -- togo at the start cell, which
    test_plan_place_cpu.py holds to oracle_search's T; togo [R, C] int16; value [R, C] float64,
    action [R, C] int8; planes, walls).  Computed once; callers must not modify it."""
    ok = c is not None and expect_valid(c)
    p, walls = planes_of(("plus", c) if ok else "base")
    togo = fr.field_from_planes(walls, pr.VAULT, p, 0, pr.MAX_STEPS)[0]
    value, action = vr.value_from_planes(walls, pr.VAULT, p, D0, 0, pr.MAX_STEPS, gamma)[:2]
    return {"valid": ok, "ticks": int(togo[pr.START]), "togo": togo, "value": value, "action": action, "planes": p,
            "walls": walls}
