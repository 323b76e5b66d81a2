"""Reference for heist_plan_masked (HeistEnv.plan_masked): the planner's answers with some emitters
switched off, without the kernel under test and without any notion of a mask.

A variant's reference is the layout with the switched-off emitters REMOVED FROM ITS LISTS, handed to
what the other planner tests already trust: plan_ref.oracle_search (the C oracle expanded level by
level) for the fewest ticks, field_ref.witness_planes for the visibility of every tick, and
field_ref.field_from_planes / value_ref.value_from_planes on those planes for the tables.

The oracle's purchase drops what the budget does not cover without saying so (wall 1, camera 3,
guard 5): the fixtures below need BUDGET = 20 (seven walls, three cameras: 16; seven walls, two
cameras and a guard: 18).  At plan_ref's 15 the third camera would silently disappear.

FIXTURES: the plan_ref 10 x 10 set-up (start (1, 1), vault (8, 8), max_steps 40, WALLROW, cam(),
GUARD).  TICKS pins the fewest ticks of every variant the tests use, measured with oracle_search.
"""
import functools

import numpy as np

import field_ref as fr
import plan_ref as pr
import value_ref as vr

BUDGET = 20
D0 = abs(pr.START[0] - pr.VAULT[0]) + abs(pr.START[1] - pr.VAULT[1])


def cam_at(col, heading, speed, row=6):
    return dict(pr.cam(heading, speed), row=row, col=col)


# name -> layout (walls, cameras, guards)
FIXTURES = {
    "cam_guard": (pr.WALLROW, [pr.cam(270, 30)], [pr.GUARD]),
    "fixed_cam": (pr.WALLROW, [pr.cam(90, 0)], []),
    "two_fixed": (pr.WALLROW, [pr.cam(90, 0), cam_at(5, 90, 0, row=7)], []),
    "three_same": (pr.WALLROW, [cam_at(3, 270, 30), cam_at(5, 270, 30), cam_at(7, 270, 30)], []),  # one direction group
    "two_cams_guard": (pr.WALLROW, [cam_at(3, 270, 30), cam_at(5, 270, 30)], [pr.GUARD]),
}

# name -> {(cameras on, guards on): fewest ticks}; a key holds one 0/1 per emitter of the layout
TICKS = {
    "cam_guard": {((1,), (1,)): 22, ((0,), (1,)): 16, ((1,), (0,)): 18, ((0,), (0,)): 14},
    "fixed_cam": {((1,), ()): -1, ((0,), ()): 14},                      # the camera is critical
    "two_fixed": {((1, 1), ()): -1, ((0, 1), ()): -1, ((1, 0), ()): -1, ((0, 0), ()): 14},  # jointly blocking
    "three_same": {((1, 1, 1), ()): 22, ((0, 1, 1), ()): 18, ((1, 0, 1), ()): 21, ((1, 1, 0), ()): 21,
                   ((0, 0, 0), ()): 14},
    "two_cams_guard": {((1, 1), (1,)): 32, ((0, 1), (1,)): 22, ((1, 0), (1,)): 20, ((1, 1), (0,)): 21},
}


def variants(name):
    """The (cameras on, guards on) keys of a fixture, the all-on variant first."""
    return list(TICKS[name])


def reduced(layout, on):
    """The layout without the emitters whose flag in on = (cameras on, guards on) is 0."""
    walls, cams, guards = layout
    con, gon = on
    assert len(con) == len(cams) and len(gon) == len(guards)
    return (walls, [c for c, k in zip(cams, con) if k], [g for g, k in zip(guards, gon) if k])


def mask_word(on, max_cams, garbage=0):
    """The variant's emitter_mask word as a Python int in int64's range: camera j is bit j, guard g
    bit max_cams + g.  garbage: bits ORed in at the slots the layout does not fill and from
    max_cams + max_guards up (the caller passes only such bits)."""
    con, gon = on
    w = garbage
    for j, k in enumerate(con):
        w |= int(k) << j
    for g, k in enumerate(gon):
        w |= int(k) << (max_cams + g)
    w &= (1 << 64) - 1
    return w - (1 << 64) if w >> 63 else w


def search(name, on, prefix=(), horizon=None):
    """plan_ref.oracle_search of the reduced layout after `prefix` actions: (T, plan, reach, planes)."""
    return pr.oracle_search(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, reduced(FIXTURES[name], on), BUDGET,
                            horizon=horizon, prefix=prefix)


@functools.lru_cache(maxsize=None)
def planes(name, on):
    """(planes, walls) of the reduced layout from reset, all 40 ticks (field_ref.witness_planes).
    Computed once; callers must not modify it."""
    p, walls, _ = fr.witness_planes(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, reduced(FIXTURES[name], on),
                                    BUDGET)
    return p, walls


@functools.lru_cache(maxsize=None)
def reference(name, on, gamma):
    """The variant from reset: dict(ticks -- oracle_search's T, from TICKS where the variant is
    pinned there (test_plan_masked_cpu.py holds the table to the search); togo [R, C] int16 --
    field_from_planes on the witness planes; value [R, C] float64, action [R, C] int8 --
    value_from_planes on them; planes, walls).  Computed once; callers must not modify it."""
    p, walls = planes(name, on)
    T = TICKS[name][on] if on in TICKS[name] else search(name, on)[0]
    togo = fr.field_from_planes(walls, pr.VAULT, p, 0, pr.MAX_STEPS)[0]
    assert int(togo[pr.START]) == T, "the recurrence and the oracle search disagree"
    value, action = vr.value_from_planes(walls, pr.VAULT, p, D0, 0, pr.MAX_STEPS, gamma)[:2]
    return {"ticks": T, "togo": togo, "value": value, "action": action, "planes": p, "walls": walls}


def filled_flags(n_cams, n_guards, max_cams, max_guards):
    """[N, max_cams + max_guards] bool in NumPy: the env fills the slot."""
    j = np.arange(max_cams + max_guards)[None, :]
    nc, ng = np.asarray(n_cams)[:, None], np.asarray(n_guards)[:, None]
    return np.where(j < max_cams, j < nc, j - max_cams < ng)
