"""References for heist_plan (HeistEnv.plan): the fewest undetected ticks to the vault.

Two independent ones, neither using the kernel under test:

* plan_from_planes: the recurrence of include/heist.h in NumPy, on boolean [R, C] planes, given
  the visibility plane of every tick, and backtrack, the canonical plan from its reach sets.
* oracle_search: no planes and no recurrence -- a level-by-level expansion of the C oracle
  (oracle.pyoracle.OracleEnv, the reference's HeistEnvironment restated).  OracleEnv has no
  clone, and reset alone keeps the camera headings, so every (cell, action) is replayed from
  scratch: set_layout + reset + the prefix + the cell's stored path + the action.  A cell's path
  is the first one found; which one does not matter, since what follows depends on the solver's
  cell and the tick alone.

CASES: the 10 x 10 fixtures (start (1, 1), vault (8, 8), max_steps 40) with the plan lengths,
canonical plans and reach-set sizes measured with the oracle search.
"""
import numpy as np

from oracle import pyoracle as po

DELTA = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))  # WAIT, UP, DOWN, LEFT, RIGHT (environment.py:239-246)


def candidates(reach, walls):
    """reach and its four one-cell shifts inside the grid, minus wall cells (a blocked move is a
    stay, which the union covers)."""
    c = reach.copy()
    c[1:, :] |= reach[:-1, :]
    c[:-1, :] |= reach[1:, :]
    c[:, 1:] |= reach[:, :-1]
    c[:, :-1] |= reach[:, 1:]
    return c & ~walls


def plan_from_planes(walls, pos, vault, planes, tick0=0, max_steps=200, done=False):
    """(T, reach) with reach[k] the bool [R, C] set after k ticks (reach[0] the start), for the
    ticks planes[0], planes[1], ... gives the visibility of (tick k uses planes[k - 1]); the
    lists stop at T, when the set empties, or when the planes run out."""
    r0 = np.zeros(walls.shape, bool)
    if not done:
        r0[pos] = True
    reach = [r0]
    for k in range(1, len(planes) + 1):
        if not reach[-1].any():
            break
        live = candidates(reach[-1], walls) & ~np.asarray(planes[k - 1], bool)
        if live[vault]:
            return k, reach
        live[vault] = False
        if tick0 + k >= max_steps:
            live[:] = False
        reach.append(live)
    return -1, reach


def backtrack(reach, T, vault):
    """The canonical plan: from x_T = vault, a_k is the lowest action with x_k - delta(a_k) in
    reach[k - 1]."""
    if T <= 0:
        return []
    R, C = reach[0].shape
    x, plan = tuple(vault), []
    for k in range(T, 0, -1):
        for a, (dr, dc) in enumerate(DELTA):
            p = (x[0] - dr, x[1] - dc)
            if 0 <= p[0] < R and 0 <= p[1] < C and reach[k - 1][p]:
                plan.append(a)
                x = p
                break
        else:
            raise AssertionError("no predecessor of %s at tick %d" % (x, k))
    return plan[::-1]


def oracle_search(R, C, max_steps, start, vault, layout, budget, horizon=None, prefix=()):
    """(T, plan, reach, planes) by expanding OracleEnv level by level after `prefix` actions:
    reach[k] as in plan_from_planes, planes[k - 1] the oracle's visibility on tick k (the same
    for every replay of that tick: the emitters do not depend on the solver)."""
    prefix = tuple(int(a) for a in prefix)

    def replay(path):
        o = po.OracleEnv(R, C, max_steps, start, vault, budget)
        o.set_layout(*layout)
        o.reset()
        for a in prefix + path:
            o.step(a)
        return o

    inf = replay(()).info()
    horizon = max_steps if horizon is None else horizon
    horizon = min(horizon, max_steps - inf["tick"])
    frontier = {} if inf["done"] else {(inf["pos_r"], inf["pos_c"]): ()}

    def mask(cells):
        m = np.zeros((R, C), bool)
        for c in cells:
            m[c] = True
        return m

    reach, planes, T = [mask(frontier)], [], -1
    for k in range(1, horizon + 1):
        if not frontier:
            break
        nxt, hit, plane = {}, False, None
        for cell in sorted(frontier):
            for a in range(5):
                o = replay(frontier[cell] + (a,))
                i = o.info()
                assert i["tick"] == inf["tick"] + k
                if plane is None:
                    plane = o.visibility().astype(bool)
                if i["vault_reached"] and not i["detected"]:
                    hit = True
                if not i["done"]:
                    nxt.setdefault((i["pos_r"], i["pos_c"]), frontier[cell] + (a,))
        planes.append(plane)
        if hit:
            T = k
            break
        reach.append(mask(nxt))
        frontier = nxt
    return T, backtrack(reach, T, vault), reach, planes


# ---- the 10 x 10 fixtures

GRID, START, VAULT, MAX_STEPS, BUDGET = 10, (1, 1), (8, 8), 40, 15
WALLROW = [(4, c) for c in range(1, 9) if c != 5]


def cam(heading, speed):
    return {"row": 6, "col": 5, "fov_angle": 60.0, "vision_range": 6, "heading": float(heading),
            "rotation_speed": float(speed)}


GUARD = {"patrol_path": [(5, c) for c in range(2, 8)], "speed": 1, "vision_range": 4, "fov_angle": 90.0}

# name -> (layout, start, T, canonical plan)
CASES = {
    "empty": (([], [], []), START, 14, [4] * 7 + [2] * 7),
    "wallrow_cam": ((WALLROW, [cam(270, 30)], []), START, 18, [4, 4, 2, 2, 0, 0, 0, 4, 4, 2, 2, 2, 0, 2, 2, 4, 4, 4]),
    "wallrow_guard": ((WALLROW, [], [GUARD]), START, 16, [4, 4, 4, 4, 2, 2, 0, 0, 2, 2, 2, 2, 2, 4, 4, 4]),
    "wallrow_both": ((WALLROW, [cam(270, 30)], [GUARD]), START, 22,
                     [4, 4, 2, 2, 0, 0, 0, 4, 4, 0, 0, 0, 0, 0, 2, 2, 2, 2, 2, 4, 4, 4]),
    "wallrow_fixed_cam": ((WALLROW, [cam(90, 0)], []), START, -1, []),       # BFS-valid, never clean
    "full_wallrow": (([(4, c) for c in range(1, 9)], [], []), START, -1, []),  # BFS-invalid
    "start_on_vault": (([], [], []), VAULT, 1, [0]),
}
# |reach_k| of wallrow_both for k = 0 .. 21
BOTH_SIZES = [1, 3, 6, 9, 12, 12, 9, 9, 12, 15, 19, 23, 29, 24, 22, 25, 26, 20, 20, 22, 28, 33]
