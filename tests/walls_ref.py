"""Reference for heist_plan_walls (HeistEnv.plan_walls): the planner's answers with walls added or
removed, without the kernel under test and without any notion of an edit.

A variant's reference is the layout with its WALL LIST EDITED -- the removed tiles dropped, the added
ones appended -- handed to what the other planner tests already trust (masked_ref.py's method):
plan_ref.oracle_search (the C oracle expanded level by level) for the fewest ticks,
field_ref.witness_planes for the visibility of every tick, and field_ref.field_from_planes /
value_ref.value_from_planes on those planes for the tables.  `level` is a NumPy flood over the
oracle's own wall plane from the start tile to the vault.

FIXTURES: two of masked_ref's 10 x 10 layouts at its budget of 20 (seven walls, a camera and a guard:
15; every edited layout below stays under it).  TABLE pins every edit the tests use: the fewest
ticks from oracle_search and the optimal return at the start cell (gamma 1) from the witness
planes, as measured with the C oracle.
"""
import functools

import numpy as np

import field_ref as fr
import masked_ref as mr
import plan_ref as pr
import value_ref as vr

BUDGET = mr.BUDGET
D0 = mr.D0
ADD, REMOVE = 1, 2

FIXTURES = {name: mr.FIXTURES[name] for name in ("cam_guard", "fixed_cam")}

# name -> (ticks, value at the start cell) of the layout as built
BUILT = {"cam_guard": (22, 11.940000000000001), "fixed_cam": (-1, 0.5714285714285716)}


def add(r, c):
    return ((r, c, ADD),)


def rem(r, c):
    return ((r, c, REMOVE),)


# name -> [(edits, ticks, value at the start cell, level)]; an edit is (row, col, op)
TABLE = {
    "cam_guard": [
        ((), 22, 11.940000000000001, 1),
        (add(6, 6), 22, 12.809999999999995, 1),           # this wall helps the Solver
        (add(7, 5), 24, 12.09, 1),                        # slower and richer
        (add(6, 4), 22, 11.89, 1),
        (add(5, 3), 22, 11.940000000000001, 1),           # redundant
        (add(6, 3), 22, 11.940000000000001, 1),
        (add(7, 7), 22, 11.940000000000001, 1),
        (add(5, 5), -1, 1.7857142857142878, 0),           # the level is BFS-invalid
        (add(3, 5), -1, 1.7857142857142878, 0),
        (rem(4, 1), 22, 11.940000000000001, 1),
        (rem(4, 2), 20, 12.09, 1),
        (rem(4, 3), 19, 12.19, 1),
    ],
    "fixed_cam": [
        ((), -1, 0.5714285714285716, 1),                  # BFS-valid, never clean
        (rem(4, 1), 14, 15.899999999999995, 1),           # each is a critical wall
        (rem(4, 2), 14, 15.899999999999995, 1),
        (rem(4, 3), 14, 15.899999999999995, 1),
        (rem(4, 4), -1, 0.3285714285714293, 1),           # taking a wall away hurts: it was shielding
        (rem(4, 6), -1, 0.5714285714285716, 1),
        (rem(4, 7), -1, 0.5714285714285716, 1),
        (rem(4, 8), -1, 0.5714285714285716, 1),
    ],
}


def rows(name):
    """The fixture's TABLE rows, the layout as built first."""
    return TABLE[name]


def edited(layout, edits):
    """The layout with its wall list edited: the removed tiles dropped, the added ones appended."""
    walls, cams, guards = layout
    gone = {(r, c) for r, c, op in edits if op == REMOVE}
    assert gone <= set(walls), "a removed tile is not in the wall list"
    more = [(r, c) for r, c, op in edits if op == ADD]
    assert not set(more) & set(walls), "an added tile is in the wall list"
    return ([w for w in walls if w not in gone] + more, cams, guards)


def flood(walls, start, goal):
    """1 iff a 4-neighbour path of non-wall tiles joins start and goal (utils.py:52-85 in NumPy)."""
    walls = np.asarray(walls, bool)
    reach = np.zeros(walls.shape, bool)
    reach[start] = True
    while True:
        nxt = reach.copy()
        nxt[1:, :] |= reach[:-1, :]
        nxt[:-1, :] |= reach[1:, :]
        nxt[:, 1:] |= reach[:, :-1]
        nxt[:, :-1] |= reach[:, 1:]
        nxt &= ~walls
        nxt[start] = True
        if nxt[goal]:
            return 1
        if (nxt == reach).all():
            return 0
        reach = nxt


def search(name, edits, prefix=(), horizon=None):
    """plan_ref.oracle_search of the edited layout after `prefix` actions: (T, plan, reach, planes)."""
    return pr.oracle_search(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, edited(FIXTURES[name], edits), BUDGET,
                            horizon=horizon, prefix=prefix)


@functools.lru_cache(maxsize=None)
def planes(name, edits):
    """(planes, walls) of the edited layout from reset, all 40 ticks (field_ref.witness_planes).
    Computed once; callers must not modify it."""
    p, walls, _ = fr.witness_planes(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, edited(FIXTURES[name], edits),
                                    BUDGET)
    return p, walls


@functools.lru_cache(maxsize=None)
def ticks(name, edits):
    """oracle_search's fewest ticks of the edited layout.  Computed once."""
    return search(name, edits)[0]


@functools.lru_cache(maxsize=None)
def reference(name, edits, gamma):
    """The variant from reset: dict(ticks -- oracle_search's T; togo [R, C] int16 -- field_from_planes on
    the witness planes; value [R, C] float64, action [R, C] int8 -- value_from_planes on them; level --
    the flood on the oracle's wall plane; planes, walls).  Computed once; callers must not modify it."""
    p, walls = planes(name, edits)
    T = ticks(name, edits)
    togo = fr.field_from_planes(walls, pr.VAULT, p, 0, pr.MAX_STEPS)[0]
    assert int(togo[pr.START]) == T, "the recurrence and the oracle search disagree"
    value, action = vr.value_from_planes(walls, pr.VAULT, p, D0, 0, pr.MAX_STEPS, gamma)[:2]
    return {"ticks": T, "togo": togo, "value": value, "action": action, "planes": p, "walls": walls,
            "level": flood(walls, pr.START, pr.VAULT)}


def edit_rows(edits, E):
    """A variant's edits as E rows (row, col, op), op 0 beyond the variant's own."""
    assert len(edits) <= E
    return [list(e) for e in edits] + [[0, 0, 0]] * (E - len(edits))


# ---- synthetic shapes for the twin-handle tests (no oracle: the twin is the yardstick there)

# name -> (R, C, max_steps, cameras, guards, budget); the budget's rest is walls, and a twin gets 8 more
SHAPES = {"10x13": (10, 13, 40, 2, 1, 21), "20x20": (20, 20, 60, 5, 3, 46), "32x32": (32, 32, 80, 5, 3, 52)}
SLACK = 8


def cpu_grid(R, C, start, vault, layout):
    """heist_set_layout's tile grid of a layout whose every asset is bought, in NumPy: 0 EMPTY, 1 WALL,
    2 START, 3 VAULT, 4 CAMERA, 5 GUARD (a guard's start tile, placed without a check)."""
    g = np.zeros((R, C), np.int8)
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = 1
    g[tuple(start)], g[tuple(vault)] = 2, 3
    walls, cams, guards = layout
    for r, c in walls:
        if 0 < r < R - 1 and 0 < c < C - 1 and g[r, c] == 0:
            g[r, c] = 1
    for cm in cams:
        if g[cm["row"], cm["col"]] == 0:
            g[cm["row"], cm["col"]] = 4
    for gd in guards:
        r, c = gd["patrol_path"][0]
        g[min(max(r, 0), R - 1), min(max(c, 0), C - 1)] = 5
    return g


def _line_tiles(a, b):
    """The tiles strictly between a and b on the straight segment, nearest to a first."""
    n = max(abs(b[0] - a[0]), abs(b[1] - a[1]))
    out = []
    for k in range(1, n):
        t = (int(round(a[0] + (b[0] - a[0]) * k / n)), int(round(a[1] + (b[1] - a[1]) * k / n)))
        if t not in out and t != tuple(a) and t != tuple(b):
            out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """Two synthetic layouts of the shape and four variants of each, every one valid with the level
    still valid (checked here on the CPU grid): dict(layouts, grids, edits [2][4] -- tuples of (row, col,
    op) --, E = 8).  Variant 0: one add.  Variant 1: an add and a remove.  Variant 2: eight edits, adds
    and removes mixed.  Variant 3: env 0 -- a wall on a later patrol point of guard 0; env 1 -- a wall
    directly between a camera (the first that has such a tile) and the vault.  A wall under a guard's start tile is left out of the
    lists, as in test_gpu_plan_masked.shape_layouts."""
    from heist_amd.layouts import synthetic_layout
    R, C, _, nc, ng, budget = SHAPES[name]
    start, vault = (1, 1), (R - 2, C - 2)
    rng = np.random.Generator(np.random.PCG64(1000 * R + C))
    lays, grids, edits = [], [], []
    for e in range(2):
        walls, cams, guards = synthetic_layout(rng, R, C, budget, n_cams=nc, n_guards=ng)
        walls = [w for w in walls if w not in {g["patrol_path"][0] for g in guards}]
        if e == 1:
            guards[0] = dict(guards[0], vision_range=8)  # off the cone cache: raycast live on every handle
        lay = (walls, cams, guards)
        g = cpu_grid(R, C, start, vault, lay)

        def ok(ed, g=g):
            """Every edit holds on g, no tile twice, and the edited level is still valid."""
            tiles = [(r, c) for r, c, _ in ed]
            if len(set(tiles)) != len(tiles):
                return False
            w = g == 1
            for r, c, op in ed:
                if not (0 < r < R - 1 and 0 < c < C - 1) or g[r, c] != (0 if op == ADD else 1) or (r, c) == start:
                    return False
                w = w.copy()
                w[r, c] = op == ADD
            return bool(flood(w, start, vault))

        def draw(n_add, n_rem, g=g, ok=ok):
            empty = [(int(r), int(c)) for r, c in np.argwhere(g == 0)]
            wall = [(int(r), int(c)) for r, c in np.argwhere(g[1:-1, 1:-1] == 1) + 1]
            for _ in range(200):
                a = [empty[i] for i in rng.permutation(len(empty))[:n_add]]
                b = [wall[i] for i in rng.permutation(len(wall))[:n_rem]]
                ed = [(r, c, ADD) for r, c in a] + [(r, c, REMOVE) for r, c in b]
                ed = tuple(ed[i] for i in rng.permutation(len(ed)))
                if ok(ed):
                    return ed
            raise AssertionError("no valid variant found")

        row = [draw(1, 0), draw(1, 1), draw(5, 3)]
        if e == 0:
            pts = [p for gd in guards[:1] for p in gd["patrol_path"][1:] if p != gd["patrol_path"][0]]
        else:
            pts = [t for cm in cams for t in _line_tiles((cm["row"], cm["col"]), vault)]
        special = [((r, c, ADD),) for r, c in pts if ok(((r, c, ADD),))]
        assert special, "%s env %d: no special tile" % (name, e)
        row.append(special[0])
        lays.append(lay)
        grids.append(g)
        edits.append(row)
    return {"layouts": lays, "grids": grids, "edits": edits, "E": 8, "start": start, "vault": vault}
