"""A plain Python restatement of the Architect's layout decode, written for the tests.

It follows the reference's greedy scan (networks.py:283-335 and _generate_patrol) one
layout at a time, applies the curriculum filter afterwards as training.py:464-467 does, and
then truncates the lists to the capacities as include/heist.h documents for
heist_architect_decode.  tests/test_decode_ref_cpu.py pins it to the reference's recorded
decodes; tests/test_gpu_decode_batch.py compares the kernel with it."""
import numpy as np

COSTS = {1: 1, 2: 3, 3: 5}  # components/budget.py BUDGET_COSTS: wall, camera, guard
_RING = ((0, 0), (0, 1), (0, 2), (1, 2), (2, 2), (2, 1), (2, 0), (1, 0))


def patrol(row, col, rows, cols):
    """networks.py:324-335: the 8-point ring around (row, col), clamped to the interior."""
    return [(max(1, min(rows - 2, row + dr - 1)), max(1, min(cols - 2, col + dc - 1))) for dr, dc in _RING]


def scan(asset_map, cam_params, budget):
    """The greedy row-major scan alone.  asset_map [R, C] classes (0 none, 1 wall, 2 camera,
    3 guard); cam_params = (fov, speed, heading), taken as float32 and widened (the reference
    reads them with .item()).  Returns (walls, cameras, guards) in the reference's list / dict
    form, everything the budget bought."""
    amap = np.asarray(asset_map)
    rows, cols = amap.shape
    fov, speed, heading = (float(np.float32(v)) for v in cam_params)
    walls, cams, guards = [], [], []
    remaining = int(budget)
    for r in range(1, rows - 1):
        for c in range(1, cols - 1):
            kind = int(amap[r, c])
            if kind == 0:
                continue
            if kind == 1 and remaining >= COSTS[1]:
                walls.append((r, c))
                remaining -= COSTS[1]
            elif kind == 2 and remaining >= COSTS[2]:
                cams.append({"row": r, "col": c, "fov_angle": fov, "rotation_speed": speed, "heading": heading,
                             "vision_range": 6})
                remaining -= COSTS[2]
            elif kind == 3 and remaining >= COSTS[3]:
                guards.append({"patrol_path": patrol(r, c, rows, cols), "speed": 1, "vision_range": 4,
                               "fov_angle": 90.0})
                remaining -= COSTS[3]
            if remaining <= 0:
                break
        if remaining <= 0:
            break
    return walls, cams, guards


def finish(lists, allow_cams=True, allow_guards=True, max_walls=None, max_cams=None, max_guards=None):
    """The curriculum filter (training.py:464-467), then truncation to the capacities
    (include/heist.h), on scan()'s lists; returns new lists."""
    walls, cams, guards = (list(x) for x in lists)
    if not allow_cams:
        cams = []
    if not allow_guards:
        guards = []
    if max_walls is not None:
        walls = walls[:max_walls]
    if max_cams is not None:
        cams = cams[:max_cams]
    if max_guards is not None:
        guards = guards[:max_guards]
    return walls, cams, guards


def decode(asset_map, cam_params, budget, allow_cams=True, allow_guards=True, max_walls=None, max_cams=None,
           max_guards=None):
    """scan() then finish(): what heist_architect_decode is documented to produce for one layout."""
    return finish(scan(asset_map, cam_params, budget), allow_cams, allow_guards, max_walls, max_cams, max_guards)
