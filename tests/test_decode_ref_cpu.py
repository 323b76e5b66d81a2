"""tests/decode_ref.py (the reference the batched GPU decode test compares against) pinned to
the reference's own recordings: every decode case of nets.npz / architect_decode.json."""
import numpy as np

import decode_ref
import golden_data as gd


def _cases():
    z = gd.load("nets.npz")
    dec = gd.load_json("architect_decode.json")
    assert len(dec) == len(z["dec_meta"]) > 0
    cur = 0
    for (R, C, budget, nw, nc, ng), case in zip(z["dec_meta"], dec):
        R, C = int(R), int(C)
        yield z["dec_maps"][cur:cur + R * C].reshape(R, C), int(budget), (int(nw), int(nc), int(ng)), case
        cur += R * C
    assert cur == len(z["dec_maps"])


def test_decode_ref_reproduces_every_recorded_case():
    n = 0
    for amap, budget, counts, case in _cases():
        fov, speed, heading = case["cam_params"]
        walls, cams, guards = decode_ref.decode(amap, (fov, speed, heading), budget)
        assert (len(walls), len(cams), len(guards)) == counts
        assert [list(w) for w in walls] == case["walls"]
        assert [[c["row"], c["col"]] for c in cams] == [list(c) for c in case["cams"]]
        for c in cams:  # the recorded .item() values are float32-exact, so they come back unchanged
            assert (c["fov_angle"], c["rotation_speed"], c["heading"], c["vision_range"]) == (fov, speed, heading, 6)
        assert [[list(p) for p in g["patrol_path"]] for g in guards] == case["guards"]
        assert all((g["speed"], g["vision_range"], g["fov_angle"]) == (1, 4, 90.0) for g in guards)
        n += 1
    assert n == 40


def test_decode_ref_filter_and_truncation_apply_after_the_scan():
    """The curriculum filter drops lists the scan already paid for (training.py:464-467), and
    a capacity cuts a list without giving its budget back."""
    amap = np.zeros((6, 6), np.int64)
    amap[1, 1:5] = (3, 2, 1, 1)  # guard 5, camera 3, two walls: 10 of a budget of 10
    amap[2, 1] = 1  # never reached
    cam = (60.0, 10.0, 45.0)
    w, c, g = decode_ref.decode(amap, cam, 10)
    assert (w, len(c), len(g)) == ([(1, 3), (1, 4)], 1, 1)
    w, c, g = decode_ref.decode(amap, cam, 10, allow_cams=False, allow_guards=False)
    assert (w, c, g) == ([(1, 3), (1, 4)], [], [])  # the walls are still the two the rest of the budget bought
    w, c, g = decode_ref.decode(amap, cam, 10, max_walls=1, max_cams=0, max_guards=0)
    assert (w, c, g) == ([(1, 3)], [], [])
    # too poor for the guard (budget 4): it is skipped and the scan goes on to the camera and a wall
    w, c, g = decode_ref.decode(amap, cam, 4)
    assert (w, [(k["row"], k["col"]) for k in c], g) == ([(1, 3)], [(1, 2)], [])
    assert decode_ref.decode(amap, cam, 0) == ([], [], [])
    assert decode_ref.patrol(1, 1, 6, 6) == [(1, 1), (1, 1), (1, 2), (1, 2), (2, 2), (2, 1), (2, 1), (1, 1)]
