"""Pin the CPU oracle (oracle/heist_oracle.c) against the reference's golden vectors.

The oracle is the checker the GPU path is compared with on the GPU box, so it
must first reproduce the Python reference exactly on every fixture the
reference produced here (tests/golden/make_golden.py).
"""
import numpy as np
import pytest

import golden_data as gd
from oracle import pyoracle as po

STATUS_RESET = 5
OFFCORNER = "env_traces_offcorner.npz"  # start and vault away from the grid corners


def _replay(tr):
    env = po.OracleEnv(tr["R"], tr["C"], tr["max_steps"], tr["start"], tr["vault"], tr["budget"])
    valid = env.set_layout(tr["walls"], tr["cams"], tr["guards"])
    return env, valid


@pytest.mark.parametrize("tr", list(gd.env_traces()) + list(gd.env_traces(OFFCORNER)), ids=lambda t: t["name"])
def test_env_trace_bit_exact(tr):
    env, valid = _replay(tr)
    assert valid == tr["valid"]
    np.testing.assert_array_equal(env.grid(), tr["grid"])
    inf = env.info()
    assert [inf["n_walls"], inf["n_cams"], inf["n_guards"], inf["spent"]] == tr["accepted"]
    for k, op in enumerate(tr["ops"]):
        if op == -1:
            env.reset()
            r, d, st = 0.0, bool(env.info()["done"]), STATUS_RESET
        else:
            r, d, st = env.step(op)
        inf = env.info()
        ctx = "%s op#%d" % (tr["name"], k)
        assert r == tr["reward"][k], ctx  # float64, bit-exact
        assert d == tr["done"][k], ctx
        assert st == tr["status"][k], ctx
        assert (inf["pos_r"], inf["pos_c"]) == tuple(tr["pos"][k]), ctx
        assert inf["tick"] == tr["tick"][k], ctx
        ch, gi, gh = env.headings()
        np.testing.assert_array_equal(ch, tr["cam_h"][k], err_msg=ctx)
        np.testing.assert_array_equal(gi, tr["g_idx"][k], err_msg=ctx)
        np.testing.assert_array_equal(gh, tr["g_h"][k], err_msg=ctx)
        np.testing.assert_array_equal(env.visibility().astype(bool), tr["vis"][k], err_msg=ctx)
        if k < len(tr["state"]):
            s = env.state_tensor()
            assert s.tobytes() == tr["state"][k].tobytes(), ctx


def test_cones_bit_exact():
    n = 0
    for c in gd.cones():
        kind = 1 if c["kind"] == 2 else 0
        got = po.cone(kind, c["walls"], c["row"], c["col"], c["fov"], c["heading"], c["range"])
        np.testing.assert_array_equal(got, c["tiles"], err_msg=str({k: c[k] for k in ("kind", "row", "col", "fov", "heading", "range")}))
        n += 1
    assert n >= 1000


def test_cone_order_fixture_sets_match_oracle():
    """cone_order.npz's ordered lists hold exactly the oracle's visible tiles, each once
    (the order itself is pinned on the GPU by test_cone_order_matches_reference_list)."""
    n = 0
    for c in gd.cone_orders():
        got = po.cone(c["kind"], c["walls"], c["row"], c["col"], c["fov"], c["heading"], c["range"])
        assert len(set(c["order"])) == len(c["order"])
        want = np.zeros((c["R"], c["C"]), bool)
        for r, cc in c["order"]:
            want[r, cc] = True
        np.testing.assert_array_equal(got, want)
        n += 1
    assert n == 600


def test_bfs_matches_reference():
    n = 0
    for c in gd.bfs_cases():
        assert po.bfs(c["grid"], c["start"], c["goal"]) == c["valid"]
        n += 1
    assert n >= 1000


def test_offcorner_fixture_covers_its_cases():
    """What make_env_traces_offcorner asserted when it wrote the file, from the file: every
    vault lane (the float4 lane of channel 2 the vault is patched into) at 20 x 20, lanes 0 and
    3 at 32 x 32, a width that is no multiple of 4, each finishing status in at least two
    traces, the vault reached wherever it can be, and the four same-quad approaches."""
    trs = list(gd.env_traces(OFFCORNER))
    assert 14 <= len(trs) and all(len(t["ops"]) <= 120 for t in trs)
    lanes = lambda R: {(t["vault"][0] * t["C"] + t["vault"][1]) & 3 for t in trs  # noqa: E731
                       if (t["R"], t["C"]) == (R, R) and t["valid"] and t["start"] != t["vault"]}
    assert lanes(20) == {0, 1, 2, 3} and {0, 3} <= lanes(32)
    assert {(13, 17), (16, 20)} <= {(t["R"], t["C"]) for t in trs}
    for t in trs:
        assert t["start"] != (1, 1) and t["vault"] != (t["R"] - 2, t["C"] - 2), t["name"]
    for code in (1, 2, 3):  # detected, vault_reached, timeout
        assert sum(bool((t["status"] == code).any()) for t in trs) >= 2, po.STATUS_NAMES[code]
    short = [t for t in trs if t["max_steps"] <= 30]
    assert len(short) == 2
    for t in trs:
        if t["valid"] and t["start"] != t["vault"] and t["max_steps"] > 30:
            assert (t["status"] == 2).any(), t["name"]
    quad = [t for t in trs if t["name"].startswith("quad_from_")]
    steps = set()
    for t in quad:  # the first op walks onto the vault from a neighbouring cell
        assert t["status"][1] == 2 and tuple(t["pos"][1]) == t["vault"], t["name"]
        steps.add((t["vault"][0] - t["start"][0], t["vault"][1] - t["start"][1]))
    assert steps == {(0, 1), (0, -1), (1, 0), (-1, 0)}
    assert len({(t["vault"][0] * t["C"] + t["vault"][1]) & 3 for t in quad}) == 4
    names = {t["name"] for t in trs}
    assert {"start_is_vault", "vault_on_border", "start_at_origin", "placement_lists"} <= names


def test_bfs_edges_match_reference():
    """bfs_edges.npz: grids up to 64 x 64 and down to 3 wide, endpoints in the last row or
    column and on wall tiles, grid-filling corridors and their plugged twins."""
    cases = list(gd.bfs_cases("bfs_edges.npz"))
    for c in cases:
        assert po.bfs(c["grid"], c["start"], c["goal"]) == c["valid"], (c["grid"].shape, c["start"], c["goal"])
    share = np.mean([c["valid"] for c in cases])
    assert len(cases) >= 190 and 0.25 <= share <= 0.75
    assert {c["grid"].shape for c in cases} == {(64, 64), (3, 64), (64, 3), (33, 64)}
    assert any(63 in c["start"] or 63 in c["goal"] for c in cases)


def test_gae_matches_reference():
    z = gd.load("ppo.npz")
    for i in range(int(z["n_gae"])):
        adv = po.gae(z["gae%d_r" % i], z["gae%d_v" % i], z["gae%d_d" % i])
        np.testing.assert_allclose(adv, z["gae%d_adv" % i], rtol=0, atol=1e-5)


def test_ppo_loss_matches_reference():
    z = gd.load("ppo.npz")
    for i in range(int(z["n_loss"])):
        g = lambda k: z["loss%d_%s" % (i, k)]  # noqa: E731
        parts, dl, dv = po.ppo_loss(g("logits"), g("values"), g("actions"), g("old"), g("adv"), g("ret"))
        assert abs(parts[1] - float(g("pg"))) < 1e-4
        assert abs(parts[2] - float(g("vl"))) < 1e-4
        assert abs(parts[3] - float(g("ent"))) < 1e-4
        np.testing.assert_allclose(dl, g("dlogits"), rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(dv, g("dvalues"), rtol=1e-4, atol=1e-6)


def test_reference_kats():
    kat = gd.load_json("kat.json")
    env = po.OracleEnv(10, 10, 200, (1, 1), (8, 8), 15)
    s = kat["sanity"]
    assert env.set_layout([(3, 3), (3, 4), (3, 5)],
                          [{"row": 5, "col": 5, "fov_angle": 60, "heading": 0, "rotation_speed": 15, "vision_range": 4}],
                          [{"patrol_path": [(7, 2), (7, 3), (7, 4), (7, 5)], "speed": 1, "vision_range": 3,
                            "fov_angle": 90}]) == s["valid"]
    env.reset()
    rews = []
    for _ in range(5):
        r, d, st = env.step(4)
        rews.append(r)
        if d:
            break
    assert rews == s["rewards"]
    assert po.STATUS_NAMES[st] == s["status"]
    assert int(env.visibility().sum()) == s["surveilled"]
    env = po.OracleEnv(10, 10)
    env.set_layout([], [], [])
    env.reset()
    tot = 0.0
    for _ in range(7):
        tot += env.step(2)[0]
    assert tot == kat["fixes_down"]
    for _ in range(7):
        r, d, st = env.step(4)
        tot += r
        if d:
            break
    assert tot == kat["fixes_right"] and po.STATUS_NAMES[st] == kat["fixes_status"]
    env.reset()
    st = env.state_tensor()
    assert float(st[2].min()) == kat["pos_channel_min"] and float(st[2].max()) == kat["pos_channel_max"]
