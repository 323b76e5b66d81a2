"""GPU parity of the environment path with the start and the vault away from the grid corners.

Every other environment test runs the solver from (1, 1) to (R-2, C-2).  There the vault sits in
lane 2 of its float4 of observation channel 2 at every grid size, its right-hand neighbour is the
border wall, and a row/column interchange of either position changes nothing.  Here the start and
vault positions (EnvironmentConfig.start_pos / vault_pos, heist_create's start_r, start_c,
vault_r, vault_c) take every vault lane, asymmetric rows and columns, the same float4 as the
solver, the border ring, (0, 0) and each other's cell.

Bar: bit-exact, against the reference's recorded traces (tests/golden/env_traces_offcorner.npz,
bfs_edges.npz) and against the C oracle (pinned to both files by tests/test_oracle_golden.py).
Actions are steered towards the vault (golden_data.steered_action) from the oracle's positions:
uniform actions almost never end on a vault that is not next to the start.
"""
import numpy as np
import pytest
import torch

import env_parity as ep
import golden_data as gd
from oracle import pyoracle as po
from heist_amd import EnvironmentConfig, EnvState, HeistEnv
from heist_amd import _native as nat
from heist_amd.layouts import synthetic_layout
from heist_amd.obs_compact import CompactObs

pytestmark = pytest.mark.gpu

TRACES = list(gd.env_traces(ep.OFFCORNER_FILE))
GRIDS = list(ep.OFFCORNER)
N = 64


def _handle(monkeypatch, knobs, *args, **kw):
    """A HeistEnv created under the HEIST_* knobs (read at heist_create)."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    try:
        return HeistEnv(*args, **kw)
    finally:
        for k in knobs:
            monkeypatch.delenv(k)


def _cfg(R, C, start, vault, budget, max_steps=ep.OFFCORNER_MAX_STEPS):
    return EnvironmentConfig(grid_rows=R, grid_cols=C, max_steps=max_steps, start_pos=start, vault_pos=vault,
                             architect_budget=budget)


def _caps(budget):
    return dict(max_cams=max(1, budget // 3), max_guards=max(1, budget // 5), max_path=16)


def _assert_rows(name, ctx, got, want):
    """got: (obs, reward64, done, status) device tensors of one tick, want: the oracle's arrays."""
    obs, r64, done, status = (x.cpu().numpy() for x in got)
    w_obs, w_r, w_d, w_s = want
    for what, a, b in (("reward64", r64, w_r), ("done", done.astype(bool), w_d), ("status", status, w_s)):
        if not np.array_equal(a, b):
            i = int(np.nonzero(a != b)[0][0])
            raise AssertionError("%s %s: %s of env %d is %r, the oracle's %r" % (name, ctx, what, i, a[i], b[i]))
    if not ep.same_bits(obs, w_obs):
        bad = np.nonzero((obs.view(np.int32) != w_obs.view(np.int32)).reshape(len(obs), -1).any(1))[0]
        i = int(bad[0])
        ch, r, c = (int(x[0]) for x in np.nonzero(obs[i].view(np.int32) != w_obs[i].view(np.int32)))
        raise AssertionError("%s %s: observation of env %d (of %d envs) differs first at channel %d cell (%d, %d): "
                             "%r, the oracle's %r" % (name, ctx, i, len(bad), ch, r, c, obs[i, ch, r, c],
                                                     w_obs[i, ch, r, c]))


# -- a. the reference's traces ---------------------------------------------------------------------
def test_fixture_is_the_one_the_cpu_suite_pins():
    assert len(TRACES) >= 14 and {(t["vault"][0] * t["C"] + t["vault"][1]) & 3 for t in TRACES} == {0, 1, 2, 3}
    assert all(t["start"] != (1, 1) and t["vault"] != (t["R"] - 2, t["C"] - 2) for t in TRACES)


@pytest.mark.parametrize("path", ["step_kernel", "lean_k1"])
@pytest.mark.parametrize("cones", [True, False], ids=["guard_cones", "live_guards"])
@pytest.mark.parametrize("tr", TRACES, ids=lambda t: t["name"])
def test_golden_trace_bit_exact(tr, cones, path, gpu_device, monkeypatch):
    """test_gpu_env.py's golden-trace body on every off-corner trace, both single-tick routes,
    guard cones cached and live."""
    ep.check_golden_trace(tr, cones, path, gpu_device, monkeypatch)


@pytest.mark.parametrize("tr", TRACES, ids=lambda t: t["name"])
def test_single_env_class_matches_golden_trace(tr, gpu_device):
    ep.check_single_env_class_trace(tr, gpu_device)


# -- b. batched single ticks against the oracle, every observation-write form -------------------------
def _step_forms(R, C):
    """name -> (knobs, expected kernel_config entries): the step kernel's split write
    (write_obs_static / write_obs_dynamic: two or more waves, C % 4 == 0) at 4 and 2 waves per env,
    its one-piece write (write_obs; HEIST_SPLIT_OBS=0, and always at one wave), whose C % 4 != 0
    loop the 13 x 17 grid takes, and the lean kernel's one-tick route where it serves the grid."""
    forms = {
        "split_w4": ({"HEIST_STEP_LEAN": 0, "HEIST_STEP_WAVES": 4}, {"step_waves": 4, "split_obs": 1}),
        "split_w2": ({"HEIST_STEP_LEAN": 0, "HEIST_STEP_WAVES": 2}, {"step_waves": 2, "split_obs": 1}),
        "whole_w4": ({"HEIST_STEP_LEAN": 0, "HEIST_STEP_WAVES": 4, "HEIST_SPLIT_OBS": 0},
                     {"step_waves": 4, "split_obs": 0}),
        "whole_w2": ({"HEIST_STEP_LEAN": 0, "HEIST_STEP_WAVES": 2, "HEIST_SPLIT_OBS": 0},
                     {"step_waves": 2, "split_obs": 0}),
    }
    if (R, C) != (32, 32):  # the one-wave step kernel exists for the small plane gap only
        forms["whole_w1"] = ({"HEIST_STEP_LEAN": 0, "HEIST_STEP_WAVES": 1}, {"step_waves": 1})
    if (R, C) == (20, 20):
        forms["lean_k1"] = ({"HEIST_STEP_LEAN": 1, "HEIST_MULTI_WAVES": 1}, {"step_lean": 1, "lean": 1})
    if (R, C) == (32, 32):
        for w in (1, 2):
            forms["lean_k1_w%d" % w] = ({"HEIST_STEP_LEAN": 1, "HEIST_MULTI_WAVES": 1, "HEIST_LEAN_WAVES": w},
                                        {"step_lean": 1, "lean": 1, "lean_waves": w})
    for knobs, want in forms.values():
        want.setdefault("step_lean", 0)
    return forms


@pytest.mark.parametrize("lane", range(4))
@pytest.mark.parametrize("R,C", GRIDS, ids=lambda v: str(v))
def test_batched_steered_vs_oracle(R, C, lane, gpu_device, monkeypatch):
    """64 envs with auto-reset and max_steps 40, the vault in float4 lane `lane`, actions steered
    from the oracles' positions: every env, every tick, on every form of the observation write,
    gives the oracle's observation bytes, float64 reward, done and status.  Counted on the oracle:
    at least 20 finishes on the vault and 20 detections, and a displayed solver on every cell of
    the vault's float4 that is not the vault."""
    start, vault, lays, budget, T = ep.offcorner_case(R, C, lane, N)
    cfg = _cfg(R, C, start, vault, budget)
    ob = ep.OracleBatch(R, C, cfg.max_steps, start, vault, lays, budget, seed=lane)
    envs = {}
    for name, (knobs, want) in _step_forms(R, C).items():
        env = _handle(monkeypatch, knobs, N, cfg, device=gpu_device, auto_reset=True, **_caps(budget))
        kc = env.kernel_config()
        assert {k: kc[k] for k in want} == want, name
        valid = env.set_layouts(lays, budget=budget).cpu().numpy().astype(bool)
        assert valid.tolist() == ob.valid, name
        assert ep.same_bits(env.reset().cpu().numpy(), ob.obs()), name
        envs[name] = env
    for t in range(T):
        acts = ob.choose()
        want = ob.step(acts)
        a = torch.from_numpy(acts).to(gpu_device)
        for name, env in envs.items():
            obs, _, done, status = env.step(a)
            _assert_rows(name, "tick %d" % t, (obs, env.reward64, done, status), want)
    print("%dx%d lane %d: %d vault finishes, %d detections, %d timeouts, in-quad lanes %s"
          % (R, C, lane, ob.n_vault, ob.n_detected, ob.n_timeout, sorted(ob.quad_offsets)))
    assert ob.n_vault >= 20 and ob.n_detected >= 20
    assert ob.quad_offsets == ep.quad_offsets_allowed(R, C, vault)
    for env in envs.values():
        env.close()


# -- c. step_multi ---------------------------------------------------------------------------------
def _multi_forms(R, C):
    """The lean K-tick kernel at one wave per env (20 x 20) and at one and two (32 x 32), the
    generic K-tick kernel (20 x 20 at two waves, 16 x 20), K single ticks (13 x 17)."""
    if (R, C) == (20, 20):
        return {"lean_w1": ({"HEIST_MULTI_WAVES": 1}, {"lean": 1, "multi_waves": 1}),
                "generic_w2": ({"HEIST_MULTI_WAVES": 2}, {"multi_waves": 2})}
    if (R, C) == (32, 32):
        return {"lean_w%d" % w: ({"HEIST_MULTI_WAVES": 1, "HEIST_LEAN_WAVES": w}, {"lean": 1, "lean_waves": w})
                for w in (1, 2)}
    if (R, C) == (16, 20):
        return {"generic_w%d" % w: ({"HEIST_MULTI_WAVES": w}, {"multi_waves": w}) for w in (1, 2)}
    return {"single_ticks": ({}, {})}


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto_reset", "no_reset"])
@pytest.mark.parametrize("lane", range(4))
@pytest.mark.parametrize("R,C", GRIDS, ids=lambda v: str(v))
def test_step_multi_steered_vs_oracle(R, C, lane, auto_reset, gpu_device, monkeypatch):
    """heist_step_multi, K = 8, against the oracle replay row by row of the [K, N] outputs.  With
    auto-reset some launch has an env that ends on the vault before the last tick: the rows after
    it show the solver back on the off-corner start.  Without it the finished envs are reset()
    between the launches."""
    K = 8
    start, vault, lays, budget, T = ep.offcorner_case(R, C, lane, N)
    cfg = _cfg(R, C, start, vault, budget)
    ob = ep.OracleBatch(R, C, cfg.max_steps, start, vault, lays, budget, seed=10 + lane, auto_reset=auto_reset)
    envs = {}
    for name, (knobs, want) in _multi_forms(R, C).items():
        env = _handle(monkeypatch, knobs, N, cfg, device=gpu_device, auto_reset=auto_reset, **_caps(budget))
        kc = env.kernel_config()
        assert {k: kc[k] for k in want} == want, name
        env.set_layouts(lays, budget=budget)
        assert ep.same_bits(env.reset().cpu().numpy(), ob.obs()), name
        envs[name] = env
    seen_restart = 0
    for it in range(T // K):
        acts, w_obs, w_r, w_d, w_s = ob.rollout(K)
        a = torch.from_numpy(acts).to(gpu_device)
        for name, env in envs.items():
            obs, _, done, status, r64 = env.step_multi(a, auto_reset=auto_reset, reward64=True)
            for k in range(K):
                _assert_rows(name, "launch %d row %d" % (it, k), (obs[k], r64[k], done[k], status[k]),
                             (w_obs[k], w_r[k], w_d[k], w_s[k]))
            if auto_reset and start != vault:
                ks, es = np.nonzero(w_s[:K - 1] == 2)
                for k, e in zip(ks, es):  # the in-kernel reset: the solver's cell is the start again
                    assert float(obs[k, e, 2, start[0], start[1]]) > 0.5, (name, it, k, e)
                    seen_restart += 1
        if not auto_reset:
            m = ob.reset_done()
            if m.any():
                want = ob.obs()
                for name, env in envs.items():
                    got = env.reset(torch.from_numpy(m.astype(np.uint8))).cpu().numpy()
                    assert ep.same_bits(got[m], want[m]), (name, it)  # (step_multi leaves env.obs's other rows alone)
    if auto_reset:
        assert ob.early_vault >= 1 and seen_restart >= 1
    assert ob.n_vault >= 1
    for env in envs.values():
        env.close()


# -- d. layout placement and validity ----------------------------------------------------------------
def crowded_layouts(n, R, C, seed):
    """Layouts made for the corner pair (synthetic_layout's default start (1, 1) and vault
    (R-2, C-2): its walls and cameras may name the real start and vault) plus extra walls on
    0.25 .. 0.45 of the interior cells (0.35 on average; the real start and vault cells and cells
    the layout already names included): about a third cut the start off from the vault."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cells = [(r, c) for r in range(1, R - 1) for c in range(1, C - 1)]
    lays = []
    for _ in range(n):
        walls, cams, guards = synthetic_layout(rng, R, C, 15, start=(1, 1), vault=(R - 2, C - 2))
        k = int(rng.uniform(0.25, 0.45) * len(cells))
        extra = [cells[i] for i in rng.permutation(len(cells))[:k]]
        lays.append((list(walls) + extra, cams, guards))
    return lays


def test_layout_placement_and_validity(gpu_device):
    """heist_set_layout with the off-corner pair on 256 crowded layouts: valid, the exported grid
    (kStart / kVault tiles, assets refused on them) and the accepted counts equal the oracle's."""
    n, R, C, budget = 256, 20, 20, 200
    start, vault = ep.OFFCORNER[(R, C)]["pairs"][3]
    lays = crowded_layouts(n, R, C, seed=41)
    named = sum((start in w) or (vault in w) for w, _, _ in lays)
    assert named >= n // 4  # wall lists that name the start or the vault cell
    cfg = _cfg(R, C, start, vault, budget)
    env = HeistEnv(n, cfg, max_cams=5, max_guards=3, max_path=16, device=gpu_device)
    valid = env.set_layouts(lays, budget=budget).cpu().numpy().astype(bool)
    st = {k: v.cpu().numpy() for k, v in env.export(grid=True).items()}
    want_valid = np.zeros(n, bool)
    for e, lay in enumerate(lays):
        o = po.OracleEnv(R, C, cfg.max_steps, start, vault, budget)
        want_valid[e] = o.set_layout(*lay)
        inf = o.info()
        np.testing.assert_array_equal(st["grid"][e], o.grid(), err_msg="env %d" % e)
        assert [int(st[k][e]) for k in ("n_walls", "n_cams", "n_guards", "spent")] == \
            [inf[k] for k in ("n_walls", "n_cams", "n_guards", "spent")], e
        assert st["grid"][e][start] == 2 or any(g["patrol_path"][0] == start for g in lay[2]), e
    np.testing.assert_array_equal(valid, want_valid)
    share = want_valid.mean()
    print("valid share %.2f" % share)
    assert 0.2 <= share <= 0.8
    env.close()


# -- e. heist_bfs_valid -------------------------------------------------------------------------------
def test_bfs_edges_bit_exact(gpu_device):
    """bfs_edges.npz (64 x 64, 3 x 64, 64 x 3, 33 x 64; endpoints in the last row and column and
    on wall tiles; corridors far longer than 4 (R + C) and their plugged twins), batched per shape
    and endpoints."""
    from heist_amd.utils import bfs_valid_batch
    groups = {}
    for c in gd.bfs_cases("bfs_edges.npz"):
        groups.setdefault((c["grid"].shape, c["start"], c["goal"]), []).append(c)
    n = n_true = 0
    for (shape, start, goal), cs in groups.items():
        g = torch.tensor(np.stack([c["grid"] for c in cs]).astype(np.int32), device=gpu_device)
        got = bfs_valid_batch(g, start, goal).cpu().numpy()
        np.testing.assert_array_equal(got, np.array([c["valid"] for c in cs]), err_msg=str((shape, start, goal)))
        n += len(cs)
        n_true += sum(c["valid"] for c in cs)
    assert n >= 190 and 0.25 * n <= n_true <= 0.75 * n


# -- f. compact observations -------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["left", "right", "above", "below"])
@pytest.mark.parametrize("lane", range(4))
def test_compact_obs_solver_on_the_vault(gpu_device, lane, side):
    """test_solver_on_the_vault's shapes with the vault in every float4 lane and the solver
    walking onto it from each side: before the step (solver next to the vault, in its float4 when
    it comes from the left or right) and after it, expand(pack(obs)) is obs bit for bit, and the
    position word of a solver on the vault holds the vault's position."""
    _, vault = ep.OFFCORNER[(20, 20)]["pairs"][lane]
    dr, dc, action = {"left": (0, -1, 4), "right": (0, 1, 3), "above": (-1, 0, 2), "below": (1, 0, 1)}[side]
    start = (vault[0] + dr, vault[1] + dc)
    n = 4
    env = HeistEnv(n, _cfg(20, 20, start, vault, 15, max_steps=200), device=gpu_device, auto_reset=False)
    env.set_layouts([([], [], [])] * n, budget=15)
    nvis = (400 + 31) // 32
    obs = env.reset()
    assert float(obs[0, 2, start[0], start[1]]) > 0.5 and float(obs[0, 2, vault[0], vault[1]]) == -1.0
    rec = env.pack_obs(obs)
    assert rec[:, nvis].tolist() == [start[0] | start[1] << 8] * n
    assert ep.same_bits(CompactObs.of_env(env, rec).expand().cpu().numpy(), obs.cpu().numpy())
    obs, _, done, status = env.step(torch.full((n,), action, dtype=torch.int64))
    assert bool(done.all()) and status.tolist() == [2] * n
    assert float(obs[:, 2].max()) <= 0.0 and float(obs[0, 2, vault[0], vault[1]]) == -1.0
    o = po.OracleEnv(20, 20, 200, start, vault, 15)
    o.set_layout([], [], [])
    o.reset()
    o.step(action)
    assert ep.same_bits(obs[0].cpu().numpy(), o.state_tensor())
    rec = env.pack_obs(obs)
    assert rec[:, nvis].tolist() == [vault[0] | vault[1] << 8] * n
    assert ep.same_bits(CompactObs.of_env(env, rec).expand().cpu().numpy(), obs.cpu().numpy())
    env.close()


# -- g. state blobs ----------------------------------------------------------------------------------
def test_state_blob_continues_and_is_refused_elsewhere(gpu_device, monkeypatch):
    """20 x 20 on the lean kernel, 16 envs, 30 steered ticks with auto-reset.  (1) save after 12
    ticks, play on, load, play the same 18 ticks again (as K-tick launches), and load into a second
    handle: each continuation equals the uninterrupted run, which equals the oracle.  (2) a handle
    that differs in exactly one of start_r, start_c, vault_r, vault_c refuses the blobs, at the
    container check and, bypassing it, on the device (header words 9..12), and writes nothing.
    tests/test_gpu_env_state.py varies the grid, max_guards and the magic, never these four."""
    n, R, C, lane = 16, 20, 20, 1
    start, vault, lays, budget, _ = ep.offcorner_case(R, C, lane, n)
    cfg = _cfg(R, C, start, vault, budget)
    ob = ep.OracleBatch(R, C, cfg.max_steps, start, vault, lays, budget, seed=77)
    knobs = {"HEIST_MULTI_WAVES": 1}

    def new(c):
        env = _handle(monkeypatch, knobs, n, c, device=gpu_device, auto_reset=True, **_caps(budget))
        assert env.kernel_config()["lean"] == 1 and env.kernel_config()["multi_waves"] == 1
        return env

    env = new(cfg)
    env.set_layouts(lays, budget=budget)
    env.reset()
    acts, w_obs, w_r, w_d, w_s = ob.rollout(30)
    assert ob.n_vault >= 1  # an auto-reset to the off-corner start happened
    a = torch.from_numpy(acts).to(gpu_device)
    st = None
    for t in range(30):
        if t == 12:
            st = env.save_state()
        obs, _, done, status = env.step(a[t])
        _assert_rows("uninterrupted", "tick %d" % t, (obs, env.reward64, done, status),
                     (w_obs[t], w_r[t], w_d[t], w_s[t]))
    end = env.export(grid=True)
    words = st.blobs[:, :64].cpu().numpy().view(np.uint32)
    assert words[:, 9:13].tolist() == [[start[0], start[1], vault[0], vault[1]]] * n
    second = new(cfg)
    for name, e in (("same handle", env), ("second handle", second)):
        assert bool(e.load_state(st).all()), name
        for t0 in (12, 21):
            obs, _, done, status, r64 = e.step_multi(a[t0:t0 + 9], reward64=True)
            for k in range(9):
                _assert_rows(name, "tick %d" % (t0 + k), (obs[k], r64[k], done[k], status[k]),
                             (w_obs[t0 + k], w_r[t0 + k], w_d[t0 + k], w_s[t0 + k]))
        got = e.export(grid=True)
        for k in end:
            assert torch.equal(got[k], end[k]), (name, k)
    for field, (s2, v2) in {"start_r": ((start[0] + 1, start[1]), vault), "start_c": ((start[0], start[1] + 1), vault),
                            "vault_r": (start, (vault[0] + 1, vault[1])),
                            "vault_c": (start, (vault[0], vault[1] + 1))}.items():
        other = new(_cfg(R, C, s2, v2, budget))
        other.set_layouts(lays, budget=budget)
        other.reset()
        other.step(a[0])
        oc, sc = other.state_config(), env.state_config()
        assert [k for k in oc if oc[k] != sc[k]] == [field]
        before, blobs_before, obs_before = other.export(grid=True), other.save_state().blobs, other.obs.clone()
        with pytest.raises(nat.HeistError):
            other.load_state(st)
        ok = other.load_state(EnvState(st.blobs, oc))  # past the container check: the device's own
        assert ok.shape == (n,) and not bool(ok.any()), field
        after = other.export(grid=True)
        for k in before:
            assert torch.equal(after[k], before[k]), (field, k)
        assert torch.equal(other.save_state().blobs, blobs_before) and torch.equal(other.obs, obs_before), field
        other.close()
    env.close()
    second.close()
