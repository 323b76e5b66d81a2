"""Shared bodies of the environment parity tests: the golden-trace replays (test_gpu_env.py,
test_gpu_env_offcorner.py) and the batched oracle replay with actions steered towards the vault.

The oracle side (OracleBatch, the OFFCORNER table) needs no GPU; the check_* functions do.
"""
import numpy as np

import golden_data as gd
from oracle import pyoracle as po

STATUS_RESET = 5
OFFCORNER_FILE = "env_traces_offcorner.npz"


def trace_cfg(tr):
    from heist_amd import EnvironmentConfig
    return EnvironmentConfig(grid_rows=tr["R"], grid_cols=tr["C"], max_steps=tr["max_steps"], start_pos=tr["start"],
                             vault_pos=tr["vault"], architect_budget=tr["budget"])


def check_golden_trace(tr, cones, path, gpu_device, monkeypatch):
    """One golden trace on one single-tick path ("step_kernel": HEIST_STEP_LEAN=0; "lean_k1":
    heist_step as a one-tick heist_step_multi launch where the lean K-tick kernel serves the
    grid), with the guard cone cache on or off: layout validity, grid and accepted counts, then
    per op the float64 reward, done, status, position, tick, headings, guard indices, the
    visibility plane and (for the recorded ops) the observation bytes."""
    import torch
    from heist_amd import HeistEnv
    if path == "lean_k1":
        monkeypatch.setenv("HEIST_MULTI_WAVES", "1")
        monkeypatch.setenv("HEIST_STEP_LEAN", "1")
    else:
        monkeypatch.setenv("HEIST_STEP_LEAN", "0")
    env = HeistEnv(1, trace_cfg(tr), max_cams=16, max_guards=8, max_path=64, device=gpu_device, auto_reset=False)
    lean_grid = (tr["R"], tr["C"]) in ((20, 20), (32, 32))
    assert env.kernel_config()["step_lean"] == (1 if path == "lean_k1" and lean_grid else 0)
    env.set_guard_cones(cones)
    valid = env.set_layouts([(tr["walls"], tr["cams"], tr["guards"])], budget=tr["budget"])
    assert bool(valid[0]) == tr["valid"]
    st = env.export(grid=True)
    np.testing.assert_array_equal(st["grid"][0].cpu().numpy(), tr["grid"])
    acc = [int(st[k][0]) for k in ("n_walls", "n_cams", "n_guards", "spent")]
    assert acc == tr["accepted"]
    nc, ng = tr["accepted"][1], tr["accepted"][2]
    for k, op in enumerate(tr["ops"]):
        ctx = "%s op#%d" % (tr["name"], k)
        if op == -1:
            obs = env.reset()
            r, d, s = 0.0, None, STATUS_RESET
        else:
            obs, _, dn, stt = env.step(torch.tensor([op]))
            r, d, s = float(env.reward64[0]), bool(dn[0]), int(stt[0])
        st = env.export()
        assert r == tr["reward"][k], ctx
        if d is not None:
            assert d == tr["done"][k], ctx
        assert s == tr["status"][k], ctx
        assert (int(st["pos_r"][0]), int(st["pos_c"][0])) == tuple(tr["pos"][k]), ctx
        assert int(st["tick"][0]) == tr["tick"][k], ctx
        assert bool(st["done"][0]) == tr["done"][k], ctx
        np.testing.assert_array_equal(st["cam_heading"][0, :nc].cpu().numpy(), tr["cam_h"][k], err_msg=ctx)
        np.testing.assert_array_equal(st["guard_idx"][0, :ng].cpu().numpy(), tr["g_idx"][k], err_msg=ctx)
        np.testing.assert_array_equal(st["guard_heading"][0, :ng].cpu().numpy(), tr["g_h"][k], err_msg=ctx)
        o = obs[0].cpu().numpy()
        np.testing.assert_array_equal(o[1] > 0.5, tr["vis"][k], err_msg=ctx)
        if k < len(tr["state"]):
            assert o.tobytes() == tr["state"][k].tobytes(), ctx


def check_single_env_class_trace(tr, gpu_device, n_ops=150):
    """One golden trace through HeistEnvironment (the reference's API, GPU-backed)."""
    from heist_amd import HeistEnvironment
    env = HeistEnvironment(trace_cfg(tr), device=gpu_device)
    assert env.set_layout(tr["walls"], tr["cams"], tr["guards"]) == tr["valid"]
    assert (len(env.walls), len(env.cameras), len(env.guards), env.budget.spent) == tuple(tr["accepted"])
    np.testing.assert_array_equal(env.grid, tr["grid"])
    for k, op in enumerate(tr["ops"][:n_ops]):
        ctx = "%s op#%d" % (tr["name"], k)
        if op == -1:
            env.reset()
            r = 0.0
        else:
            _, r, d, info = env.step(int(op))
            assert d == tr["done"][k], ctx
            assert po.STATUS_NAMES[int(tr["status"][k])] == info["status"], ctx
        assert r == tr["reward"][k], ctx
        assert env.solver_pos == tuple(tr["pos"][k]) and env.tick == tr["tick"][k], ctx
        assert [c.heading for c in env.cameras] == list(tr["cam_h"][k]), ctx
        assert [g.current_idx for g in env.guards] == list(tr["g_idx"][k]), ctx
        np.testing.assert_array_equal(env.visibility_map.visibility > 0.5, tr["vis"][k], err_msg=ctx)
        if k < len(tr["state"]):
            assert env.get_state_tensor().tobytes() == tr["state"][k].tobytes(), ctx


# -- start and vault away from the corners: the batched configurations ---------------------------
# Per grid: the layouts' budget and synthetic_layouts keywords, the ticks of a batched run, and one
# (start, vault) pair per vault lane 0..3, lane = (vault_r * C + vault_c) & 3: the lane of channel
# 2's float4 the vault is patched into where C % 4 == 0.  No start is (1, 1), no vault (R-2, C-2),
# no pair is symmetric in rows and columns, and every start is within 16 steps of its vault, so
# that steered solvers (golden_data.steered_action) arrive within max_steps = 40.  seeds: the
# layout seed per lane, chosen on the CPU oracle so that the steered walks of 64 envs stand on every
# cell of the vault's float4 (the cells beyond the vault are only reached by the rule's random moves).
OFFCORNER = {
    (20, 20): dict(budget=15, kw={}, T=80, seeds=(0, 0, 0, 0),
                   pairs=[((11, 13), (5, 8)), ((16, 3), (12, 9)), ((6, 15), (14, 10)), ((3, 4), (7, 11))]),
    (32, 32): dict(budget=40, kw={"n_cams": 4, "n_guards": 3}, T=80, seeds=(0, 0, 1, 0),
                   pairs=[((12, 18), (20, 12)), ((16, 14), (9, 21)), ((22, 26), (14, 18)), ((15, 17), (22, 23))]),
    (13, 17): dict(budget=15, kw={}, T=60, seeds=(0, 0, 2, 0),
                   pairs=[((9, 14), (3, 9)), ((10, 14), (3, 10)), ((2, 13), (8, 6)), ((9, 4), (3, 12))]),
    (16, 20): dict(budget=15, kw={}, T=60, seeds=(0, 0, 0, 0),
                   pairs=[((12, 17), (5, 12)), ((4, 12), (12, 5)), ((3, 5), (9, 14)), ((11, 15), (4, 7))]),
}
OFFCORNER_MAX_STEPS = 40


def offcorner_case(R, C, lane, n):
    """(start, vault, layouts, budget, T) of the batched run on an R x C grid with the vault in
    `lane`.  Every other env has walls only: its solver is never seen, so the steered walks end
    on the vault and pass the cells next to it; the others carry the grid's cameras and guards."""
    from heist_amd.layouts import synthetic_layouts
    g = OFFCORNER[(R, C)]
    start, vault = g["pairs"][lane]
    assert (vault[0] * C + vault[1]) & 3 == lane
    s = 7000 + 100 * R + 10 * lane + g["seeds"][lane]
    watched = synthetic_layouts(n, R, C, g["budget"], seed=s, start=start, vault=vault, **g["kw"])
    walls = synthetic_layouts(n, R, C, g["budget"], seed=s + 1, start=start, vault=vault, n_cams=0, n_guards=0)
    lays = [watched[i] if i % 2 == 0 else walls[i] for i in range(n)]
    return start, vault, lays, g["budget"], g["T"]


def quad_offsets_allowed(R, C, vault):
    """The lanes, other than the vault's, of the vault's float4 (cells 4q .. 4q+3 of the
    flattened grid) that a solver can stand on: the cells inside the border ring."""
    v = vault[0] * C + vault[1]
    out = set()
    for l in range(4):
        r, c = divmod((v & ~3) + l, C)
        if l != (v & 3) and 1 <= r <= R - 2 and 1 <= c <= C - 2:
            out.add(l)
    return out


class OracleBatch:
    """n oracle envs of one configuration, stepped together; actions steered towards the vault
    from the oracles' own positions.  Counts what the tests require to have happened."""

    def __init__(self, R, C, max_steps, start, vault, lays, budget, seed, auto_reset=True):
        self.R, self.C, self.start, self.vault, self.auto_reset = R, C, tuple(start), tuple(vault), auto_reset
        self.envs = []
        self.valid = []
        for lay in lays:
            o = po.OracleEnv(R, C, max_steps, start, vault, budget)
            self.valid.append(o.set_layout(*lay))
            o.reset()
            self.envs.append(o)
        self.rng = np.random.default_rng(seed)
        self.n_vault = self.n_detected = self.n_timeout = 0
        self.quad_offsets = set()  # in-quad lanes a displayed solver stood on, next to the vault
        self.early_vault = 0       # (step_multi) launches with a vault finish before the last tick

    def obs(self):
        return np.stack([o.state_tensor() for o in self.envs])

    def choose(self):
        acts = np.empty(len(self.envs), np.int64)
        for i, o in enumerate(self.envs):
            inf = o.info()
            acts[i] = gd.steered_action(self.rng, (inf["pos_r"], inf["pos_c"]), self.vault)
        return acts

    def step(self, acts):
        """One tick of every env: (obs [n, 3, R, C], reward64 [n], done [n], status [n]), the
        observation after the auto-reset of a finished env as HeistEnv.step gives it."""
        n = len(self.envs)
        r64, done, status = np.empty(n, np.float64), np.empty(n, bool), np.empty(n, np.int8)
        v = self.vault[0] * self.C + self.vault[1]
        for i, o in enumerate(self.envs):
            r64[i], done[i], status[i] = o.step(int(acts[i]))
            self.n_vault += status[i] == 2
            self.n_detected += status[i] == 1
            self.n_timeout += status[i] == 3
            if done[i] and self.auto_reset and status[i] != 4:
                o.reset()
            inf = o.info()
            cell = inf["pos_r"] * self.C + inf["pos_c"]
            if cell >> 2 == v >> 2 and cell != v:
                self.quad_offsets.add(cell & 3)
        return self.obs(), r64, done, status

    def rollout(self, K):
        """K steered ticks: (actions [K, n], obs [K, n, 3, R, C], reward64, done, status [K, n])."""
        A, O, R_, D, S = [], [], [], [], []
        for k in range(K):
            a = self.choose()
            o, r, d, s = self.step(a)
            A.append(a); O.append(o); R_.append(r); D.append(d); S.append(s)
        S = np.stack(S)
        self.early_vault += bool((S[:K - 1] == 2).any())
        return np.stack(A), np.stack(O), np.stack(R_), np.stack(D), S

    def reset_done(self):
        """reset() every finished env (between launches without auto-reset); returns the mask."""
        m = np.array([bool(o.info()["done"]) for o in self.envs])
        for i in np.nonzero(m)[0]:
            self.envs[i].reset()
        return m


def same_bits(a, b):
    """float32 arrays equal bit for bit (signed zeros count)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))
