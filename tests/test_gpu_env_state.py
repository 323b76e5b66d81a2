"""GPU tests of env state save / load / fork (heist_state_save, heist_state_load; HeistEnv.save_state /
load_state; HeistEnvironment.get_state / set_state).

Bar: bit-exact.  An env loaded from a blob must give, tick for tick, the observation bytes, the
float64 reward, done and status the saved env gave, and the same export() at the end -- on the
handle it came from, on that handle after its layouts changed, on another handle, in another
process, and forked against the C oracle replaying the history (reference environment.py:183-299).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import pyoracle as po
from heist_amd import EnvironmentConfig, EnvState, HeistEnv, HeistEnvironment
from heist_amd import _native as nat
from heist_amd.layouts import synthetic_layouts

pytestmark = pytest.mark.gpu

MAX_STEPS = 30  # every env times out, and auto-resets, before the save at tick 33
GRIDS = {
    "20x20_lean": dict(R=20, C=20, budget=15, kw={}, env={"HEIST_MULTI_WAVES": "1"}),
    "32x32_w1": dict(R=32, C=32, budget=40, kw={"n_cams": 4, "n_guards": 3},
                     env={"HEIST_MULTI_WAVES": "1", "HEIST_LEAN_WAVES": "1"}),
    "32x32_w2": dict(R=32, C=32, budget=40, kw={"n_cams": 4, "n_guards": 3},
                     env={"HEIST_MULTI_WAVES": "1", "HEIST_LEAN_WAVES": "2"}),
    "12x12": dict(R=12, C=12, budget=15, kw={}, env={}),
    "13x17": dict(R=13, C=17, budget=15, kw={}, env={}),
}
MODES = ("step", "multi1", "multi20", "multi63", "mixed")


def _cfg(g):
    return EnvironmentConfig(grid_rows=g["R"], grid_cols=g["C"], max_steps=MAX_STEPS, architect_budget=g["budget"])


def _new_env(grid, n, device, monkeypatch, cones=True):
    g = GRIDS[grid]
    for k, v in g["env"].items():
        monkeypatch.setenv(k, v)
    env = HeistEnv(n, _cfg(g), max_cams=max(1, g["budget"] // 3), max_guards=max(1, g["budget"] // 5), max_path=8,
                   device=device)
    kc = env.kernel_config()
    if grid == "20x20_lean":
        assert kc["lean"] == 1 and kc["multi_waves"] == 1
    if grid.startswith("32x32"):
        assert kc["lean_waves"] == int(grid[-1])
    env.set_guard_cones(cones)
    return env


def _make(grid, n, device, monkeypatch, cones=True, seed=11):
    """A HeistEnv of n envs on seeded random layouts, reset."""
    g = GRIDS[grid]
    env = _new_env(grid, n, device, monkeypatch, cones)
    lays = synthetic_layouts(n, g["R"], g["C"], g["budget"], seed=seed, **g["kw"])
    env.set_layouts(lays, budget=g["budget"])
    env.reset()
    return env, lays


def _actions(T, n, seed, device):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 5, (T, n))).to(device)


def _play(env, acts, mode="step", auto=True):
    """Play acts [T, n]; the outputs of every tick: obs as int32 words, reward64, done, status."""
    T = int(acts.shape[0])
    out = {"obs": [], "reward64": [], "done": [], "status": []}

    def single(a):
        o, _, d, s = env.step(a, auto_reset=auto)
        for k, v in (("obs", o), ("reward64", env.reward64), ("done", d), ("status", s)):
            out[k].append(v.clone())

    def multi(a):
        o, _, d, s, r = env.step_multi(a, auto_reset=auto, reward64=True)
        for k, v in (("obs", o), ("reward64", r), ("done", d), ("status", s)):
            out[k].extend(v.unbind(0))

    if mode == "step":
        for t in range(T):
            single(acts[t])
    elif mode == "mixed":  # single ticks, then one K-tick launch: a save behind it is followed by single ticks
        for t in range(T // 2):
            single(acts[t])
        if T - T // 2:
            multi(acts[T // 2:])
    else:
        K = int(mode[5:])
        for t in range(0, T, K):
            multi(acts[t:t + K])
    if T == 0:
        return None
    res = {k: torch.stack(v) for k, v in out.items()}
    res["obs"] = res["obs"].view(torch.int32)
    return res


def _cat(parts):
    parts = [p for p in parts if p is not None]
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


def _tail(run, t0, t1=None):
    return {k: v[t0:t1] for k, v in run.items()}


def _assert_same(a, b, ctx=""):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape, "%s %s: shape" % (ctx, k)
        if not torch.equal(a[k], b[k]):
            bad = (a[k] != b[k]).reshape(a[k].shape[0], -1).any(1).nonzero().reshape(-1)
            raise AssertionError("%s %s differs, first at row %d" % (ctx, k, int(bad[0])))


def _run_with_saves(env, acts, mode, auto, save=True):
    """Play acts in the segments [0, 7), [7, 33), [33, T) with a save (and an export) before each."""
    saves, parts, t = {}, [], 0
    for t0 in (0, 7, 33):
        parts.append(_play(env, acts[t:t0], mode, auto))
        t = t0
        if save:
            saves[t0] = (env.save_state(), env.export(grid=True))
    parts.append(_play(env, acts[33:], mode, auto))
    return _cat(parts), env.export(grid=True), saves


# -- 1. continuation ---------------------------------------------------------------------------
@pytest.mark.parametrize("auto", [True, False], ids=["auto_reset", "no_auto_reset"])
@pytest.mark.parametrize("cones", [True, False], ids=["guard_cones", "live_guards"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("grid", list(GRIDS))
def test_continuation(gpu_device, monkeypatch, grid, mode, cones, auto):
    """Save after 0, 7 and 33 ticks of one run (40 more ticks after the last save; 63 where the
    launches are 63 ticks long); loading each save back and playing the run's remaining actions
    gives the run's remaining outputs and its final export."""
    n = 48
    env, _ = _make(grid, n, gpu_device, monkeypatch, cones)
    assert env.kernel_config()["guard_cones"] == int(cones)
    L = 63 if mode == "multi63" else 40
    acts = _actions(33 + L, n, 5, gpu_device)
    run, end, saves = _run_with_saves(env, acts, mode, auto)
    if auto:  # the situations the save at tick 33 holds: a guard off its patrol start, envs that auto-reset
        ex33 = saves[33][1]
        assert bool((ex33["guard_idx"] != 0).any())
        assert bool(run["done"][:33].any())
        assert bool((ex33["tick"] < 33).any())
    for t0 in (0, 7, 33):
        st, ex = saves[t0]
        assert len(st) == n and st.blobs.shape[1] == env.state_config()["bytes"]
        assert bool(env.load_state(st).all())
        _assert_same(env.export(grid=True), ex, "export after load, t0 %d" % t0)
        _assert_same(_play(env, acts[t0:], mode, auto), _tail(run, t0), "t0 %d" % t0)
        _assert_same(env.export(grid=True), end, "final export, t0 %d" % t0)
    env.close()


# -- 2. save reads only ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["step", "multi20"])
@pytest.mark.parametrize("grid", ["20x20_lean", "13x17"])
def test_save_is_read_only(gpu_device, monkeypatch, grid, mode):
    n = 48
    acts = _actions(73, n, 6, gpu_device)
    env, _ = _make(grid, n, gpu_device, monkeypatch)
    run, end, _ = _run_with_saves(env, acts, mode, True)
    env2, _ = _make(grid, n, gpu_device, monkeypatch)
    run2, end2, _ = _run_with_saves(env2, acts, mode, True, save=False)
    _assert_same(run, run2)
    _assert_same(end, end2)
    env.close()
    env2.close()


# -- 3. self-contained -------------------------------------------------------------------------
def _saved_run(grid, n, device, monkeypatch, mode):
    env, _ = _make(grid, n, device, monkeypatch, seed=21)
    _play(env, _actions(9, n, 7, device), "step", True)
    st = env.save_state()
    acts = _actions(40, n, 8, device)
    A = _play(env, acts, mode, True)
    return env, st, acts, A, env.export(grid=True)


@pytest.mark.parametrize("grid", ["20x20_lean", "32x32_w2", "13x17"])
def test_self_contained(gpu_device, monkeypatch, tmp_path, grid):
    """The blob carries its layout: it loads into the same handle after every env got another
    layout, and into a second handle that never saw the layouts (there through torch.save)."""
    n, mode = 48, "multi20"
    g = GRIDS[grid]
    env, st, acts, A, endA = _saved_run(grid, n, gpu_device, monkeypatch, mode)
    env.set_layouts(synthetic_layouts(n, g["R"], g["C"], g["budget"], seed=999, **g["kw"]), budget=g["budget"])
    env.reset()
    _play(env, _actions(10, n, 9, gpu_device), "step", True)
    assert bool(env.load_state(st).all())
    _assert_same(_play(env, acts, mode, True), A, "same handle")
    _assert_same(env.export(grid=True), endA, "same handle")
    path = str(tmp_path / "state.pt")
    st.save(path)
    st2 = EnvState.load(path)
    assert st2.device.type == "cpu" and torch.equal(st2.blobs, st.blobs.cpu()) and st2.config == st.config
    env2 = _new_env(grid, n, gpu_device, monkeypatch)
    assert bool(env2.load_state(st2).all())
    _assert_same(_play(env2, acts, mode, True), A, "second handle")
    _assert_same(env2.export(grid=True), endA, "second handle")
    env.close()
    env2.close()


def test_self_contained_other_process_one_wave_step_kernel(gpu_device, monkeypatch, tmp_path):
    """A handle created under HEIST_STEP_WAVES=1 in a fresh child process continues the saved
    envs bit for bit (the knob does not change results; the blob does not depend on it)."""
    n, grid = 48, "20x20_lean"
    g = GRIDS[grid]
    env, st, acts, A, endA = _saved_run(grid, n, gpu_device, monkeypatch, "step")
    assert env.kernel_config()["step_waves"] != 1
    cfg = _cfg(g)
    job = {"cfg": {"grid_rows": cfg.grid_rows, "grid_cols": cfg.grid_cols, "max_steps": cfg.max_steps,
                   "architect_budget": cfg.architect_budget},
           "n": n, "max_cams": env.max_cams, "max_guards": env.max_guards, "max_path": env.max_path,
           "state": st.cpu().state_dict(), "actions": acts.cpu(), "auto_reset": True}
    jp, op = str(tmp_path / "job.pt"), str(tmp_path / "out.pt")
    torch.save(job, jp)
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "env_state_child.py")
    r = subprocess.run([sys.executable, child, jp, op], env={**os.environ, "HEIST_STEP_WAVES": "1"},
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = torch.load(op, weights_only=False)
    assert out["step_waves"] == 1 and bool(out["loaded"].all())
    _assert_same({k: out[k] for k in A}, {k: v.cpu() for k, v in A.items()}, "child")
    _assert_same(out["export"], {k: v.cpu() for k, v in endA.items()}, "child")
    env.close()


# -- 4. fork against the oracle ----------------------------------------------------------------
def test_fork_matches_oracle(gpu_device, monkeypatch):
    """Env 0 after 12 ticks, loaded into all 16 envs, continued under 16 action sequences: each
    equals the oracle replaying layout 0 through the history and that env's own actions."""
    n, grid = 16, "20x20_lean"
    g = GRIDS[grid]
    env, lays = _make(grid, n, gpu_device, monkeypatch, seed=33)
    hist = _actions(12, n, 10, gpu_device)
    _play(env, hist, "step", True)
    st = env.save_state([0])
    assert len(st) == 1
    ok = env.load_state(st, index=torch.zeros(n, dtype=torch.int64))
    assert ok.shape == (n,) and bool(ok.all())
    fa = _actions(30, n, 12, gpu_device)
    B = {k: v.cpu().numpy() for k, v in _play(env, fa, "multi20", True).items()}
    h0, fa_h = hist[:, 0].cpu().numpy(), fa.cpu().numpy()
    n_done = 0
    for e in range(n):
        o = po.OracleEnv(g["R"], g["C"], MAX_STEPS, (1, 1), (g["R"] - 2, g["C"] - 2), g["budget"])
        o.set_layout(*lays[0])
        o.reset()
        for a in h0:
            if o.step(int(a))[1]:
                o.reset()
        for k in range(30):
            r, d, s = o.step(int(fa_h[k, e]))
            if d:
                o.reset()
                n_done += 1
            ctx = "env %d tick %d" % (e, k)
            assert (B["reward64"][k, e], bool(B["done"][k, e]), int(B["status"][k, e])) == (r, d, s), ctx
            assert B["obs"][k, e].tobytes() == o.state_tensor().tobytes(), ctx
    assert n_done >= n  # every fork ran into a time-out (max_steps 30) and auto-reset
    env.close()


# -- 5. subset ---------------------------------------------------------------------------------
def test_subset_load_leaves_other_envs(gpu_device, monkeypatch):
    n = 32
    env, _ = _make("20x20_lean", n, gpu_device, monkeypatch, seed=44)
    _play(env, _actions(3, n, 13, gpu_device), "step", True)
    early = env.save_state()
    early_ex = env.export(grid=True)
    _play(env, _actions(12, n, 14, gpu_device), "multi20", True)
    now = env.save_state()
    before = env.export(grid=True)
    acts = _actions(20, n, 15, gpu_device)
    ref = _play(env, acts, "multi20", True)
    assert bool(env.load_state(now).all())
    ids = [4, 0, 31, 17, 9]
    rest = torch.tensor([e for e in range(n) if e not in ids], device=gpu_device)
    idt = torch.tensor(ids, device=gpu_device)
    ok = env.load_state(early, env_ids=ids, index=ids)
    assert ok.shape == (5,) and bool(ok.all())
    after = env.export(grid=True)
    for k in before:
        assert torch.equal(after[k][rest], before[k][rest]), k
        assert torch.equal(after[k][idt], early_ex[k][idt]), k
    got = _play(env, acts, "multi20", True)
    for k in ref:
        assert torch.equal(got[k][:, rest], ref[k][:, rest]), k
    env.close()


# -- 6. rejection ------------------------------------------------------------------------------
def _as_blobs_of(env, st):
    """st's blobs cut or zero-padded to env's blob size under env's configuration: what a caller
    who bypasses the container check hands the device."""
    cfg = env.state_config()
    b = torch.zeros((len(st), cfg["bytes"]), dtype=torch.uint8, device=st.device)
    w = min(cfg["bytes"], st.blobs.shape[1])
    b[:, :w] = st.blobs[:, :w]
    return EnvState(b, cfg)


def test_rejection(gpu_device, monkeypatch):
    n = 8
    env, _ = _make("20x20_lean", n, gpu_device, monkeypatch, seed=55)
    first = env.save_state()
    first_ex = env.export(grid=True)
    _play(env, _actions(5, n, 16, gpu_device), "step", True)
    keep = env.save_state()
    keep_ex = env.export(grid=True)
    acts = _actions(10, n, 17, gpu_device)
    ref = _play(env, acts, "step", True)
    assert bool(env.load_state(keep).all())

    small, _ = _make("12x12", n, gpu_device, monkeypatch, seed=56)
    g = GRIDS["20x20_lean"]
    fewer = HeistEnv(n, _cfg(g), max_cams=5, max_guards=2, max_path=8, device=gpu_device)
    fewer.set_layouts(synthetic_layouts(n, 20, 20, 10, seed=57), budget=10)
    fewer.reset()
    no_magic = first.blobs.clone()
    no_magic[:, :4] = 0
    cases = {"12x12 blob": _as_blobs_of(env, small.save_state()),
             "max_guards 2 blob": _as_blobs_of(env, fewer.save_state()),
             "magic overwritten": EnvState(no_magic, first.config)}
    for name, bad in cases.items():
        ok = env.load_state(bad)
        assert ok.shape == (n,) and not bool(ok.any()), name
        _assert_same(env.export(grid=True), keep_ex, name)
    # the container check: a mismatching configuration raises before any launch
    for other in (small, fewer):
        with pytest.raises(nat.HeistError):
            env.load_state(other.save_state())
    _assert_same(env.export(grid=True), keep_ex, "after the raises")
    _assert_same(_play(env, acts, "step", True), ref, "continuation after rejected loads")
    assert bool(env.load_state(keep).all())

    # per-item rejection: the neighbours of a bad item are loaded (tick 0 of `first`), the bad one is not
    def check(ok, want, loaded_envs):
        assert ok.cpu().tolist() == want
        ex = env.export(grid=True)
        for e in range(n):
            src = first_ex if e in loaded_envs else keep_ex
            for k in ex:
                assert torch.equal(ex[k][e], src[k][e]), (k, e)
        assert bool(env.load_state(keep).all())

    check(env.load_state(first, env_ids=[1, 99, 3], index=[1, 2, 3]), [True, False, True], {1, 3})
    check(env.load_state(first, env_ids=[1, -1, 3], index=[1, 2, 3]), [True, False, True], {1, 3})
    check(env.load_state(first, env_ids=[2, 2, 4], index=[2, 5, 4]), [False, False, True], {4})
    check(env.load_state(first, env_ids=[5, 6, 7], index=[5, n, 7]), [True, False, True], {5, 7})
    check(env.load_state(first, env_ids=[5, 6, 7], index=[5, -1, 7]), [True, False, True], {5, 7})
    _assert_same(_play(env, acts, "step", True), ref, "continuation at the end")
    # arguments the host sees
    L, P = nat.lib(), nat.ptr
    buf = torch.zeros(first.blobs.numel() + 16, dtype=torch.uint8, device=gpu_device)
    s = nat.stream(gpu_device)
    assert L.heist_state_load(env._h, None, -1, P(buf), n, None, None, s) == 100000
    assert L.heist_state_load(env._h, None, 1, None, n, None, None, s) == 100000
    assert L.heist_state_load(env._h, None, 1, P(buf[1:]), n, None, None, s) == 100000
    assert L.heist_state_save(env._h, None, 1, P(buf[1:]), s) == 100000
    assert L.heist_state_save(env._h, None, -1, P(buf), s) == 100000
    assert L.heist_state_load(env._h, None, 0, None, 0, None, None, s) == 0
    for e in (env, small, fewer):
        e.close()


# -- 7. bounds ---------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 3, 48])
def test_save_stays_inside_its_blobs(gpu_device, monkeypatch, m):
    n = 48
    env, _ = _make("13x17", n, gpu_device, monkeypatch, seed=66)
    nb = env.state_config()["bytes"]
    assert nb % 16 == 0 and nb == nat.lib().heist_state_bytes(env._h)
    buf = torch.full((m * nb + 256,), 0xA5, dtype=torch.uint8, device=gpu_device)
    ids = None if m == n else torch.arange(n - m, n, dtype=torch.int32, device=gpu_device)
    nat.check(nat.lib().heist_state_save(env._h, nat.ptr(ids), m, nat.ptr(buf), nat.stream(gpu_device)), "save")
    assert bool((buf[m * nb:] == 0xA5).all())
    blobs = buf[:m * nb].view(m, nb)
    assert torch.equal(blobs, env.save_state(ids).blobs)
    assert bytes(blobs[0, :4].cpu().tolist()) == b"HEST"
    env.close()


# -- 8. the single-env compatibility class -----------------------------------------------------
def test_compat_class_get_set_state(gpu_device):
    cfg = EnvironmentConfig(max_steps=200)
    env = HeistEnvironment(cfg, device=gpu_device)
    walls, cams, guards = synthetic_layouts(1, 20, 20, 15, seed=77, n_cams=2, n_guards=1)[0]
    env.set_layout(walls, cams, guards)
    env.reset()
    rng = np.random.default_rng(18)
    for a in rng.integers(0, 5, 5):
        env.step(int(a))
    st = env.get_state()
    tensor0 = env.get_state_tensor()
    acts = [int(a) for a in rng.integers(0, 5, 15)]
    rew1 = [env.step(a)[1] for a in acts]
    es1, txt1, obs1 = env.get_environment_state(), env.render_text(), env.get_state_tensor()
    env.set_state(st)
    assert env.tick == 5 and env.solver_path == [env.solver_pos]
    assert env.get_state_tensor().tobytes() == tensor0.tobytes()
    rew2 = [env.step(a)[1] for a in acts]
    es2, txt2, obs2 = env.get_environment_state(), env.render_text(), env.get_state_tensor()
    assert rew1 == rew2 and txt1 == txt2 and obs1.tobytes() == obs2.tobytes()
    assert es1["solver_path"][-16:] == es2["solver_path"]  # the path restarts at the cell of the saved tick
    for k in es1:
        if k != "solver_path":
            assert es1[k] == es2[k], k


# -- the lift-out tool -------------------------------------------------------------------------
def test_replay_tool_lifts_one_env_out(gpu_device, monkeypatch, tmp_path, capsys):
    """tools/replay_env.py on env 5 of a saved batch prints, tick for tick, what env 5 gave in the batch."""
    from heist_amd import STATUS_NAMES
    n, e = 16, 5
    env, _ = _make("20x20_lean", n, gpu_device, monkeypatch, seed=88)
    _play(env, _actions(6, n, 19, gpu_device), "step", True)
    path = str(tmp_path / "batch.pt")
    env.save_state().save(path)
    acts = _actions(12, n, 20, gpu_device)
    ref = _play(env, acts, "step", False)
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import replay_env
    capsys.readouterr()
    replay_env.main([path, "--env", str(e), "--actions", ",".join(str(int(a)) for a in acts[:, e].cpu())])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if " action " in ln]
    assert len(lines) == 12
    for k, ln in enumerate(lines):
        assert "reward %r " % float(ref["reward64"][k, e]) in ln, ln
        assert "done %d " % int(ref["done"][k, e]) in ln and "status %s " % STATUS_NAMES[int(ref["status"][k, e])] in ln, ln
    env.close()
