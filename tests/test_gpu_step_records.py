"""heist_step_multi_records (HeistEnv.step_multi_records): K-tick launches whose rows are the
compact observation records, written by the K-tick kernels themselves (the lean kernel, the
generic K-tick kernel) or, where neither serves the handle, by K x (heist_step, heist_obs_pack).

Every case builds two identical envs: a runs step_multi_records over launches of 1, 2, 20 and 7
ticks, b one heist_step per tick.  For every tick and every env (invalid layouts included) the
record must equal b.pack_obs of b's observation, reward, float64 reward, done and status must be
equal, and both must end in the same exported state.  Independent of the kernels under test and
of heist_obs_pack, the records of the oracle-replayed envs are compared with records built in
NumPy from the C oracle's state_tensor().
"""
import functools

import numpy as np
import pytest
import torch

from heist_amd import EnvironmentConfig, _native as nat
from heist_amd.layouts import synthetic_layouts
from heist_amd.obs_compact import CompactObs, record_words
from test_gpu_env import _twin_envs
from test_gpu_lean_reset import (LAUNCHES, _actions, _check_counts, _plan, edge20_case, fan20_case, ivl20_case,
                                 mix32_case, wide20_case)

pytestmark = pytest.mark.gpu

HEIST_EINVAL = 100000

# name -> (builder, its argument or None, the action seed test_gpu_lean_reset runs the case with:
# that file shows the oracle replay meets the situation counts for these seeds)
CASES = {"fan20": (fan20_case, 2, 902), "ivl20": (ivl20_case, 2, 922), "wide20": (wide20_case, "fov151", 910),
         "edge20": (edge20_case, None, 940), "mix32": (mix32_case, None, 930)}


def _numpy_record(row, R, C, vault):
    """The record of one oracle observation (the bytes of its [3][R][C] float32 state_tensor())."""
    t = np.frombuffer(row, np.float32).reshape(3, R, C)
    nvis, W = (R * C + 31) // 32, record_words(R, C)
    bits = np.packbits(t[1].reshape(-1) != 0, bitorder="little")
    vis = np.zeros(4 * nvis, np.uint8)
    vis[:len(bits)] = bits
    cells = np.argwhere(t[2] > 0.5)
    assert len(cells) <= 1
    r, c = (int(cells[0][0]), int(cells[0][1])) if len(cells) else vault
    rec = np.zeros(W, np.uint32)
    rec[:nvis] = vis.view(np.uint32)
    rec[nvis] = r | c << 8
    return rec


@functools.lru_cache(maxsize=None)
def _case(name, auto_reset):
    """A case's layouts, actions and oracle replay (no GPU), once for the tests that share it."""
    builder, arg, seed = CASES[name]
    cfg, lays, budget, mc, mg = builder() if arg is None else builder(arg)
    acts = _actions(len(lays), sum(LAUNCHES), seed)
    valid, pick, rows, counts = _plan(cfg, lays, budget, acts, LAUNCHES, auto_reset)
    print("situation counts:", counts)
    _check_counts(counts, budget, auto_reset)
    want = {int(i): np.stack([_numpy_record(r[0], cfg.grid_rows, cfg.grid_cols, cfg.vault_pos) for r in rows[int(i)]])
            for i in pick}
    return cfg, lays, budget, mc, mg, acts, pick, rows, want


def _compare(a, b, acts_d, auto_reset, pick=(), rows=None, want=None):
    k0 = 0
    W = record_words(a.rows, a.cols)
    for K in LAUNCHES:
        rec, rew, done, status, r64 = a.step_multi_records(acts_d[k0:k0 + K], auto_reset=auto_reset, reward64=True)
        assert rec.shape == (K, a.n_envs, W) and rec.dtype == torch.int32
        rec_h = rec.cpu().numpy().view(np.uint32)
        r64_h, done_h, st_h = (x.cpu().numpy() for x in (r64, done, status))
        for k in range(K):
            o, r, d, s = b.step(acts_d[k0 + k], auto_reset=auto_reset)
            ctx = "tick %d" % (k0 + k)
            assert torch.equal(rec[k], b.pack_obs(o)), ctx
            assert torch.equal(r64[k], b.reward64) and torch.equal(rew[k], r), ctx
            assert torch.equal(done[k], d) and torch.equal(status[k], s), ctx
            for i in pick:
                _, r_, d_, s_ = rows[int(i)][k0 + k]
                assert (float(r64_h[k, i]), bool(done_h[k, i]), int(st_h[k, i])) == (r_, d_, s_), "env %d %s" % (i, ctx)
                np.testing.assert_array_equal(rec_h[k, i], want[int(i)][k0 + k], "env %d %s" % (i, ctx))
        k0 += K
    sa, sb = a.export(grid=True), b.export(grid=True)
    for key in sb:
        assert torch.equal(sa[key], sb[key]), key


def _run_case(gpu_device, monkeypatch, name, auto_reset, lean, multi_waves=1, lean_waves=None):
    cfg, lays, budget, mc, mg, acts, pick, rows, want = _case(name, auto_reset)
    if multi_waves is not None:
        monkeypatch.setenv("HEIST_MULTI_WAVES", str(multi_waves))
    if lean_waves is not None:
        monkeypatch.setenv("HEIST_LEAN_WAVES", str(lean_waves))
    if not lean:
        monkeypatch.setenv("HEIST_LEAN", "0")
    a, b = _twin_envs(len(lays), cfg, lays, budget, gpu_device, max_cams=mc, max_guards=mg, max_path=16)
    kc = a.kernel_config()
    assert a.records_direct == 1 and kc["lean"] == (1 if lean else 0), kc
    if lean_waves is not None and torch.cuda.get_device_properties(gpu_device).multi_processor_count >= 256:
        assert kc["lean_waves"] == lean_waves, kc
    _compare(a, b, acts.to(gpu_device), auto_reset, pick, rows, want)
    a.close()
    b.close()


# ---- the lean kernel's record form (step_lean_kernel<.., REC>)

@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto_reset", "no_reset"])
@pytest.mark.parametrize("name", ["fan20", "ivl20"])
def test_lean20_resets(gpu_device, monkeypatch, name, auto_reset):
    """20 x 20, max_steps 2: shared fan and interval fans; resets at the first and the last tick of a
    launch and on consecutive ticks (a reset row's position word is the start cell), frozen envs
    without auto-reset."""
    _run_case(gpu_device, monkeypatch, name, auto_reset, lean=True)


@pytest.mark.parametrize("name", ["wide20", "edge20"])
def test_lean20_wide_fans_and_edge_layouts(gpu_device, monkeypatch, name):
    _run_case(gpu_device, monkeypatch, name, True, lean=True)


@pytest.mark.parametrize("waves", [1, 2])
def test_lean32_one_and_two_waves(gpu_device, monkeypatch, waves):
    """32 x 32: 32 visibility words and a 4-word tail; with two waves each wave stores its own
    quads' words, wave 0 the tail; the generic-body envs of the batch write records too."""
    _run_case(gpu_device, monkeypatch, "mix32", True, lean=True, lean_waves=waves)


# ---- the generic K-tick kernel's record form (step_multi_kernel<.., REC>)

@pytest.mark.parametrize("multi_waves", [1, None], ids=["one_wave", "default_waves"])
@pytest.mark.parametrize("name", ["fan20", "ivl20"])
def test_generic20(gpu_device, monkeypatch, name, multi_waves):
    """HEIST_LEAN=0: the generic K-tick kernel, one wave per env and the handle's default (four
    waves per env at 64 envs).

    fan20 at two or more waves per env is the case that found cast_rays' packed flush of a shared
    fan entry with more than 64 unique directions handing zero directions to some (camera,
    direction) pairs: the 96.5-degree fan of five cameras has such entries at ticks 3, 12, 17 and
    22."""
    _run_case(gpu_device, monkeypatch, name, True, lean=False, multi_waves=multi_waves)


@pytest.mark.parametrize("multi_waves", [2, None], ids=["two_waves", "default_waves"])
def test_generic20_obs_form_wide_shared_fan(gpu_device, monkeypatch, multi_waves):
    """heist_step_multi itself (the observation rows) on the generic kernel at two and four waves
    per env, fan20's layouts: every row equals heist_step's and, for the oracle-replayed envs,
    the oracle's state_tensor(), the ticks whose shared fan entry has more than 64 unique
    directions (a packed march of table and register directions) included."""
    cfg, lays, budget, mc, mg, acts, pick, rows, _ = _case("fan20", True)
    if multi_waves is not None:
        monkeypatch.setenv("HEIST_MULTI_WAVES", str(multi_waves))
    monkeypatch.setenv("HEIST_LEAN", "0")
    a, b = _twin_envs(len(lays), cfg, lays, budget, gpu_device, max_cams=mc, max_guards=mg, max_path=16)
    kc = a.kernel_config()
    assert kc["lean"] == 0 and kc["multi_waves"] == (multi_waves or 4), kc
    acts_d = acts.to(gpu_device)
    k0 = 0
    for K in LAUNCHES:
        obs, rew, done, status, _ = a.step_multi(acts_d[k0:k0 + K], auto_reset=True)
        obs_h = obs.cpu().numpy()
        for k in range(K):
            o, r, d, s = b.step(acts_d[k0 + k], auto_reset=True)
            ctx = "tick %d" % (k0 + k)
            assert torch.equal(obs[k].view(torch.int32), o.view(torch.int32)), ctx
            assert torch.equal(rew[k], r) and torch.equal(done[k], d) and torch.equal(status[k], s), ctx
            for i in pick:
                assert obs_h[k, i].tobytes() == rows[int(i)][k0 + k][0], "env %d %s" % (i, ctx)
        k0 += K
    a.close()
    b.close()


def _synthetic(gpu_device, n, R, C, seed, budget=15):
    """test_gpu_obs_compact._env's layouts on twin envs, every valid env replayed by the oracle."""
    from oracle import pyoracle as po
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=C)
    lays = synthetic_layouts(n, R, C, budget, seed=seed)
    acts = _actions(n, sum(LAUNCHES), seed)
    pick, rows, want = [], {}, {}
    for i, lay in enumerate(lays):
        o = po.OracleEnv(R, C, cfg.max_steps, cfg.start_pos, cfg.vault_pos, budget)
        if not o.set_layout(*lay):
            continue
        o.reset()
        pick.append(i)
        rows[i] = []
        for t in range(sum(LAUNCHES)):
            r, d, s = o.step(int(acts[t, i]))
            if d:
                o.reset()
            rows[i].append((o.state_tensor().tobytes(), r, d, s))
        want[i] = np.stack([_numpy_record(r[0], R, C, cfg.vault_pos) for r in rows[i]])
    assert pick
    a, b = _twin_envs(n, cfg, lays, budget, gpu_device)
    return a, b, acts.to(gpu_device), pick, rows, want


@pytest.mark.parametrize("R,C", [(64, 64), (10, 12)])
def test_generic_other_grids(gpu_device, R, C):
    """64 x 64: 128 visibility words, two passes of the observation lanes.  10 x 12: three quads
    per grid row, so a word spans rows; 120 cells, a partial last word."""
    a, b, acts, pick, rows, want = _synthetic(gpu_device, 16, R, C, seed=11 + R)
    assert a.records_direct == 1
    _compare(a, b, acts, True, pick, rows, want)
    a.close()
    b.close()


# ---- the fallback: K x (heist_step into the scratch row, heist_obs_pack)

def test_fallback_width_not_a_multiple_of_4(gpu_device):
    a, b, acts, pick, rows, want = _synthetic(gpu_device, 16, 13, 17, seed=24)
    assert a.records_direct == 0
    K, n, W = 3, 16, record_words(13, 17)
    bufs = [torch.empty((K, n, W), dtype=torch.int32, device=gpu_device), torch.empty((K, n), device=gpu_device),
            torch.empty((K, n), dtype=torch.uint8, device=gpu_device),
            torch.empty((K, n), dtype=torch.int8, device=gpu_device)]
    before = a.export(grid=True)
    with torch.cuda.device(gpu_device):
        rc = nat.lib().heist_step_multi_records(a._h, K, nat.ptr(acts[:K].contiguous()), nat.ptr(bufs[0]),
                                                nat.ptr(bufs[1]), None, nat.ptr(bufs[2]), nat.ptr(bufs[3]), 1, None,
                                                a._stream())
    assert rc == HEIST_EINVAL
    after = a.export(grid=True)
    for key in before:  # refused before any launch
        assert torch.equal(before[key], after[key]), key
    _compare(a, b, acts, True, pick, rows, want)
    a.close()
    b.close()


def test_fallback_with_sample_counters_armed(gpu_device, monkeypatch):
    cfg, lays, budget, mc, mg, acts, pick, rows, want = _case("fan20", True)
    monkeypatch.setenv("HEIST_MULTI_WAVES", "1")
    a, b = _twin_envs(len(lays), cfg, lays, budget, gpu_device, max_cams=mc, max_guards=mg, max_path=16)
    assert a.records_direct == 1
    counter = torch.zeros(len(lays), dtype=torch.int64, device=gpu_device)
    a.count_samples(counter)
    assert a.records_direct == 0
    _compare(a, b, acts.to(gpu_device), True, pick, rows, want)
    assert int(counter.sum()) > 0
    a.count_samples(None)
    assert a.records_direct == 1
    a.close()
    b.close()


# ---- the position word, the round trip, argument checks

@pytest.mark.parametrize("auto_reset", [False, True], ids=["no_reset", "auto_reset"])
def test_solver_on_the_vault(gpu_device, auto_reset):
    """Start (1, 1), vault (1, 2), action RIGHT: the record names the vault's cell, or with
    auto-reset the start cell of the next attempt."""
    cfg = EnvironmentConfig(grid_rows=20, grid_cols=20, start_pos=(1, 1), vault_pos=(1, 2))
    n = 4
    a, b = _twin_envs(n, cfg, [([], [], [])] * n, 15, gpu_device)
    assert a.records_direct == 1
    acts = torch.full((1, n), 4, dtype=torch.int64, device=gpu_device)
    rec, _, done, status, _ = a.step_multi_records(acts, auto_reset=auto_reset)
    assert bool(done.all()) and status[0].tolist() == [2] * n
    nvis = (400 + 31) // 32
    assert rec[0, :, nvis].tolist() == [(1 | 2 << 8) if not auto_reset else (1 | 1 << 8)] * n
    o, _, _, _ = b.step(acts[0], auto_reset=auto_reset)
    assert torch.equal(rec[0], b.pack_obs(o))
    a.close()
    b.close()


def test_round_trip_and_arguments(gpu_device, monkeypatch):
    """One K = 20 launch at 20 x 20: CompactObs.of_env(a, records).expand() is, bit for bit, the
    observations of b's 20 steps; records_out is written in place; bad arguments are refused."""
    cfg, lays, budget, mc, mg, acts, _, _, _ = _case("ivl20", True)
    monkeypatch.setenv("HEIST_MULTI_WAVES", "1")
    a, b = _twin_envs(len(lays), cfg, lays, budget, gpu_device, max_cams=mc, max_guards=mg, max_path=16)
    n, K = len(lays), 20
    acts_d = acts[:K].to(gpu_device)
    out = torch.empty((K, n, 16), dtype=torch.int32, device=gpu_device)
    rec, _, _, _, r64 = a.step_multi_records(acts_d, records_out=out)
    assert rec.data_ptr() == out.data_ptr() and r64 is None
    back = CompactObs.of_env(a, rec).expand()
    want = torch.stack([b.step(acts_d[k])[0].clone() for k in range(K)]).reshape(-1, 3, 20, 20)
    assert torch.equal(back.view(torch.int32), want.view(torch.int32))
    with pytest.raises(ValueError):
        a.step_multi_records(acts_d[:, :n - 1])
    with pytest.raises(ValueError):
        a.step_multi_records(acts_d, records_out=out[:, :, :15])
    with pytest.raises(ValueError):
        a.step_multi_records(acts_d, records_out=torch.empty((K * n * 16 + 1,), dtype=torch.int32,
                                                             device=gpu_device)[1:].view(K, n, 16))
    lib = nat.lib()
    with torch.cuda.device(gpu_device):
        args = [nat.ptr(acts_d), nat.ptr(out), nat.ptr(torch.empty((K, n), device=gpu_device)), None,
                nat.ptr(torch.empty((K, n), dtype=torch.uint8, device=gpu_device)),
                nat.ptr(torch.empty((K, n), dtype=torch.int8, device=gpu_device)), 1, None, a._stream()]
        assert lib.heist_step_multi_records(a._h, 0, *args) == HEIST_EINVAL
        assert lib.heist_step_multi_records(a._h, 1025, *args) == HEIST_EINVAL
        assert lib.heist_step_multi_records(a._h, K, args[0], None, *args[2:]) == HEIST_EINVAL
        assert lib.heist_step_multi_records(a._h, K, args[0], nat._vp(out.data_ptr() + 4), *args[2:]) == HEIST_EINVAL
    a.close()
    b.close()


def test_replay_tool_records_switch(gpu_device, monkeypatch, tmp_path, capsys):
    """tools/replay_env.py --records prints what the tool prints without it."""
    import os
    cfg, lays, budget, mc, mg, acts, _, _, _ = _case("fan20", True)
    a, _ = _twin_envs(len(lays), cfg, lays, budget, gpu_device, max_cams=mc, max_guards=mg, max_path=16)
    a.step_multi_records(acts[:5].to(gpu_device))
    path = str(tmp_path / "batch.pt")
    a.save_state().save(path)
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import replay_env
    e = 7
    argv = [path, "--env", str(e), "--actions", ",".join(str(int(x)) for x in acts[5:25, e]), "--auto-reset",
            "--device", str(gpu_device)]
    capsys.readouterr()
    replay_env.main(argv)
    plain = capsys.readouterr().out
    replay_env.main(argv + ["--records"])
    assert capsys.readouterr().out == plain and plain.count(" action ") == 20
    a.close()
