"""Timing probe of the env state blobs (heist_state_save / heist_state_load), HIP events after a
settle, three rounds, the sides alternating in one process.  One JSON line with, per config:

  save_us, load_us        one call over all 4,096 envs (the bound C function on resolved pointers)
  bytes_per_env, *_TBps   blob bytes and blob bytes moved per second (a load also rebuilds the
                          guard cone cache, recomputes the dispatch order: three more launches)
  set_layout_reset_us     one heist_set_layout + heist_reset of the same batch on the same build:
                          what a load replaces on resume

  c2_20x20   BASELINE C2: the fixed Architect checkpoint's layouts, budget 15
  c5_32x32   BASELINE C5's layouts (exactly 4 cameras + 3 guards, budget 40) at 4,096 envs
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-project-heist-architect-adversarial-reinforcement-learning-framework-cse4019_amd")]
import torch  # noqa: E402

from heist_amd import EnvironmentConfig, HeistEnv  # noqa: E402
from heist_amd import _native as nat  # noqa: E402
from heist_amd.layouts import architect_checkpoint_layouts, valid_synthetic_layouts  # noqa: E402
from heist_amd.vec_env import LayoutBatch  # noqa: E402


def timed(dev, fn, reps, settle_ms=100.0):
    """ms per call of fn over reps calls, after settle_ms of the same calls."""
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < settle_ms:
        fn()
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / reps


def probe(dev, R, budget, which, n=4096):
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=R, architect_budget=budget)
    env = HeistEnv(n, cfg, max_cams=max(1, budget // 3), max_guards=max(1, budget // 5), max_path=16, device=dev)
    if which == "architect":
        lb, _ = architect_checkpoint_layouts(env, budget, 1234, os.path.join(ROOT, "checkpoints", "architect_c2_fixed.pt"))
    else:
        lays = valid_synthetic_layouts(env, budget, seed=99, n_cams=4, n_guards=3)
        lb = LayoutBatch.from_lists(lays, budget, env.max_cams, env.max_guards, env.max_path, dev, R, R)
    env.set_layout_batch(lb)
    env.reset()
    env.step_multi(torch.randint(0, 5, (17, n), device=dev))  # a state in mid-episode
    st = env.save_state()
    before = env.export(grid=True)
    assert bool(env.load_state(st).all())
    after = env.export(grid=True)
    assert all(torch.equal(before[k], after[k]) for k in before)
    L, s, h = nat.lib(), torch.cuda.current_stream(dev).cuda_stream, env._h
    blobs, status = st.blobs, torch.zeros(n, dtype=torch.uint8, device=dev)
    save = lambda: L.heist_state_save(h, None, n, blobs.data_ptr(), s)  # noqa: E731
    load = lambda: L.heist_state_load(h, None, n, blobs.data_ptr(), n, None, status.data_ptr(), s)  # noqa: E731

    def relayout():
        env.set_layout_batch(lb)
        env.reset()

    nb = int(blobs.shape[1])
    out = {"n_envs": n, "grid": R, "budget": budget, "max_cams": env.max_cams, "max_guards": env.max_guards,
           "max_path": env.max_path, "bytes_per_env": nb, "guards_total": int(before["n_guards"].sum()),
           "save_us": [], "load_us": [], "set_layout_reset_us": []}
    for _ in range(3):
        out["save_us"].append(timed(dev, save, 200) * 1e3)
        out["load_us"].append(timed(dev, load, 100) * 1e3)
        out["set_layout_reset_us"].append(timed(dev, relayout, 100) * 1e3)
    assert bool(status.all())
    out["save_TBps"] = [n * nb / (u * 1e-6) / 1e12 for u in out["save_us"]]
    out["load_TBps"] = [n * nb / (u * 1e-6) / 1e12 for u in out["load_us"]]
    env.close()
    return out


def main():
    dev = torch.device("cuda:0")
    res = {"c2_20x20": probe(dev, 20, 15, "architect"), "c5_32x32": probe(dev, 32, 40, "synthetic")}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
