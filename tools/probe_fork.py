"""Timing probe of the fork inside a handle (heist_state_fork) against a save + load of the same
envs, HIP events after a settle, three rounds, the sides alternating in one process (the
conventions and the two configurations of tools/probe_env_state.py).  Of 4,096 envs the first
half are sources and the second half destinations.  One JSON line with, per config:

  fork_copy_us     (a) one fork of 2,048 items into destinations that hold other layouts: the
                   sources rotate from call to call, so every call copies the cone blocks
  fork_keep_us     (b) the same fork repeated: the destinations hold the layout, cones are kept
  fork_one_us          the same call with one item: the launches' floor (the fork kernel, then the
                   dispatch-order kernel over all envs), so (b) minus it is the 2,048 items' work
  save_load_us     (c) heist_state_save of the sources + heist_state_load into the destinations
  step5_us         (d) one K = 5 heist_step_multi launch of the whole handle, launches back to back
  fork_step5_us        the search loop: fork (b), then that launch; minus fork_keep_us it is
  step5_after_fork_us  the launch behind a fork, which finds the fan table stale and refills it
  status_copy / status_keep   how many items of the last call of (a) / (b) gave status 0, 1, 2, 3

  c2_20x20   BASELINE C2: the fixed Architect checkpoint's layouts, budget 15
  c5_32x32   BASELINE C5's layouts (exactly 4 cameras + 3 guards, budget 40) at 4,096 envs
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-project-heist-architect-adversarial-reinforcement-learning-framework-cse4019_amd"),
                os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402

from heist_amd import EnvironmentConfig, HeistEnv  # noqa: E402
from heist_amd import _native as nat  # noqa: E402
from heist_amd.layouts import architect_checkpoint_layouts, valid_synthetic_layouts  # noqa: E402
from heist_amd.vec_env import LayoutBatch  # noqa: E402
from probe_env_state import timed  # noqa: E402

K = 5


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
    half = n // 2
    L, s, h = nat.lib(), torch.cuda.current_stream(dev).cuda_stream, env._h
    dst = torch.arange(half, n, dtype=torch.int32, device=dev)
    rot = [((torch.arange(half, dtype=torch.int32) + 97 * r) % half).to(dev) for r in range(8)]
    status = torch.zeros(half, dtype=torch.uint8, device=dev)
    blobs = torch.empty((half, env.state_config()["bytes"]), dtype=torch.uint8, device=dev)
    calls = [0]

    def fork_copy():
        calls[0] += 1
        L.heist_state_fork(h, rot[calls[0] % len(rot)].data_ptr(), dst.data_ptr(), half, status.data_ptr(), s)

    fork_keep = lambda: L.heist_state_fork(h, rot[0].data_ptr(), dst.data_ptr(), half, status.data_ptr(), s)  # noqa: E731

    fork_one = lambda: L.heist_state_fork(h, rot[0].data_ptr(), dst.data_ptr(), 1, status.data_ptr(), s)  # noqa: E731

    def save_load():
        L.heist_state_save(h, rot[0].data_ptr(), half, blobs.data_ptr(), s)
        L.heist_state_load(h, dst.data_ptr(), half, blobs.data_ptr(), half, None, status.data_ptr(), s)

    acts = torch.randint(0, 5, (K, n), device=dev)
    obs = torch.empty((K, n, 3, R, R), dtype=torch.float32, device=dev)
    rew = torch.empty((K, n), dtype=torch.float32, device=dev)
    done = torch.empty((K, n), dtype=torch.uint8, device=dev)
    stat = torch.empty((K, n), dtype=torch.int8, device=dev)
    step5 = env.step_multi_launcher(K, acts, obs, rew, done, stat, True)

    def fork_step5():
        fork_keep()
        step5()

    # the fork against the blob route, once, before any timing
    save_load()
    want = env.save_state().blobs.clone()
    fork_copy()
    fork_keep()
    assert torch.equal(env.save_state().blobs, want)

    def histogram():
        return torch.bincount(status.long(), minlength=4).cpu().tolist()

    out = {"n_envs": n, "items": half, "grid": R, "budget": budget, "max_cams": env.max_cams, "max_guards": env.max_guards,
           "max_path": env.max_path, "bytes_per_env": int(blobs.shape[1]),
           "guards_total": int(env.export()["n_guards"][:half].sum()),
           "fork_copy_us": [], "fork_keep_us": [], "fork_one_us": [], "save_load_us": [], "step5_us": [], "fork_step5_us": []}
    for _ in range(3):
        out["fork_copy_us"].append(timed(dev, fork_copy, 200) * 1e3)
        out["status_copy"] = histogram()
        fork_keep()
        out["fork_keep_us"].append(timed(dev, fork_keep, 200) * 1e3)
        out["status_keep"] = histogram()
        out["fork_one_us"].append(timed(dev, fork_one, 200) * 1e3)
        out["save_load_us"].append(timed(dev, save_load, 100) * 1e3)
        assert bool(status.all())
        out["step5_us"].append(timed(dev, step5, 200) * 1e3)
        fork_keep()
        out["fork_step5_us"].append(timed(dev, fork_step5, 200) * 1e3)
    out["step5_after_fork_us"] = [a - b for a, b in zip(out["fork_step5_us"], out["fork_keep_us"])]
    env.close()
    return out


def main():
    dev = torch.device("cuda:0")
    res = {"c2_20x20": probe(dev, 20, 15, "architect"), "c5_32x32": probe(dev, 32, 40, "synthetic")}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
