"""Timing probe of the compact observation records (heist_obs_pack / heist_obs_expand,
AdversarialTrainer(obs_storage="compact")), HIP events after a warm-up, the two sides of every
comparison alternating in one process.  One JSON line:

  pack        heist_obs_pack on one tick's [4096, 3, 20, 20] rows beside heist_step alone
              (synthetic layouts, budget 15), and both in the rollout's order (step, pack); the
              kernel without HeistEnv.pack_obs's host path, and per tick of one 32-tick launch
  expand      heist_obs_expand of a 16,384-sample minibatch drawn from a [32, 4096] rollout
              buffer beside states[b] on the full float32 buffer for the same b
  train       train_iteration seconds and torch.cuda.max_memory_allocated, obs_storage "full"
              against "compact": the default cadence at 4096 envs, T = 32, and
              solver_cadence="layout_batch" at PROBE_LB_N envs (default 512) with 5 attempts
"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-project-heist-architect-adversarial-reinforcement-learning-framework-cse4019_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from heist_amd import CompactObs, EnvironmentConfig, HeistEnv  # noqa: E402
from heist_amd.layouts import synthetic_layouts  # noqa: E402
from heist_amd.training import AdversarialTrainer  # noqa: E402


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


def probe_kernels(dev):
    n, T, mb = 4096, 32, 16384
    env = HeistEnv(n, EnvironmentConfig(), max_cams=5, max_guards=3, device=dev)
    env.set_layouts(synthetic_layouts(n, 20, 20, 15, seed=7), budget=15)
    env.reset()
    acts = torch.randint(0, 5, (T, n), device=dev)
    full = torch.empty((T, n, 3, 20, 20), dtype=torch.float32, device=dev)
    for t in range(T):
        env.step(acts[t], obs_out=full[t])
    rec = env.pack_obs(full)
    co = CompactObs.of_env(env, rec)
    one = torch.empty_like(rec[0])
    k = [0]

    def step():
        k[0] += 1
        env.step(acts[k[0] % T])

    def step_pack():
        step()
        env.pack_obs(env.obs, out=one)

    # the pack kernel without pack_obs's Python path (its checks and the device guard are ~10 us
    # of host time per call, which back-to-back calls of a ~3 us kernel measure instead of it):
    # the bound C function on resolved pointers, and one launch over the buffer's T * n rows
    from heist_amd import _native as nat
    fn, st = nat.lib().heist_obs_pack, torch.cuda.current_stream(dev).cuda_stream
    raw = lambda: fn(env.obs.data_ptr(), n, 20, 20, 18, 18, one.data_ptr(), st)  # noqa: E731
    bulk = lambda: fn(full.data_ptr(), T * n, 20, 20, 18, 18, rec.data_ptr(), st)  # noqa: E731
    pack = {"step_us": [], "pack_us": [], "step_then_pack_us": [], "pack_raw_call_us": [], "pack_bulk_us_per_tick": []}
    for _ in range(3):
        pack["pack_raw_call_us"].append(timed(dev, raw, 400) * 1e3)
        pack["pack_bulk_us_per_tick"].append(timed(dev, bulk, 50) * 1e3 / T)
        pack["step_us"].append(timed(dev, step, 400) * 1e3)
        pack["pack_us"].append(timed(dev, lambda: env.pack_obs(env.obs, out=one), 400) * 1e3)
        pack["step_then_pack_us"].append(timed(dev, step_pack, 400) * 1e3)
    flat = full.reshape(T * n, 3, 20, 20)
    b = torch.randperm(T * n, device=dev)[:mb]
    assert torch.equal(co.expand(b).view(torch.int32), flat[b].view(torch.int32))
    expand = {"expand_us": [], "gather_full_us": [], "samples": mb, "bytes_stored": mb * 4800}
    for _ in range(3):
        expand["expand_us"].append(timed(dev, lambda: co.expand(b), 100) * 1e3)
        expand["gather_full_us"].append(timed(dev, lambda: flat[b], 100) * 1e3)
    env.close()
    return {"pack": pack, "expand": expand}


def probe_train(dev, cadence, n, T, A, iters):
    rows = {}
    # PROBE_ORDER: the trainers are built one after the other in one process, and a later one can
    # run a few percent slower whatever it stores; run both orders before reading a difference
    for storage in os.environ.get("PROBE_ORDER", "full,compact,full,compact").split(","):
        d = tempfile.mkdtemp()
        tr = AdversarialTrainer(EnvironmentConfig(), solver_episodes_per_layout=A, total_episodes=10 ** 9, save_dir=d,
                                log_dir=d, n_envs=n, rollout_len=T, minibatch=16384, device=dev, seed=0,
                                solver_cadence=cadence, obs_storage=storage)
        tr.global_episode = 200
        tr._assign_layouts(np.arange(n))
        tr.train_iteration()  # warm-up: code objects, MIOpen's choices, the allocator's pools
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        secs, ticks = [], []
        for _ in range(iters):
            t0 = time.perf_counter()
            out = tr.train_iteration()
            torch.cuda.synchronize(dev)
            secs.append(time.perf_counter() - t0)
            ticks.append(int(out.get("rollout_ticks", T)))
        rows.setdefault(storage, []).append({"iteration_s": secs, "rollout_ticks": ticks,
                                             "max_memory_allocated": int(torch.cuda.max_memory_allocated(dev)),
                                             "allocated_before": int(base)})
        tr.env.close()
        del tr
        torch.cuda.empty_cache()
    return {"n_envs": n, "T": T, "attempts": A, "runs": rows}


def main():
    dev = torch.device("cuda:0")
    res = {}
    which = os.environ.get("PROBE_PARTS", "kernels,rollout,layout_batch").split(",")
    if "kernels" in which:
        res.update(probe_kernels(dev))
    if "rollout" in which:
        res["train_rollout"] = probe_train(dev, "rollout", 4096, 32, 4, 3)
    if "layout_batch" in which:
        res["train_layout_batch"] = probe_train(dev, "layout_batch", int(os.environ.get("PROBE_LB_N", "512")), 32, 5, 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
