"""heist_step_multi against heist_step_multi_records (the K-tick kernels emitting compact records
instead of observation rows), same process, same handle, HIP events.

  python tools/probe_step_records.py            # bench.py's headline: C2, 4,096 envs of 20 x 20, K = 20
  python tools/probe_step_records.py --c5       # bench.py --full's C5: 2,048 envs of 32 x 32, 4 cameras + 3 guards

After a warm-up and a clock-settle phase the two forms alternate, five windows each; a window is
bench.py's (time_env): the fan table marked stale, `warmup` untimed ticks that refill it, then
`steps` ticks in K-tick launches between two events.  Both forms advance the same envs, so window
i of one form and window i of the other start from states one window apart.  Prints one JSON line:
per-tick medians, the windows, their spread, and the device bytes of the outputs per launch.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-project-heist-architect-adversarial-reinforcement-learning-framework-cse4019_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from heist_amd import EnvironmentConfig, HeistEnv, _native as nat  # noqa: E402
from heist_amd.layouts import valid_synthetic_layouts  # noqa: E402
from heist_amd.obs_compact import record_words  # noqa: E402

WINDOWS = 5


def make_env(dev, c5, n):
    R, budget = (32, 40) if c5 else (20, 15)
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=R, max_steps=200, architect_budget=budget)
    env = HeistEnv(n, cfg, max_cams=max(1, budget // 3), max_guards=max(1, budget // 5), max_path=16, device=dev,
                   auto_reset=True)
    if c5:
        valid_synthetic_layouts(env, budget, seed=99, n_cams=4, n_guards=3)
    else:
        bench.architect_layouts(env, budget, seed=1234)
    env.reset()
    return env


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--c5", action="store_true")
    ap.add_argument("--envs", type=int, default=None)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--ticks-per-launch", type=int, default=20)
    ap.add_argument("--settle-launches", type=int, default=64)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    N = args.envs or (2048 if args.c5 else 4096)
    K, steps, warmup = args.ticks_per_launch, args.steps, args.warmup
    env = make_env(dev, args.c5, N)
    kc = env.kernel_config()
    assert env.records_direct == 1, kc
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)
    actions = torch.randint(0, 5, (warmup + steps, N), device=dev, generator=gen, dtype=torch.int64)
    W = record_words(env.rows, env.cols)
    obs = torch.empty((K, N, 3, env.rows, env.cols), dtype=torch.float32, device=dev)
    rec = torch.empty((K, N, W), dtype=torch.int32, device=dev)
    rew = torch.empty((K, N), device=dev)
    done = torch.empty((K, N), dtype=torch.uint8, device=dev)
    status = torch.empty((K, N), dtype=torch.int8, device=dev)
    stream = torch.cuda.current_stream(dev)
    lib = nat.lib()

    def launcher(form, k0, k):  # every argument resolved now: the timed loop only issues launches
        a = actions[k0:k0 + k].data_ptr()
        if form == "obs":
            args_ = (env._h, k, a, obs.data_ptr(), rew.data_ptr(), None, done.data_ptr(), status.data_ptr(), 1,
                     stream.cuda_stream)
            fn = lib.heist_step_multi
        else:
            args_ = (env._h, k, a, rec.data_ptr(), rew.data_ptr(), None, done.data_ptr(), status.data_ptr(), 1, None,
                     stream.cuda_stream)
            fn = lib.heist_step_multi_records

        def launch():
            rc = fn(*args_)
            if rc:
                nat.check(rc, fn.__name__)
        return launch

    def prepare(form, k0, n):
        return [launcher(form, k0 + j, min(K, n - j)) for j in range(0, n, K)]

    def window(form):
        env.set_ray_mode(kc["ray_mode"])  # marks the fan table stale, as bench.py's windows do
        for launch in prepare(form, 0, warmup):
            launch()
        ready = prepare(form, warmup, steps)
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for launch in ready:
            launch()
        b.record(stream)
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / steps * 1e3  # us per tick

    for form in ("obs", "records"):
        for launch in prepare(form, 0, warmup):
            launch()
    settle = prepare("obs", 0, K) + prepare("records", 0, K)
    for i in range(args.settle_launches):
        settle[i & 1]()
        if i % 16 == 15:
            torch.cuda.synchronize(dev)
    torch.cuda.synchronize(dev)
    us = {"obs": [], "records": []}
    for _ in range(WINDOWS):
        for form in ("obs", "records"):
            us[form].append(window(form))
    out = {"config": "c5_32x32" if args.c5 else "c2_20x20", "envs": N, "ticks_per_launch": K, "steps": steps,
           "kernel": bench.multi_kernel_name(kc, env.rows, env.cols), "lean_waves": kc["lean_waves"],
           "output_bytes_per_launch": {"obs": obs.numel() * 4, "records": rec.numel() * 4}}
    for form, v in us.items():
        out[form] = {"us_per_tick_median": statistics.median(v), "us_per_tick_min": min(v), "us_per_tick_max": max(v),
                     "spread_frac": (max(v) - min(v)) / statistics.median(v), "windows_us_per_tick": v}
    out["records_over_obs"] = out["records"]["us_per_tick_median"] / out["obs"]["us_per_tick_median"]
    env.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
