"""The exact planner (heist_plan, HeistEnv.plan) on a batch of layouts: what share of them the
Solver can finish undetected, in how many ticks at best, how many pass the BFS check and are
unsolvable all the same -- and what the launch costs next to heist_step_multi_records, the
existing launch that casts the same rays, same process, same handle, HIP events.

  python tools/plan_env.py                       # bench.py's C2: 4,096 envs of 20 x 20, Architect layouts, horizon 200
  python tools/plan_env.py --layouts synthetic   # random layouts instead of the checkpoint's
  python tools/plan_env.py --layouts empty       # no walls, cameras or guards: every env plans exactly its
                                                 # Manhattan distance in ticks, none casts a ray -- the cost
                                                 # of the prologue, the DP step and the row stores alone
  python tools/plan_env.py --ckpt checkpoints/architect_ep500.pt
  python tools/plan_env.py --field               # the planner field (heist_plan_field, HeistEnv.plan_field) next to
                                                 # heist_plan on the three batches above, one JSON line each,
                                                 # also written to profiles/plan_field.log (--out)
  python tools/plan_env.py --field --all-ticks   # ... and the launch that writes every tick's field as well
  python tools/plan_env.py --value [--gamma G] [--all-ticks]
                                                 # the planner value (heist_plan_value, HeistEnv.plan_value) next to
                                                 # heist_plan_field, same protocol, plus the histogram of the start
                                                 # cell's value, the share of envs whose return-optimal episode
                                                 # (follow_value replayed) is longer than plan().ticks and the mean
                                                 # of value[start] minus the fastest plan's return; also written
                                                 # to profiles/plan_value.log
  python tools/plan_env.py --play [--noise P] [--gamma G]
                                                 # the planner playout (heist_plan_play, HeistEnv.plan_play) on the
                                                 # Architect batch: with and without records, at noise 0 and P, next
                                                 # to the path it replaces (follow_value + step_multi_records on a
                                                 # twin handle restored from the saved state + value_targets) and to
                                                 # heist_plan_value itself; also written to profiles/plan_play.log
  python tools/plan_env.py --q [--noise P] [--gamma G]
                                                 # the planner Q (heist_plan_q, HeistEnv.plan_q) on the states of a
                                                 # noisy table play, K = horizon, on the three batches: the launch,
                                                 # search.q_values on the same device tensors and the
                                                 # plan_value(all_ticks=True) launch that makes its inputs; also
                                                 # written to profiles/plan_q.log
  python tools/plan_env.py --ablate [--gamma G]   # the planner what-if (heist_plan_masked, HeistEnv.plan_ablate) on the
                                                 # three batches: every emitter switched off in turn, M = 1 + n_slot
                                                 # variants per env in one launch -- the histograms of critical and
                                                 # redundant emitters per layout, the share of unsolvable layouts with
                                                 # and without a critical emitter, and the launch next to the route it
                                                 # replaces, M x (heist_plan_field + heist_plan_value); also written to
                                                 # profiles/plan_masked.log
  python tools/plan_env.py --place [--gamma G]    # the planner placement (heist_plan_place, HeistEnv.plan_place) on the
                                                 # Architect batch: the launch at 8 candidate cameras per env next to
                                                 # heist_plan_masked with 8 all-on masks and to the route without it
                                                 # (set_layout_batch + reset + plan_field + plan_value on a twin handle,
                                                 # one candidate per env per pass), then a full placement_scan of 64
                                                 # envs x every interior cell x 8 headings with its headroom, blocking
                                                 # and relocation-rank figures; also written to profiles/plan_place.log
  python tools/plan_env.py --place-guard [--gamma G]  # the guard placement (heist_plan_place_guard) on the Architect
                                                 # batch: 8 Architect guards per env next to heist_plan_place with 8
                                                 # cameras and to the twin-handle route, then a full guard scan of 64
                                                 # envs with headroom per budget point next to the best camera's; also
                                                 # written to profiles/plan_place_guard.log
  python tools/plan_env.py --walls [--gamma G]   # the planner walls (heist_plan_walls, HeistEnv.plan_walls) on the
                                                 # Architect batch: 8 wall adds per env next to the same launch without
                                                 # edits, to heist_plan_masked on a handle without the guard cone cache
                                                 # and to the twin-handle route, then a full wall_placement_scan of 64
                                                 # envs and the wall ablation of the batch; also written to
                                                 # profiles/plan_walls.log

The planner only reads the envs, so every timed launch does the same work from the same state
(fresh after reset): `--warmup` untimed launches, then `--runs` launches each between two events;
the median is reported.  The records launches (K = horizon ticks of random actions, auto-reset)
follow on the same handle, timed the same way.  Prints one JSON line.
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
from heist_amd import EnvironmentConfig, HeistEnv  # noqa: E402
from heist_amd.layouts import valid_synthetic_layouts  # noqa: E402


def timed(dev, fn, warmup, runs):
    """Milliseconds of each of `runs` calls of fn (one launch each), after `warmup` untimed ones."""
    stream = torch.cuda.current_stream(dev)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        torch.cuda.synchronize(dev)
        ms.append(a.elapsed_time(b))
    return ms


def make_env(args, kind, dev):
    """A reset handle of args.envs envs under `kind` layouts (architect, synthetic, empty)."""
    R, N, budget = args.grid, args.envs, args.budget
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=R, max_steps=args.max_steps, architect_budget=budget)
    env = HeistEnv(N, cfg, max_cams=max(1, budget // 3), max_guards=max(1, budget // 5), max_path=16, device=dev,
                   auto_reset=True)
    if kind == "architect":
        bench.architect_layouts(env, budget, seed=args.seed, ckpt=args.ckpt)
    elif kind == "synthetic":
        valid_synthetic_layouts(env, budget, seed=args.seed)
    else:
        env.set_layouts([([], [], [])] * N, budget=budget)
    env.reset()
    return env


def field_table(args, dev):
    """heist_plan_field next to heist_plan, same handle, same process, same state (both only read
    the envs): one JSON line per batch."""
    H = min(args.horizon or args.max_steps, 1024)
    lines = []
    for kind in ("architect", "empty", "synthetic"):
        env = make_env(args, kind, dev)
        kc = env.kernel_config()
        assert env.plan_field_supported == 1, kc
        res, f = env.plan(H), env.plan_field(H)
        sr, sc = env.config.start_pos
        ok = res.ticks > 0
        walls = env.grid_snapshot() == 1
        out = {"config": "%dx%d" % (args.grid, args.grid), "envs": args.envs, "layouts": kind, "horizon": H,
               "multi_waves": kc["multi_waves"], "solvable_frac": float(ok.float().mean()),
               "field_at_start_equals_plan": bool(torch.equal(f.togo[:, sr, sc].int(), res.ticks)),
               "winnable_cell_frac": float((f.togo > 0).sum()) / float((~walls).sum()),
               "togo_max": int(f.togo.max())}
        p = statistics.median(timed(dev, lambda: env.plan(H), args.warmup, args.runs))
        ms = timed(dev, lambda: env.plan_field(H), args.warmup, args.runs)
        m = statistics.median(ms)
        out["plan_launch_ms_median"] = p
        out["field"] = {"launch_ms_median": m, "launch_ms": ms, "us_per_tick_of_horizon": m / H * 1e3,
                        "ns_per_env_tick": m * 1e6 / (H * args.envs), "over_plan": m / p}
        if args.all_ticks:
            ms = timed(dev, lambda: env.plan_field(H, all_ticks=True), args.warmup, args.runs)
            a = statistics.median(ms)
            out["field_all_ticks"] = {"launch_ms_median": a, "launch_ms": ms, "over_field": a / m,
                                      "togo_ticks_mb": H * args.envs * args.grid * args.grid * 2 / 1e6}
        env.close()
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("$ python tools/plan_env.py --field%s\n" % (" --all-ticks" if args.all_ticks else ""))
        fh.write("\n".join(lines) + "\n")


def value_table(args, dev):
    """heist_plan_value next to heist_plan_field, same handle, same process, same state (both only
    read the envs): one JSON line per batch."""
    from heist_amd.search import discounted_return, follow_value
    H = min(args.horizon or args.max_steps, 1024)
    lines = []
    for kind in ("architect", "empty", "synthetic"):
        env = make_env(args, kind, dev)
        kc = env.kernel_config()
        assert env.plan_value_supported == 1, kc
        N = args.envs
        sr, sc = env.config.start_pos
        res = env.plan(H)
        ok = res.ticks > 0
        # the fastest plan's return and the value's own play, both through the env kernels on a
        # second handle with the same layouts (the timed handle stays fresh after reset); in chunks,
        # value_ticks being 8 H N R C bytes
        twin = make_env(args, kind, dev)
        _, _, fdone, _, fr64 = twin.step_multi_records(res.actions, auto_reset=False, reward64=True)
        fast_ret = discounted_return(fr64, fdone, args.gamma)
        twin.close()
        v0 = torch.empty(N, dtype=torch.float64, device=dev)
        ep = torch.empty(N, dtype=torch.int64, device=dev)
        replay_ok = True
        step = max(1, min(N, 512))
        for lo in range(0, N, step):
            ids = list(range(lo, min(lo + step, N)))
            part = HeistEnv(len(ids), env.config, max_cams=env.max_cams, max_guards=env.max_guards,
                            max_path=env.max_path, device=dev, auto_reset=False)
            assert bool(part.load_state(env.save_state(ids)).all())
            pv = part.plan_value(H, gamma=args.gamma, all_ticks=True)
            start_r = torch.full((len(ids),), sr, dtype=torch.int64, device=dev)
            acts = follow_value(pv, start_r, torch.full_like(start_r, sc))
            _, _, done, _, r64 = part.step_multi_records(acts, auto_reset=False, reward64=True)
            v0[lo:lo + len(ids)] = pv.value[:, sr, sc]
            ep[lo:lo + len(ids)] = done.int().argmax(0) + 1
            replay_ok &= bool(torch.equal(discounted_return(r64, done, args.gamma).view(torch.int64),
                                          pv.value[:, sr, sc].contiguous().view(torch.int64)))
            part.close()
            del pv
        hist = {}
        for v in v0.cpu().tolist():
            lo = int(v // 2 * 2)
            hist["%d..%d" % (lo, lo + 2)] = hist.get("%d..%d" % (lo, lo + 2), 0) + 1
        out = {"config": "%dx%d" % (args.grid, args.grid), "envs": N, "layouts": kind, "horizon": H,
               "gamma": args.gamma, "multi_waves": kc["multi_waves"], "solvable_frac": float(ok.float().mean()),
               "replayed_return_equals_value_bitwise": replay_ok,
               "value_at_start": {"mean": float(v0.mean()), "min": float(v0.min()), "max": float(v0.max()),
                                  "histogram": dict(sorted(hist.items(), key=lambda kv: float(kv[0].split("..")[0])))},
               "optimal_episode_ticks_mean": float(ep.float().mean()),
               "optimal_episode_longer_than_fastest_plan_frac":
                   float((ep[ok] > res.ticks[ok]).float().mean()) if bool(ok.any()) else None,
               "optimal_episode_longer_frac_of_all_envs": float(((ep > res.ticks) & ok).float().mean()),
               "value_minus_fastest_plan_return_mean":
                   float((v0[ok] - fast_ret[ok]).mean()) if bool(ok.any()) else None}
        f = statistics.median(timed(dev, lambda: env.plan_field(H), args.warmup, args.runs))
        ms = timed(dev, lambda: env.plan_value(H, gamma=args.gamma), args.warmup, args.runs)
        m = statistics.median(ms)
        out["field_launch_ms_median"] = f
        out["value"] = {"launch_ms_median": m, "launch_ms": ms, "us_per_tick_of_horizon": m / H * 1e3,
                        "ns_per_env_tick": m * 1e6 / (H * N), "over_field": m / f, "minus_field_ms": m - f}
        if args.all_ticks:
            ms = timed(dev, lambda: env.plan_value(H, gamma=args.gamma, all_ticks=True), args.warmup, args.runs)
            a = statistics.median(ms)
            out["value_all_ticks"] = {"launch_ms_median": a, "launch_ms": ms, "over_value": a / m,
                                      "value_ticks_mb": H * N * args.grid * args.grid * 8 / 1e6,
                                      "action_ticks_mb": H * N * args.grid * args.grid / 1e6}
        env.close()
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    out_path = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "plan_value.log")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("$ python tools/plan_env.py --value --gamma %r%s\n" % (args.gamma, " --all-ticks" if args.all_ticks else ""))
        fh.write("\n".join(lines) + "\n")


def play_table_mode(args, dev):
    """heist_plan_play next to the Python path it replaces and to heist_plan_value, same process,
    same handle (all of them only read it; the replay runs on a twin restored from its state)."""
    from heist_amd.search import follow_value, value_targets
    H = min(args.horizon or args.max_steps, 1024)
    N, R = args.envs, args.grid
    env = make_env(args, args.layouts, dev)
    kc = env.kernel_config()
    assert env.plan_value_supported == 1, kc
    sr, sc = env.config.start_pos
    nvis = (R * R + 31) // 32
    pv = env.plan_value(H, gamma=args.gamma, all_ticks=True)
    state = env.save_state()
    twin = HeistEnv(N, env.config, max_cams=env.max_cams, max_guards=env.max_guards, max_path=env.max_path, device=dev,
                    auto_reset=False)
    start_r = torch.full((N,), sr, dtype=torch.int64, device=dev)
    start_c = torch.full_like(start_r, sc)

    def python_path():
        acts = follow_value(pv, start_r, start_c)
        twin.load_state(state)
        rec, _, done, status, r64 = twin.step_multi_records(acts, auto_reset=False, reward64=True)
        word = rec[:, :, nvis].long()
        pos_r = torch.cat([start_r[None], (word & 0xFF)[:-1]])
        pos_c = torch.cat([start_c[None], ((word >> 8) & 0xFF)[:-1]])
        return acts, rec, r64, done, status, value_targets(pv, pos_r, pos_c)

    out = {"config": "%dx%d" % (R, R), "envs": N, "layouts": args.layouts, "horizon": H, "gamma": args.gamma,
           "multi_waves": kc["multi_waves"], "noise": args.noise}
    ref = python_path()
    p0 = env.plan_play(pv.action_ticks, pv.vis, values=pv.value_ticks, noise=0.0, seed=args.seed)
    played = torch.arange(H, device=dev).reshape(H, 1) < p0.length.reshape(1, N)
    out["noise0_equals_python_path"] = bool(
        torch.equal(p0.actions, ref[0]) and torch.equal(p0.records[played], ref[1][played])
        and torch.equal(p0.reward64.view(torch.int64), ref[2].view(torch.int64)) and torch.equal(p0.done, ref[3])
        and torch.equal(p0.status, ref[4]) and torch.equal(p0.value[played].view(torch.int64),
                                                          ref[5][0][played].view(torch.int64)))
    pn = env.plan_play(pv.action_ticks, pv.vis, values=pv.value_ticks, noise=args.noise, seed=args.seed)
    for name, p in (("noise0", p0), ("noisy", pn)):
        last = p.status.gather(0, (p.length.long() - 1).clamp(min=0).reshape(1, N))[0]
        out[name] = {"length_mean": float(p.length.float().mean()),
                     "ended": {k: float((last == v).float().mean())
                               for k, v in (("detected", 1), ("vault_reached", 2), ("timeout", 3))},
                     "steps_off_expert_frac": float(((p.actions != p.expert.long()) & (p.expert >= 0)).sum())
                     / max(1.0, float(p.length.clamp(min=0).sum()))}
    for records in (True, False):
        for noise in (0.0, args.noise):
            ms = timed(dev, lambda: env.plan_play(pv.action_ticks, pv.vis, values=pv.value_ticks, noise=noise,
                                                  seed=args.seed, records=records), args.warmup, args.runs)
            out["play_%s_noise_%g" % ("records" if records else "no_records", noise)] = {
                "launch_ms_median": statistics.median(ms), "launch_ms": ms}
    ms = timed(dev, python_path, args.warmup, args.runs)
    out["python_path"] = {"ms_median": statistics.median(ms), "ms": ms}
    for all_ticks in (False, True):
        ms = timed(dev, lambda: env.plan_value(H, gamma=args.gamma, all_ticks=all_ticks), args.warmup, args.runs)
        out["plan_value_all_ticks" if all_ticks else "plan_value"] = {"launch_ms_median": statistics.median(ms),
                                                                      "launch_ms": ms}
    m = out["play_records_noise_0"]["launch_ms_median"]
    out["python_path_over_play"] = out["python_path"]["ms_median"] / m
    out["play_over_plan_value_all_ticks"] = m / out["plan_value_all_ticks"]["launch_ms_median"]
    env.close()
    twin.close()
    line = json.dumps(out)
    print(line, flush=True)
    out_path = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "plan_play.log")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("$ python tools/plan_env.py --play --noise %r --gamma %r\n" % (args.noise, args.gamma))
        fh.write(line + "\n")


def q_mode(args, dev):
    """heist_plan_q next to its restatement in torch (search.q_values on the same device tensors) and
    to the plan_value(all_ticks=True) launch that makes its inputs, same process, same handle (all
    of them only read it): one JSON line per batch.  The states are those of a noisy table play
    (plan_play at --noise), K = horizon rows."""
    from heist_amd.obs_compact import record_cells
    from heist_amd.search import q_values
    H = min(args.horizon or args.max_steps, 1024)
    N, R = args.envs, args.grid
    lines = []
    for kind in ("architect", "empty", "synthetic"):
        env = make_env(args, kind, dev)
        kc = env.kernel_config()
        assert env.plan_value_supported == 1, kc
        cfg = env.config
        pv = env.plan_value(H, gamma=args.gamma, all_ticks=True)
        play = env.plan_play(pv.action_ticks, pv.vis, noise=args.noise, seed=args.seed)
        x = env.export()
        start = torch.stack([x["pos_r"], x["pos_c"]], 1).to(torch.int32).unsqueeze(0)
        pos = torch.cat([start, record_cells(play.records, R, R)[:-1]]).contiguous()
        taken = play.actions
        valid = torch.arange(H, device=dev).reshape(H, 1) < play.length.reshape(1, N)
        consts = (cfg.reward_step, cfg.reward_detection, cfg.reward_vault)

        def torch_path():
            return q_values(pv.value_ticks, pv.vis, pv.grid, pv.tick, pos, cfg.max_steps, x["initial_dist"],
                            cfg.vault_pos, consts, gamma=args.gamma, taken=taken)

        got, ref = env.plan_q(pv, pos, taken), torch_path()
        same = all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                               b.view(torch.int64) if b.dtype == torch.float64 else b)
                   for a, b in ((getattr(got, f), getattr(ref, f)) for f in env.PLAN_Q_OUTPUTS))
        sets = torch.zeros_like(got.optimal, dtype=torch.int64)
        for a in range(5):
            sets += (got.optimal.long() >> a) & 1
        nd = max(1, int(valid.sum()))
        out = {"config": "%dx%d" % (R, R), "envs": N, "layouts": kind, "horizon": H, "K": H, "gamma": args.gamma,
               "noise": args.noise, "multi_waves": kc["multi_waves"], "states": H * N, "valid_decisions": int(valid.sum()),
               "kernel_equals_q_values_bitwise": bool(same),
               "optimal_rate": float((got.gap[valid] == 0.0).sum()) / nd, "gap_mean": float(got.gap[valid].sum()) / nd,
               "optimal_set_size_mean": float(sets[valid].sum()) / nd,
               "decisions_with_several_optimal_actions_frac": float((sets[valid] >= 2).sum()) / nd}
        del got, ref
        ms = timed(dev, lambda: env.plan_q(pv, pos, taken), args.warmup, args.runs)
        out["plan_q"] = {"launch_ms_median": statistics.median(ms), "launch_ms": ms,
                         "ns_per_state": statistics.median(ms) * 1e6 / (H * N)}
        ms = timed(dev, lambda: env.plan_q(pv, pos, taken, outputs=("optimal", "gap")), args.warmup, args.runs)
        out["plan_q_optimal_gap_only"] = {"launch_ms_median": statistics.median(ms), "launch_ms": ms}
        # the launch alone: 20 back-to-back ctypes calls on buffers made once, between two events,
        # so the host's share of one plan_q() call (allocations, argument checks) is not in it
        from heist_amd import _native as nat
        bufs = env.plan_q(pv, pos, taken)
        fn, P = nat.lib().heist_plan_q, nat.ptr
        raw = (env._h, H, H, float(args.gamma), P(pv.value_ticks), P(pv.vis), P(pv.tick), P(pos), P(taken), P(bufs.q),
               P(bufs.value), P(bufs.best), P(bufs.optimal), P(bufs.gap), env._stream())
        ms = [m / 20 for m in timed(dev, lambda: [fn(*raw) for _ in range(20)], args.warmup, args.runs)]
        out["plan_q_launch_alone"] = {"launch_ms_median": statistics.median(ms), "launch_ms": ms,
                                      "ns_per_state": statistics.median(ms) * 1e6 / (H * N)}
        ms = timed(dev, torch_path, args.warmup, args.runs)
        out["torch_q_values"] = {"ms_median": statistics.median(ms), "ms": ms}
        ms = timed(dev, lambda: env.plan_value(H, gamma=args.gamma, all_ticks=True), args.warmup, args.runs)
        out["plan_value_all_ticks"] = {"launch_ms_median": statistics.median(ms), "launch_ms": ms}
        q = out["plan_q"]["launch_ms_median"]
        out["torch_q_values_over_plan_q"] = out["torch_q_values"]["ms_median"] / q
        out["plan_q_over_plan_value_all_ticks"] = q / out["plan_value_all_ticks"]["launch_ms_median"]
        env.close()
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    out_path = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "plan_q.log")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("$ python tools/plan_env.py --q --noise %r --gamma %r\n" % (args.noise, args.gamma))
        fh.write("\n".join(lines) + "\n")


def ablate_table(args, dev):
    """heist_plan_masked's leave-one-out launch next to M x (heist_plan_field + heist_plan_value), the
    existing route without its set_layout / reset, same handle, same process, same state (all of
    them only read the envs): one JSON line per batch."""
    from heist_amd.search import ablation_masks
    H = min(args.horizon or args.max_steps, 1024)
    N = args.envs
    lines = []
    for kind in ("architect", "empty", "synthetic"):
        env = make_env(args, kind, dev)
        kc = env.kernel_config()
        assert env.plan_masked_supported == 1, kc
        ab = env.plan_ablate(H, gamma=args.gamma)
        M = ab.ticks.shape[1]
        unsolv = ab.ticks[:, 0] < 0
        n_unsolv, n_filled = int(unsolv.sum()), int(ab.filled.sum())
        with_crit = int((unsolv & ab.critical.any(1)).sum())

        def hist(per_env):
            return {str(k): int((per_env == k).sum()) for k in range(int(per_env.max()) + 1)}

        mc = env.max_cams
        f = ab.filled
        out = {"config": "%dx%d" % (args.grid, args.grid), "envs": N, "layouts": kind, "horizon": H, "gamma": args.gamma,
               "multi_waves": kc["multi_waves"], "variants_per_env": M, "filled_emitters": n_filled,
               "solvable_frac": float((~unsolv).float().mean()), "unsolvable_layouts": n_unsolv,
               "unsolvable_with_a_critical_emitter_frac": with_crit / n_unsolv if n_unsolv else None,
               "unsolvable_jointly_blocked_frac": (n_unsolv - with_crit) / n_unsolv if n_unsolv else None,
               "redundant_emitter_frac": int(ab.redundant.sum()) / n_filled if n_filled else None,
               "critical_emitters_per_layout": hist(ab.critical.sum(1)),
               "redundant_emitters_per_layout": hist(ab.redundant.sum(1)),
               "camera_credit_mean": float(ab.credit[:, :mc][f[:, :mc]].mean()) if bool(f[:, :mc].any()) else None,
               "guard_credit_mean": float(ab.credit[:, mc:][f[:, mc:]].mean()) if bool(f[:, mc:].any()) else None,
               "credit_min": float(ab.credit.min()),
               "ticks_saved_mean_where_both_solvable":
                   float(ab.ticks_saved[f & (ab.ticks[:, :1] > 0)].float().mean()) if bool((f & (ab.ticks[:, :1] > 0)).any()) else None}
        del ab
        x = env.export()
        masks = ablation_masks(x["n_cams"], x["n_guards"], env.max_cams, env.max_guards)
        ms = timed(dev, lambda: env.plan_masked(masks, H, gamma=args.gamma), args.warmup, args.runs)
        m = statistics.median(ms)
        ys = timed(dev, lambda: (env.plan_field(H), env.plan_value(H, gamma=args.gamma)), args.warmup, args.runs)
        y = statistics.median(ys) * M
        out["masked"] = {"launch_ms_median": m, "launch_ms": ms, "ns_per_variant_tick": m * 1e6 / (H * N * M)}
        out["yardstick_M_x_field_plus_value"] = {"ms": y, "field_plus_value_ms_median": statistics.median(ys),
                                                 "field_plus_value_ms": ys}
        out["masked_over_yardstick"] = m / y
        env.close()
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    out_path = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "plan_masked.log")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("$ python tools/plan_env.py --ablate --gamma %r\n" % args.gamma)
        fh.write("\n".join(lines) + "\n")


def place_mode(args, dev):
    """heist_plan_place on the Architect batch, one JSON line per row, each with its N, M and device
    seconds per variant: (a) the launch at M = 8 candidates per env, with the same launch on
    candidates that are not valid (no cast: the row copies and the two sweeps alone); (b)
    heist_plan_masked on the same handle with 8 all-on masks, and with 8 all-off masks (the forward
    loop without a ray); (c) the route without the kernel -- the candidates laid into a twin handle
    with one more camera slot by set_layout_batch + reset + plan_field + plan_value, one candidate
    per env per pass; (d) a full placement_scan of 64 envs x every interior cell x 8 headings, with
    the headroom and blocking it finds and the relocation rank of every camera of those layouts."""
    from heist_amd.components.security import Camera
    from heist_amd.search import camera_candidates, placement_scan, relocation_scan
    from heist_amd.vec_env import LayoutBatch
    H = min(args.horizon or args.max_steps, 1024)
    N, R, M = args.envs, args.grid, 8
    ref = Camera(0, 0)
    env = make_env(args, "architect", dev)
    kc = env.kernel_config()
    assert env.plan_place_supported == 1, kc
    head = {"config": "%dx%d" % (R, R), "layouts": "architect", "horizon": H, "gamma": args.gamma,
            "multi_waves": kc["multi_waves"], "camera": [ref.fov_angle, ref.rotation_speed, ref.vision_range]}
    lines = []

    def emit(row):
        lines.append(json.dumps(dict(head, **row)))
        print(lines[-1], flush=True)

    def med(fn, runs=None):
        ms = timed(dev, fn, args.warmup, runs or args.runs)
        return statistics.median(ms), ms

    # (a) M = 8 candidates per env: a random interior cell each, heading 45 m, the reference's camera
    gen = torch.Generator().manual_seed(args.seed)
    cell = torch.randint(1, R - 1, (N, M, 2), generator=gen).double()
    cd = torch.cat([cell, torch.full((N, M, 1), ref.fov_angle, dtype=torch.float64),
                    (45.0 * torch.arange(M, dtype=torch.float64)).reshape(1, M, 1).expand(N, M, 1),
                    torch.full((N, M, 1), ref.rotation_speed, dtype=torch.float64),
                    torch.full((N, M, 1), float(ref.vision_range), dtype=torch.float64)], 2).to(dev)
    base = env.plan_field(H).vis
    pp = env.plan_place(cd, H, gamma=args.gamma, base=base)
    valid, ticks_a, value_a = pp.valid.clone(), pp.ticks.clone(), pp.value.clone()
    del pp
    a, a_ms = med(lambda: env.plan_place(cd, H, gamma=args.gamma, base=base))
    nan = torch.full((N, M, 6), float("nan"), dtype=torch.float64, device=dev)
    s, s_ms = med(lambda: env.plan_place(nan, H, gamma=args.gamma, base=base))
    emit({"row": "a", "what": "plan_place", "envs": N, "M": M, "valid_frac": float(valid.float().mean()),
          "launch_ms_median": a, "launch_ms": a_ms, "seconds_per_variant": a * 1e-3 / (N * M),
          "invalid_candidates_launch_ms_median": s, "invalid_candidates_launch_ms": s_ms,
          "sweeps_and_copy_seconds_per_variant": s * 1e-3 / (N * M),
          "forward_seconds_per_variant": (a - s) * 1e-3 / (N * M)})

    # (b) plan_masked, 8 all-on masks (every emitter cast per variant) and 8 all-off masks
    on = torch.full((N, M), -1, dtype=torch.int64, device=dev)
    b, b_ms = med(lambda: env.plan_masked(on, H, gamma=args.gamma))
    o, o_ms = med(lambda: env.plan_masked(torch.zeros_like(on), H, gamma=args.gamma))
    x = env.export()
    emit({"row": "b", "what": "plan_masked all-on", "envs": N, "M": M,
          "emitters_per_env_mean": float((x["n_cams"] + x["n_guards"]).float().mean()),
          "launch_ms_median": b, "launch_ms": b_ms, "seconds_per_variant": b * 1e-3 / (N * M),
          "all_off_launch_ms_median": o, "all_off_launch_ms": o_ms, "all_off_seconds_per_variant": o * 1e-3 / (N * M),
          "place_over_masked": a / b})

    # (c) the route without the kernel: candidate 0 of every env as a camera of a twin's layout
    layouts, spent = env.layout_lists()
    c0 = cd[:, 0].cpu().tolist()
    plus = [(w, cams + [{"row": int(v[0]), "col": int(v[1]), "fov_angle": v[2], "heading": v[3], "rotation_speed": v[4],
                         "vision_range": int(v[5])}], g) for (w, cams, g), v in zip(layouts, c0)]
    twin = HeistEnv(N, env.config, max_cams=env.max_cams + 1, max_guards=env.max_guards, max_path=env.max_path,
                    device=dev, auto_reset=True)
    lb = LayoutBatch.from_lists(plus, [sp + 3 for sp in spent], twin.max_cams, twin.max_guards, twin.max_path, dev, R, R)
    sr, sc = env.config.start_pos

    def route():
        twin.set_layout_batch(lb)
        twin.reset()
        return twin.plan_field(H), twin.plan_value(H, gamma=args.gamma)

    pf, pv = route()
    v0 = valid[:, 0]
    same = bool(torch.equal(pf.togo[:, sr, sc][v0], ticks_a[:, 0][v0])
                and torch.equal(pv.value[:, sr, sc][v0].contiguous().view(torch.int64),
                                value_a[:, 0][v0].contiguous().view(torch.int64)))
    del pf, pv
    c, c_ms = med(route)
    emit({"row": "c", "what": "set_layout_batch + reset + plan_field + plan_value on a twin handle", "envs": N, "M": 1,
          "twin_equals_plan_place_bitwise_on_valid_candidates": same,
          "pass_ms_median": c, "pass_ms": c_ms, "seconds_per_variant": c * 1e-3 / N, "route_over_place": (c / N) / (a / (N * M))})
    twin.close()

    # (d) a full scan: 64 envs, every interior cell, 8 headings; then every camera's relocation rank
    n = min(64, N)
    side = HeistEnv(n, env.config, max_cams=env.max_cams, max_guards=env.max_guards, max_path=env.max_path, device=dev,
                    auto_reset=True)
    assert bool(side.load_state(env.save_state(list(range(n)))).all())
    full = camera_candidates(side.grid_snapshot(), [45.0 * h for h in range(8)], ref.fov_angle, ref.rotation_speed,
                             ref.vision_range)
    scan = placement_scan(side, full, H, gamma=args.gamma)
    d, d_ms = med(lambda: placement_scan(side, full, H, gamma=args.gamma), runs=min(args.runs, 3))
    Mf = int(full.shape[1])
    solv = scan.ticks0 >= 0
    ranks, n_valid = [], []
    for j in range(side.max_cams):
        rs = relocation_scan(side, j, horizon=H, gamma=args.gamma)
        keep = rs.rank >= 0
        ranks += rs.rank[keep].cpu().tolist()
        n_valid += rs.scan.valid.sum(1)[keep].cpu().tolist()
    emit({"row": "d", "what": "placement_scan, every interior cell x 8 headings", "envs": n, "M": Mf,
          "scan_ms_median": d, "scan_ms": d_ms, "seconds_per_variant": d * 1e-3 / (n * Mf),
          "valid_frac": float(scan.valid.float().mean()), "solvable_baselines": int(solv.sum()), **scan.metrics(),
          "headroom_max": float(scan.headroom().max()), "value0_mean": float(scan.value0.mean()),
          "blocking_frac_max": float(scan.blocking().max()),
          "relocation": {"cameras": len(ranks), "rank0_frac": sum(r == 0 for r in ranks) / max(1, len(ranks)),
                         "rank_median": statistics.median(ranks) if ranks else None,
                         "rank_mean": sum(ranks) / max(1, len(ranks)),
                         "valid_tiles_mean": sum(n_valid) / max(1, len(n_valid))}})
    side.close()
    env.close()
    out_path = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "plan_place.log")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("$ python tools/plan_env.py --place --gamma %r\n" % args.gamma)
        fh.write("\n".join(lines) + "\n")


def place_guard_mode(args, dev):
    """heist_plan_place_guard on the Architect batch, one JSON line per row, each with its N, M and
    device seconds per variant: (a) the launch at M = 8 Architect guards per env (the decode's 8-point
    patrol, speed 1, range 4, fov 90, on a random interior tile each); (b) heist_plan_place in the
    same process with 8 reference cameras per env; (c) the route without the kernel -- candidate 0 of
    every env laid into a twin handle with one more guard slot by set_layout_batch + reset +
    plan_field + plan_value -- with the bitwise-equality flag; (d) a full guard_placement_scan of 64
    envs x every interior tile, with its headroom and blocking share, and next to it the best
    camera's headroom, both per budget point (guard 5, camera 3)."""
    from heist_amd.components.security import Camera
    from heist_amd.search import (CAMERA_COST, GUARD_COST, architect_patrol, camera_candidates, guard_candidates,
                                  guard_placement_scan, placement_scan)
    from heist_amd.vec_env import LayoutBatch
    H = min(args.horizon or args.max_steps, 1024)
    N, R, M = args.envs, args.grid, 8
    ref = Camera(0, 0)
    env = make_env(args, "architect", dev)
    kc = env.kernel_config()
    assert env.plan_place_guard_supported == 1, kc
    head = {"config": "%dx%d" % (R, R), "layouts": "architect", "horizon": H, "gamma": args.gamma,
            "multi_waves": kc["multi_waves"], "guard": [1, 4, 90.0]}
    lines = []

    def emit(row):
        lines.append(json.dumps(dict(head, **row)))
        print(lines[-1], flush=True)

    def med(fn, runs=None):
        ms = timed(dev, fn, args.warmup, runs or args.runs)
        return statistics.median(ms), ms

    # (a) M = 8 Architect guards per env, each decoded from a random interior tile
    gen = torch.Generator().manual_seed(args.seed)
    cell = torch.randint(1, R - 1, (N, M, 2), generator=gen)
    ring = {(r, c): architect_patrol(r, c, R, R) for r in range(1, R - 1) for c in range(1, R - 1)}
    pa = torch.tensor([[ring[(int(r), int(c))] for r, c in row] for row in cell.tolist()], dtype=torch.int32).to(dev)
    me = torch.tensor([8, 1, 4, 0], dtype=torch.int32).reshape(1, 1, 4).expand(N, M, 4).contiguous().to(dev)
    fv = torch.tensor([90.0, 0.0], dtype=torch.float64).reshape(1, 1, 2).expand(N, M, 2).contiguous().to(dev)
    base = env.plan_field(H).vis
    pp = env.plan_place_guard(pa, me, fv, H, gamma=args.gamma, base=base)
    valid, ticks_a, value_a = pp.valid.clone(), pp.ticks.clone(), pp.value.clone()
    del pp
    a, a_ms = med(lambda: env.plan_place_guard(pa, me, fv, H, gamma=args.gamma, base=base))
    none = torch.zeros_like(me)
    s, s_ms = med(lambda: env.plan_place_guard(pa, none, fv, H, gamma=args.gamma, base=base))
    emit({"row": "a", "what": "plan_place_guard", "envs": N, "M": M, "valid_frac": float(valid.float().mean()),
          "launch_ms_median": a, "launch_ms": a_ms, "seconds_per_variant": a * 1e-3 / (N * M),
          "invalid_candidates_launch_ms_median": s, "invalid_candidates_launch_ms": s_ms,
          "sweeps_and_copy_seconds_per_variant": s * 1e-3 / (N * M),
          "forward_seconds_per_variant": (a - s) * 1e-3 / (N * M)})

    # (b) plan_place in the same process: the reference camera on the same tiles, heading 45 m
    cd = torch.cat([cell.double(), torch.full((N, M, 1), ref.fov_angle, dtype=torch.float64),
                    (45.0 * torch.arange(M, dtype=torch.float64)).reshape(1, M, 1).expand(N, M, 1),
                    torch.full((N, M, 1), ref.rotation_speed, dtype=torch.float64),
                    torch.full((N, M, 1), float(ref.vision_range), dtype=torch.float64)], 2).to(dev)
    b, b_ms = med(lambda: env.plan_place(cd, H, gamma=args.gamma, base=base))
    emit({"row": "b", "what": "plan_place, 8 reference cameras per env", "envs": N, "M": M, "launch_ms_median": b,
          "launch_ms": b_ms, "seconds_per_variant": b * 1e-3 / (N * M), "guard_over_camera": a / b})

    # (c) the route without the kernel: candidate 0 of every env as a guard of a twin's layout
    layouts, spent = env.layout_lists()
    plus = [(w, cams, g + [{"patrol_path": ring[(int(rc[0]), int(rc[1]))], "speed": 1, "vision_range": 4,
                            "fov_angle": 90.0}]) for (w, cams, g), rc in zip(layouts, cell[:, 0].tolist())]
    twin = HeistEnv(N, env.config, max_cams=env.max_cams, max_guards=env.max_guards + 1, max_path=env.max_path,
                    device=dev, auto_reset=True)
    lb = LayoutBatch.from_lists(plus, [sp + GUARD_COST for sp in spent], twin.max_cams, twin.max_guards, twin.max_path,
                                dev, R, R)
    sr, sc = env.config.start_pos

    def route():
        twin.set_layout_batch(lb)
        twin.reset()
        return twin.plan_field(H), twin.plan_value(H, gamma=args.gamma)

    pf, pv = route()
    v0 = valid[:, 0]
    same = bool(torch.equal(pf.togo[:, sr, sc][v0], ticks_a[:, 0][v0])
                and torch.equal(pv.value[:, sr, sc][v0].contiguous().view(torch.int64),
                                value_a[:, 0][v0].contiguous().view(torch.int64)))
    del pf, pv
    c, c_ms = med(route)
    emit({"row": "c", "what": "set_layout_batch + reset + plan_field + plan_value on a twin handle", "envs": N, "M": 1,
          "twin_equals_plan_place_guard_bitwise_on_valid_candidates": same,
          "pass_ms_median": c, "pass_ms": c_ms, "seconds_per_variant": c * 1e-3 / N, "route_over_place_guard": (c / N) / (a / (N * M))})
    twin.close()

    # (d) a full scan: 64 envs, the Architect's guard on every interior tile; the best camera next to it
    n = min(64, N)
    side = HeistEnv(n, env.config, max_cams=env.max_cams, max_guards=env.max_guards, max_path=env.max_path, device=dev,
                    auto_reset=True)
    assert bool(side.load_state(env.save_state(list(range(n)))).all())
    grid = side.grid_snapshot()
    full = guard_candidates(grid)
    scan = guard_placement_scan(side, full, H, gamma=args.gamma)
    d, d_ms = med(lambda: guard_placement_scan(side, full, H, gamma=args.gamma), runs=min(args.runs, 3))
    cams = placement_scan(side, camera_candidates(grid, [45.0 * h for h in range(8)], ref.fov_angle, ref.rotation_speed,
                                                  ref.vision_range), H, gamma=args.gamma)
    Mf = int(full[0].shape[1])
    gm, cm = scan.metrics("guard"), cams.metrics("camera")
    emit({"row": "d", "what": "guard_placement_scan, every interior tile", "envs": n, "M": Mf,
          "scan_ms_median": d, "scan_ms": d_ms, "seconds_per_variant": d * 1e-3 / (n * Mf),
          "valid_frac": float(scan.valid.float().mean()), "solvable_baselines": int((scan.ticks0 >= 0).sum()), **gm,
          "headroom_max": float(scan.headroom().max()), "blocking_frac_max": float(scan.blocking().max()),
          "guard_headroom_per_point": gm["guard_headroom_mean"] / GUARD_COST, **cm,
          "camera_headroom_per_point": cm["camera_headroom_mean"] / CAMERA_COST})
    side.close()
    env.close()
    out_path = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "plan_place_guard.log")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("$ python tools/plan_env.py --place-guard --gamma %r\n" % args.gamma)
        fh.write("\n".join(lines) + "\n")


def walls_mode(args, dev):
    """heist_plan_walls on the Architect batch, one JSON line per row, each with its N, M and device
    seconds per variant: (a) the launch at M = 8 with one random valid add per variant; (a') the same
    launch with op 0 everywhere; (b) heist_plan_masked with every slot on, on a handle of the same
    layouts that caches no guard cone -- the same work without edits; (c) the route without the
    kernel -- variant 0 of every env laid into a twin handle by set_layout_batch + reset + plan_field
    + plan_value -- with the bitwise-equality flag; (d) a full wall_placement_scan of 64 envs x every
    interior tile, with the best wall's headroom per budget point; (e) the wall ablation of every
    layout, with the shares of critical, redundant and shielding walls."""
    from heist_amd.search import WALL_COST, wall_candidates, wall_placement_scan
    from heist_amd.vec_env import LayoutBatch
    H = min(args.horizon or args.max_steps, 1024)
    N, R, M = args.envs, args.grid, 8
    env = make_env(args, "architect", dev)
    kc = env.kernel_config()
    assert env.plan_walls_supported == 1, kc
    head = {"config": "%dx%d" % (R, R), "layouts": "architect", "horizon": H, "gamma": args.gamma,
            "multi_waves": kc["multi_waves"], "guard_cones": kc["guard_cones"]}
    lines = []

    def emit(row):
        lines.append(json.dumps(dict(head, **row)))
        print(lines[-1], flush=True)

    def med(fn, runs=None):
        ms = timed(dev, fn, args.warmup, runs or args.runs)
        return statistics.median(ms), ms

    # (a) one random valid add per variant: M = 8 of the env's interior EMPTY tiles (the start holds the Solver)
    gen = torch.Generator().manual_seed(args.seed)
    grid = env.grid_snapshot().cpu()
    free = (grid[:, 1:-1, 1:-1] == 0).reshape(N, -1)
    score = torch.rand(free.shape, generator=gen) + free.double()          # the EMPTY tiles first, in random order
    cell = score.argsort(1, descending=True)[:, :M]
    assert bool(free.gather(1, cell).all()), "an env with fewer than 8 EMPTY tiles"
    ed = torch.stack([cell // (R - 2) + 1, cell % (R - 2) + 1, torch.ones_like(cell)], -1).to(torch.int32)
    ed = ed.reshape(N, M, 1, 3).to(dev)
    pw = env.plan_walls(ed, horizon=H, gamma=args.gamma)
    valid, level, ticks_a, value_a = pw.valid.clone(), pw.level.clone(), pw.ticks.clone(), pw.value.clone()
    del pw
    a, a_ms = med(lambda: env.plan_walls(ed, horizon=H, gamma=args.gamma))
    emit({"row": "a", "what": "plan_walls, one random valid add per variant", "envs": N, "M": M,
          "valid_frac": float(valid.float().mean()), "level_frac": float(level.float().mean()),
          "launch_ms_median": a, "launch_ms": a_ms, "seconds_per_variant": a * 1e-3 / (N * M)})
    none = torch.zeros_like(ed)
    p0 = env.plan_walls(none, horizon=H, gamma=args.gamma)
    ticks_0, value_0, vis_0 = p0.ticks.clone(), p0.value.clone(), p0.vis[:, :, 0].clone()
    del p0
    z, z_ms = med(lambda: env.plan_walls(none, horizon=H, gamma=args.gamma))
    emit({"row": "a'", "what": "plan_walls, op 0 everywhere", "envs": N, "M": M, "launch_ms_median": z, "launch_ms": z_ms,
          "seconds_per_variant": z * 1e-3 / (N * M), "edits_over_none": a / z})

    # (b) plan_masked, every slot on, on a handle of the same layouts without the guard cone cache
    layouts, spent = env.layout_lists()
    plain = HeistEnv(N, env.config, max_cams=env.max_cams, max_guards=env.max_guards, max_path=env.max_path, device=dev,
                     auto_reset=True)
    plain.set_guard_cones(False)
    plain.set_layout_batch(LayoutBatch.from_lists(layouts, spent, plain.max_cams, plain.max_guards, plain.max_path, dev, R, R))
    plain.reset()
    on = torch.full((N, M), -1, dtype=torch.int64, device=dev)
    pm = plain.plan_masked(on, H, gamma=args.gamma)
    same_b = bool(torch.equal(pm.ticks, ticks_0) and torch.equal(pm.value.view(torch.int64), value_0.view(torch.int64))
                  and torch.equal(pm.vis[:, :, 0], vis_0))
    del pm, vis_0
    b, b_ms = med(lambda: plain.plan_masked(on, H, gamma=args.gamma))
    emit({"row": "b", "what": "plan_masked, every slot on, guard cones off", "envs": N, "M": M,
          "guard_cones": plain.kernel_config()["guard_cones"], "equals_plan_walls_without_edits_bitwise": same_b,
          "launch_ms_median": b, "launch_ms": b_ms, "seconds_per_variant": b * 1e-3 / (N * M), "walls_over_masked": a / b})
    plain.close()

    # (c) the route without the kernel: variant 0 of every env as one more wall of a twin's layout
    plus = [(list(w) + [(int(rc[0]), int(rc[1]))], cams, g) for (w, cams, g), rc in zip(layouts, ed[:, 0, 0, :2].tolist())]
    twin = HeistEnv(N, env.config, max_cams=env.max_cams, max_guards=env.max_guards, max_path=env.max_path, device=dev,
                    auto_reset=True)
    lb = LayoutBatch.from_lists(plus, [sp + WALL_COST for sp in spent], twin.max_cams, twin.max_guards, twin.max_path,
                                dev, R, R)
    sr, sc = env.config.start_pos

    def route():
        twin.set_layout_batch(lb)
        twin.reset()
        return twin.plan_field(H), twin.plan_value(H, gamma=args.gamma)

    pf, pv = route()
    v0 = valid[:, 0] & level[:, 0]
    same = bool(torch.equal(pf.togo[:, sr, sc][v0], ticks_a[:, 0][v0])
                and torch.equal(pv.value[:, sr, sc][v0].contiguous().view(torch.int64),
                                value_a[:, 0][v0].contiguous().view(torch.int64)))
    del pf, pv
    c, c_ms = med(route)
    emit({"row": "c", "what": "set_layout_batch + reset + plan_field + plan_value on a twin handle", "envs": N, "M": 1,
          "twin_equals_plan_walls_bitwise_on_valid_level_variants": same, "pass_ms_median": c, "pass_ms": c_ms,
          "seconds_per_variant": c * 1e-3 / N, "route_over_walls": (c / N) / (a / (N * M))})
    twin.close()

    # (d) a full scan: 64 envs, a wall on every interior tile
    n = min(64, N)
    side = HeistEnv(n, env.config, max_cams=env.max_cams, max_guards=env.max_guards, max_path=env.max_path, device=dev,
                    auto_reset=True)
    assert bool(side.load_state(env.save_state(list(range(n)))).all())
    full = wall_candidates(side.grid_snapshot())
    scan = wall_placement_scan(side, full, H, gamma=args.gamma)
    d, d_ms = med(lambda: wall_placement_scan(side, full, H, gamma=args.gamma), runs=min(args.runs, 3))
    Mf = int(full.shape[1])
    wm = scan.metrics()
    emit({"row": "d", "what": "wall_placement_scan, every interior tile", "envs": n, "M": Mf, "scan_ms_median": d,
          "scan_ms": d_ms, "seconds_per_variant": d * 1e-3 / (n * Mf), "valid_frac": float(scan.valid.float().mean()),
          "solvable_baselines": int((scan.ticks0 >= 0).sum()), **wm, "headroom_max": float(scan.headroom().max()),
          "wall_headroom_per_point": wm["wall_headroom_mean"] / WALL_COST})
    side.close()

    # (e) the wall ablation of every layout: one launch, M = 1 + the batch's largest wall count
    ab = env.plan_wall_ablate(horizon=H, gamma=args.gamma)
    Me = int(ab.ticks.shape[1])
    e, e_ms = med(lambda: env.plan_wall_ablate(horizon=H, gamma=args.gamma), runs=min(args.runs, 3))
    emit({"row": "e", "what": "wall ablation (plan_wall_ablate)", "envs": N, "M": Me, "walls": int(ab.filled.sum()),
          "pass_ms_median": e, "pass_ms": e_ms, "seconds_per_variant": e * 1e-3 / (N * Me),
          "unsolvable_layouts": int((ab.ticks[:, 0] < 0).sum()), **ab.metrics(),
          "credit_min": float(ab.credit.min()), "credit_max": float(ab.credit.max())})
    env.close()
    out_path = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "plan_walls.log")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("$ python tools/plan_env.py --walls --gamma %r\n" % args.gamma)
        fh.write("\n".join(lines) + "\n")


DEFAULT_OUT = os.path.join(ROOT, "profiles", "plan_field.log")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--grid", type=int, default=20)
    ap.add_argument("--budget", type=int, default=15)
    ap.add_argument("--max-steps", type=int, default=200)
    ap.add_argument("--horizon", type=int, default=None, help="default: max_steps (at most 1024)")
    ap.add_argument("--layouts", choices=("architect", "synthetic", "empty"), default="architect")
    ap.add_argument("--ckpt", default=None, help="Architect checkpoint (default: the fixed C2 one)")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--field", action="store_true", help="time heist_plan_field next to heist_plan on all three batches")
    ap.add_argument("--all-ticks", action="store_true", help="with --field / --value: also the launch that writes "
                    "togo_ticks / value_ticks and action_ticks")
    ap.add_argument("--value", action="store_true", help="time heist_plan_value next to heist_plan_field on all three "
                    "batches, with the start cell's values and the length of the return-optimal episodes")
    ap.add_argument("--gamma", type=float, default=1.0, help="with --value / --ablate / --place: the discount")
    ap.add_argument("--play", action="store_true", help="time heist_plan_play next to the Python path it replaces and "
                    "to heist_plan_value on the --layouts batch")
    ap.add_argument("--noise", type=float, default=0.1, help="with --play / --q: the noisy play's probability")
    ap.add_argument("--q", action="store_true", help="time heist_plan_q next to search.q_values on the same device "
                    "tensors and to the plan_value(all_ticks=True) launch that feeds it, on all three batches")
    ap.add_argument("--ablate", action="store_true", help="time heist_plan_masked's leave-one-out launch next to "
                    "M x (heist_plan_field + heist_plan_value) on all three batches, with the critical / redundant emitters")
    ap.add_argument("--place", action="store_true", help="time heist_plan_place next to heist_plan_masked and to the "
                    "twin-handle route on the Architect batch, then a full placement_scan of 64 envs")
    ap.add_argument("--place-guard", action="store_true", help="time heist_plan_place_guard next to heist_plan_place "
                    "and to the twin-handle route on the Architect batch, then a full guard_placement_scan of 64 envs "
                    "(log: profiles/plan_place_guard.log)")
    ap.add_argument("--walls", action="store_true", help="time heist_plan_walls next to heist_plan_masked without the "
                    "guard cone cache and to the twin-handle route on the Architect batch, then a full wall_placement_scan "
                    "of 64 envs and the wall ablation of the batch (log: profiles/plan_walls.log)")
    ap.add_argument("--out", default=DEFAULT_OUT, help="--field's log (--value's: profiles/plan_value.log, --play's: "
                    "profiles/plan_play.log, --q's: profiles/plan_q.log, --ablate's: profiles/plan_masked.log, --place's: "
                    "profiles/plan_place.log)")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if args.walls:
        return walls_mode(args, dev)
    if args.place_guard:
        return place_guard_mode(args, dev)
    if args.place:
        return place_mode(args, dev)
    if args.ablate:
        return ablate_table(args, dev)
    if args.q:
        return q_mode(args, dev)
    if args.play:
        return play_table_mode(args, dev)
    if args.value:
        return value_table(args, dev)
    if args.field:
        return field_table(args, dev)
    R, N, budget = args.grid, args.envs, args.budget
    cfg = EnvironmentConfig(grid_rows=R, grid_cols=R, max_steps=args.max_steps, architect_budget=budget)
    env = HeistEnv(N, cfg, max_cams=max(1, budget // 3), max_guards=max(1, budget // 5), max_path=16, device=dev,
                   auto_reset=True)
    if args.layouts == "architect":
        bench.architect_layouts(env, budget, seed=args.seed, ckpt=args.ckpt)
    elif args.layouts == "synthetic":
        valid_synthetic_layouts(env, budget, seed=args.seed)
    else:
        env.set_layouts([([], [], [])] * N, budget=budget)
    valid = env.valid.clone().bool()
    env.reset()
    H = min(args.horizon or args.max_steps, 1024)
    kc = env.kernel_config()
    assert env.plan_supported == 1, kc

    res = env.plan(H)
    ticks = res.ticks.cpu()
    ok = ticks > 0
    rows_live = (res.reach != 0).any(2).sum(0).cpu()  # reach rows that hold a cell
    planned = torch.where(ok, ticks.long(), torch.clamp(rows_live + 1, max=H))  # ticks each env's block ran
    hist = {}
    for t in ticks[ok].tolist():
        lo = t // 10 * 10
        hist["%d-%d" % (lo, lo + 9)] = hist.get("%d-%d" % (lo, lo + 9), 0) + 1
    plan_ms = timed(dev, lambda: env.plan(H), args.warmup, args.runs)

    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)
    actions = torch.randint(0, 5, (H, N), device=dev, generator=gen, dtype=torch.int64)
    rec_ms = timed(dev, lambda: env.step_multi_records(actions), args.warmup, args.runs)

    p, r = statistics.median(plan_ms), statistics.median(rec_ms)
    out = {"config": "%dx%d" % (R, R), "envs": N, "layouts": args.layouts, "horizon": H, "budget": budget,
           "multi_waves": kc["multi_waves"], "records_kernel": bench.multi_kernel_name(kc, R, R),
           "records_direct": env.records_direct,
           "solvable_frac": float(ok.float().mean()), "bfs_valid": int(valid.sum()),
           "bfs_valid_but_unsolvable": int((valid.cpu() & ~ok).sum()),
           "optimal_ticks": {"min": int(ticks[ok].min()) if ok.any() else None,
                             "mean": float(ticks[ok].float().mean()) if ok.any() else None,
                             "max": int(ticks[ok].max()) if ok.any() else None, "histogram": hist},
           "planned_ticks_mean": float(planned.float().mean()),
           "plan": {"launch_ms_median": p, "launch_ms": plan_ms, "us_per_tick_of_horizon": p / H * 1e3,
                    "us_per_planned_tick": p / float(planned.float().mean()) * 1e3,
                    "ns_per_env_tick_planned": p * 1e6 / float(planned.sum())},
           "records": {"launch_ms_median": r, "launch_ms": rec_ms, "us_per_tick": r / H * 1e3,
                       "ns_per_env_tick": r * 1e6 / (H * N)}}
    out["plan_over_records_per_tick_run"] = out["plan"]["us_per_planned_tick"] / out["records"]["us_per_tick"]
    env.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
