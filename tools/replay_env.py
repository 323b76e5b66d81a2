"""Lift one env out of a saved batch and replay it on its own.

Loads an EnvState file (EnvState.save, or the "env_state" entry of a trainer's env_ep{N}.pt),
picks one of its envs, loads it into a 1-env HeistEnv of the saved configuration and steps it
under the given actions, printing one line per tick: tick, action, reward (float64), done, status.

  python tools/replay_env.py state.pt --env 137 --actions 4,4,2,0,1
  python tools/replay_env.py checkpoints/env_ep250.pt --env 5 --actions-file acts.txt --auto-reset
  python tools/replay_env.py state.pt --env 137 --actions-file long.txt --records

--records replays through HeistEnv.step_multi_records (launches of up to 1024 ticks whose rows are
64-byte records, not observations) and prints the same lines: the position is the record's
position word, and nothing is expanded that is not printed.

The reward constants are not part of a saved state: pass --rewards step,detection,vault when the
run used others than EnvironmentConfig's defaults.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-project-heist-architect-adversarial-reinforcement-learning-framework-cse4019_amd")]
import torch  # noqa: E402

from heist_amd import EnvironmentConfig, EnvState, HeistEnv, STATUS_NAMES  # noqa: E402


def load_states(path):
    sd = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(sd, dict) and sd.get("format") == "heist_env_checkpoint":
        sd = sd["env_state"]
    return EnvState.from_state_dict(sd)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("state")
    ap.add_argument("--env", type=int, default=0, help="which saved env (row of the file's blobs)")
    ap.add_argument("--actions", default="", help="comma-separated actions 0..4 (wait, up, down, left, right)")
    ap.add_argument("--actions-file", help="whitespace- or comma-separated actions")
    ap.add_argument("--auto-reset", action="store_true", help="reset the env when it finishes, as training does")
    ap.add_argument("--rewards", help="reward_step,reward_detection,reward_vault")
    ap.add_argument("--records", action="store_true",
                    help="replay in K-tick launches that emit compact records (same output)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    st = load_states(args.state)
    if not 0 <= args.env < len(st):
        ap.error("--env %d: the file holds %d envs" % (args.env, len(st)))
    text = args.actions
    if args.actions_file:
        with open(args.actions_file) as f:
            text = f.read()
    acts = [int(x) for x in text.replace(",", " ").split()]
    c = st.config
    kw = {}
    if args.rewards:
        kw = dict(zip(("reward_step", "reward_detection", "reward_vault"), (float(x) for x in args.rewards.split(","))))
    cfg = EnvironmentConfig(grid_rows=c["rows"], grid_cols=c["cols"], max_steps=c["max_steps"],
                            start_pos=(c["start_r"], c["start_c"]), vault_pos=(c["vault_r"], c["vault_c"]), **kw)
    env = HeistEnv(1, cfg, max_cams=c["max_cams"], max_guards=c["max_guards"], max_path=c["max_path"],
                   device=args.device, auto_reset=args.auto_reset)
    env.set_guard_cones(bool(c["guard_cones"]))
    if not bool(env.load_state(st[args.env])[0]):
        sys.exit("the device rejected the saved state")
    ex = env.export()
    print("env %d of %s: pos (%d, %d) tick %d done %d, %d cameras, %d guards, %d walls" % (
        args.env, args.state, int(ex["pos_r"][0]), int(ex["pos_c"][0]), int(ex["tick"][0]), int(ex["done"][0]),
        int(ex["n_cams"][0]), int(ex["n_guards"][0]), int(ex["n_walls"][0])))
    if args.records:
        from heist_amd.obs_compact import record_words
        nvis = (c["rows"] * c["cols"] + 31) // 32
        assert nvis < record_words(c["rows"], c["cols"])
        for k0 in range(0, len(acts), 1024):
            chunk = acts[k0:k0 + 1024]
            rec, _, done, status, r64 = env.step_multi_records(torch.tensor(chunk).reshape(-1, 1), reward64=True)
            pos = rec[:, 0, nvis].cpu().tolist()  # pos_r | pos_c << 8
            r64, done, status = r64[:, 0].cpu().tolist(), done[:, 0].cpu().tolist(), status[:, 0].cpu().tolist()
            for j, a in enumerate(chunk):
                print("%4d  action %d  reward %r  done %d  status %s  pos (%d, %d)" % (
                    k0 + j, a, float(r64[j]), int(done[j]), STATUS_NAMES[int(status[j])], pos[j] & 0xff,
                    (pos[j] >> 8) & 0xff))
        env.close()
        return
    for k, a in enumerate(acts):
        env.step(torch.tensor([a]))
        ex = env.export()
        print("%4d  action %d  reward %r  done %d  status %s  pos (%d, %d)" % (
            k, a, float(env.reward64[0]), int(env.done[0]), STATUS_NAMES[int(env.status[0])], int(ex["pos_r"][0]),
            int(ex["pos_c"][0])))
    env.close()


if __name__ == "__main__":
    main()
