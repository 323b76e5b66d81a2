"""Child process of tests/test_gpu_env_state.py (test infrastructure): load saved env states
into a HeistEnv created in THIS process -- under whatever HEIST_* variables the parent put into
its environment -- play the given actions and write every tick's outputs.

usage: python env_state_child.py <job.pt> <out.pt>
job.pt: {"cfg": EnvironmentConfig fields, "n", "max_cams", "max_guards", "max_path", "state":
EnvState state_dict, "actions" [T, n] int64, "auto_reset"}."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "rl-project-heist-architect-adversarial-reinforcement-learning-framework-cse4019_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(job_path, out_path):
    from heist_amd import EnvironmentConfig, EnvState, HeistEnv
    job = torch.load(job_path, weights_only=False)
    cfg = EnvironmentConfig(**job["cfg"])
    dev = torch.device("cuda:0")
    env = HeistEnv(job["n"], cfg, max_cams=job["max_cams"], max_guards=job["max_guards"], max_path=job["max_path"],
                   device=dev)
    status = env.load_state(EnvState.from_state_dict(job["state"]))
    rows = []
    for a in job["actions"].to(dev):
        obs, _, done, st = env.step(a, auto_reset=job["auto_reset"])
        rows.append((obs.view(torch.int32).cpu().clone(), env.reward64.cpu().clone(), done.cpu().clone(),
                     st.cpu().clone()))
    out = {"loaded": status.cpu(), "step_waves": env.kernel_config()["step_waves"],
           "obs": torch.stack([r[0] for r in rows]), "reward64": torch.stack([r[1] for r in rows]),
           "done": torch.stack([r[2] for r in rows]), "status": torch.stack([r[3] for r in rows]),
           "export": {k: v.cpu() for k, v in env.export(grid=True).items()}}
    torch.cuda.synchronize()
    torch.save(out, out_path)
    env.close()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
