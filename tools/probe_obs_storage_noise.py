"""Run-to-run noise of one train_iteration under obs_storage="full" against itself and against
"compact" (identical seeds; the setup of tests/test_gpu_obs_compact.py::_train_once): the
largest absolute difference of any loss part or Solver parameter against the first full run and
over all pairs, per cadence.  The constant FULL_RUN_TO_RUN_NOISE of that test records its
full-against-full figure.  One line: FULL_NOISE {json}."""
import json
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "rl-project-heist-architect-adversarial-reinforcement-learning-framework-cse4019_amd"),
                os.path.join(ROOT, "tests")]
import torch  # noqa: E402

import test_gpu_obs_compact as T  # noqa: E402


def diff(x, y):
    worst = 0.0
    for k in ("solver_policy_loss", "solver_value_loss", "solver_entropy"):
        worst = max(worst, abs(x[1][k] - y[1][k]))
    for a, b in zip(x[2], y[2]):
        worst = max(worst, float((a - b).abs().max()))
    return worst


def main():
    dev = torch.device("cuda:0")
    res = {}
    for cadence in ("rollout", "layout_batch"):
        tmp = pathlib.Path(tempfile.mkdtemp())
        full = [T._train_once(tmp, dev, cadence, "full", "r%d" % i) for i in range(8)]
        comp = [T._train_once(tmp, dev, cadence, "compact", "c%d" % i) for i in range(6)]
        res[cadence] = {"full_vs_full0": [diff(f, full[0]) for f in full[1:]],
                        "full_pairs_max": max(diff(a, b) for a in full for b in full),
                        "compact_vs_full0": [diff(c, full[0]) for c in comp],
                        "compact_pairs_max": max(diff(a, b) for a in comp for b in comp)}
    print("FULL_NOISE", json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
