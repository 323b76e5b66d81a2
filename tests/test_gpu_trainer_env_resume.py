"""GPU test of AdversarialTrainer(checkpoint_env=True): a checkpoint that also holds the batch
(env states, per-env bookkeeping, LSTM state, observation), and a resume that continues it.

The resumed env is checked by action replay -- the saved run's third-iteration actions stepped
on the resumed trainer's env give that run's reward64 / done / status tick for tick -- so the
test depends neither on RNG streams nor on the update's run-to-run float noise.
"""
import glob
import os

import numpy as np
import pytest
import torch

from heist_amd import EnvironmentConfig
from heist_amd.training import AdversarialTrainer

pytestmark = pytest.mark.gpu

N, T, A = 16, 40, 2
TENSORS = ("b_valid", "b_attempts", "b_scored", "b_solve", "b_detect", "b_timeout", "b_steps", "b_reward", "b_logp",
           "b_value", "h", "c")


def _trainer(tmp_path, device, **kw):
    cfg = EnvironmentConfig(grid_rows=12, grid_cols=12, max_steps=60)
    return AdversarialTrainer(cfg, solver_episodes_per_layout=A, total_episodes=10 ** 6, save_dir=str(tmp_path / "ck"),
                              log_dir=str(tmp_path / "logs"), n_envs=N, rollout_len=T, device=device, seed=0,
                              minibatch=512, **kw)


def _started(tmp_path, device, **kw):
    tr = _trainer(tmp_path, device, **kw)
    tr.global_episode = 200  # curriculum phase with cameras and guards
    tr._assign_layouts(np.arange(N))
    return tr


def test_resume_continues_the_batch(gpu_device, tmp_path):
    tr = _started(tmp_path, gpu_device, checkpoint_env=True)
    tr.train_iteration()
    tr.train_iteration()
    ep = tr.global_episode
    tr._save_checkpoint(ep)
    assert os.path.exists(os.path.join(tr.save_dir, "env_ep%d.pt" % ep))
    saved = {k: getattr(tr, k).clone() for k in TENSORS}
    saved_obs, saved_meta, saved_eps = tr.env.obs.clone(), list(tr.b_meta), tr.b_episode.copy()
    saved_export = tr.env.export(grid=True)
    counters = (tr.solver._act_counter, tr.solver._act_seed)
    saved_layouts = tr.layout_lists(range(N))
    assert bool(saved["b_valid"].any())
    assert int((saved_export["n_walls"] + saved_export["n_cams"] + saved_export["n_guards"]).sum()) > 0
    tr._trace = []
    tr.train_iteration()  # run A's third iteration
    trace = tr._trace
    assert len(trace) == T

    tr2 = _trainer(tmp_path, gpu_device, checkpoint_env=True)
    assert tr2.resume_from_checkpoint() == ep
    assert tr2._env_restored and tr2.global_episode == ep
    for k in TENSORS:
        assert torch.equal(getattr(tr2, k), saved[k]), k
    assert torch.equal(tr2.env.obs, saved_obs)
    assert tr2.b_meta == saved_meta and np.array_equal(tr2.b_episode, saved_eps)
    assert (tr2.solver._act_counter, tr2.solver._act_seed) == counters
    assert tr2.layout_lists(range(N)) == saved_layouts
    ex = tr2.env.export(grid=True)
    for k in ex:
        assert torch.equal(ex[k], saved_export[k]), k
    for t, (a, r64, done, status) in enumerate(trace):
        _, _, d, s = tr2.env.step(a)
        assert torch.equal(tr2.env.reward64, r64), "tick %d reward64" % t
        assert torch.equal(d, done) and torch.equal(s, status), "tick %d" % t
    tr.env.close()
    tr2.env.close()


def test_option_off_writes_no_env_file_and_resumes_fresh(gpu_device, tmp_path):
    tr = _started(tmp_path, gpu_device)
    assert tr.checkpoint_env is False
    tr.train_iteration()
    ep = tr.global_episode
    tr._save_checkpoint(ep)
    assert glob.glob(os.path.join(tr.save_dir, "env_ep*")) == []
    tr2 = _trainer(tmp_path, gpu_device)
    assert tr2.resume_from_checkpoint() == ep and not tr2._env_restored
    assert not bool(tr2.b_valid.any())
    ex = tr2.env.export()
    assert int(ex["tick"].abs().sum()) == 0 and int((ex["n_walls"] + ex["n_cams"] + ex["n_guards"]).sum()) == 0
    # an env file in the directory is not read with the option off either
    tr3 = _started(tmp_path, gpu_device, checkpoint_env=True)
    tr3.global_episode = ep
    tr3._save_env_checkpoint(ep)
    assert os.path.exists(os.path.join(tr.save_dir, "env_ep%d.pt" % ep))
    tr4 = _trainer(tmp_path, gpu_device)
    assert tr4.resume_from_checkpoint() == ep and not tr4._env_restored
    assert int(tr4.env.export()["tick"].abs().sum()) == 0
    for t in (tr, tr2, tr3, tr4):
        t.env.close()
