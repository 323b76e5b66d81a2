"""The Solver's whole fp32 PPO update on the GPU against the reference's own update
(agents/solver.py:112-217) on real buffers: tests/golden/solver_update_<case>.npz holds, per case,
reference episodes on Architect layouts, the shuffles, and what the reference's update() computed
from the nets.npz weights -- normalised advantages, returns, per-step loss parts, pre-clip
gradients and total norms at the first step, the first short (tail) minibatch and the last step,
the metrics and the parameter change.  Chained here as SolverAgent.update() chains them: heist_gae,
heist_adv_normalize, the shuffled gather (heist_train_obs_nhwc4 reads the gathered rows'
strides), the fp32-MFMA convolutions or MIOpen with the fused tail, heist_ppo_loss,
clip_grad_norm_ and Adam.

cases  g20    20 x 20, 129 transitions, 3 x 64: minibatches 64, 64, 1 (MFMA, one-band last unit)
       g32    32 x 32, 86 transitions: 64, 22 (MFMA two-row bands)
       g10    10 x 10, 70 transitions: 64, 6 (fused tail around MIOpen)
       clip20 as g20 with the two head output layers scaled and stale old log-probs on a third
              of the rows: 45 % of the first minibatch's ratios clipped, entropy 1.54
       big20  20 x 20, one minibatch of 4,099 rows (several MFMA units per workgroup, the split-K
              weight gradients of the linear layers, which engage at 4,096 rows)

Bounds: 1e-4 (the project's stated parity) at the first step; at later steps and for the
parameter change max(1e-4, 10 x the reference's own float32-vs-float64 error for that tensor,
recorded in the fixture).  Conv tensors are compared in full (gradients relative to their max, the
parameter change in relative L2), the others by L2 norm and 4 fixed projections
(tests/test_architect_update.py's form: gradients within 4 x bound x norm, the parameter change
within bound x norm); clip20's two scaled head layers, whose Adam steps float32 cannot resolve,
element by element within 2 float32 spacings (_check_delta).  tests/solver_update_ref.py (tied to the fixture by
tests/test_solver_update_ref_cpu.py) serves one purpose here: when a conv gradient misses 1e-4,
it is recomputed in float64 under the GPU forward's own ReLU masks, held to 1e-4 against that,
and the mask differences from float64's own are counted (at most 1e-5 of the pre-activations).
"""
import json

import numpy as np
import pytest
import torch

import solver_update_ref as sr
from mfma_forward import mfma_forward
from heist_amd.agents import SolverAgent
from heist_amd.ppo import compute_gae, normalize_advantages, ppo_loss

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = sr.load_case(name)
    return _CASES[name]


def _agent(c, dev, epochs=None, batch=None):
    ag = SolverAgent(c["R"], c["C"], ppo_epochs=epochs or c["epochs"], batch_size=batch or c["batch"], device=dev)
    ag.network.load_state_dict(sr.golden_params(c["head_scale"]))
    return ag


def _dev_buffers(c, dev):
    t = lambda a, dt: torch.as_tensor(np.asarray(a)).to(dt).to(dev)  # noqa: E731
    return (t(c["states"], torch.float32), t(c["actions"], torch.int64), t(c["logp"], torch.float32),
            t(c["values"], torch.float32), t(c["rewards"], torch.float32), t(c["dones"], torch.float32))


def _advantages(c, ag, values, rewards, dones):
    """compute_gae + normalize_advantages as update() chains them, held to the fixture."""
    adv, ret = compute_gae(rewards, values, dones, gamma=ag.gamma, lam=ag.gae_lambda)
    adv = normalize_advantages(adv, group="local")
    e_a = float(np.abs(adv.cpu().numpy() - c["adv"]).max())
    e_r = float(np.abs(ret.cpu().numpy() - c["ret"]).max())
    assert e_a <= 1e-4 and e_r <= 1e-4, (e_a, e_r)
    return adv, ret, e_a, e_r


def _grads64(params):
    params = list(params)
    # every parameter is in the loss graph (lstm.weight_hh_l0 through the zero hidden state): a
    # missing gradient is not the exact zero the checks ask for
    assert all(p.grad is not None for p in params)
    return [p.grad.detach().double().cpu().numpy() for p in params]


def _total_norm(grads):
    return float(np.sqrt(sum(float((g ** 2).sum()) for g in grads)))


def _bounds(c, j):
    """Per tensor max(1e-4, 10 x the reference's own error) at recorded step j (conv tensors: relative
    to the max; the others: relative L2)."""
    floor = np.where(np.arange(len(sr.PARAMS)) < sr.N_CONV, c["floor_grad_max"][j], c["floor_grad_l2"][j])
    return np.maximum(1e-4, 10 * floor)


def _forced_mask_fallback(c, net, x, rows, got, bad, what):
    """The allowed way out for conv tensors that missed their bound: float64 under the GPU forward's
    own ReLU masks, 1e-4; mask differences from float64's own at most 1e-5 of the pre-activations."""
    assert all(n.startswith("conv") for n, _, _ in bad), "%s: %s" % (what, bad)
    assert net._train_conv_ok(x), "%s: %s" % (what, bad)
    masks = [(a > 0).cpu() for a in mfma_forward(net, x)]
    perm = np.concatenate([rows, np.setdiff1d(np.arange(c["T"]), rows)])[None]
    r = sr.run_update(sr.golden_params(c["head_scale"]), c["states"], c["actions"], c["logp"], c["values"],
                      c["rewards"], c["dones"].astype(np.float32), perm, 1, len(rows), record=[0], masks={0: masks},
                      keep_signs=True, stop_after=1)
    flips = sum(int((m != o).sum()) for m, o in zip(masks, r["signs"][0]))
    total = sum(m.numel() for m in masks)
    errs = {n: sr.rel_max(got[sr.PARAMS.index(n)], r["steps"][0]["grads"][n].numpy()) for n, _, _ in bad}
    print("%s: forced-mask fallback for %s; ReLU decisions differing from float64: %d of %d; errors %s"
          % (what, [n for n, _, _ in bad], flips, total, errs))
    assert flips <= 1e-5 * total, (what, flips, total)
    assert max(errs.values()) <= 1e-4, (what, errs)
    return flips


def _first_step(c, dev, mfma, force_masks=False):
    ag = _agent(c, dev)
    states, actions, old_logp, values, rewards, dones = _dev_buffers(c, dev)
    adv, ret, e_a, e_r = _advantages(c, ag, values, rewards, dones)
    rows = c["perms"][0][:c["batch"]].astype(np.int64)
    b = torch.as_tensor(rows).to(dev)
    x = states[b]
    assert ag.network._train_conv_ok(x) == mfma
    if not mfma:  # as _ppo_epochs: MIOpen's convolutions want channels-last
        x = x.contiguous(memory_format=torch.channels_last)
    ag.network.train()
    ag.optimizer.zero_grad(set_to_none=True)
    logits, new_values, _ = ag.network(x)
    loss, parts = ppo_loss(logits, new_values.reshape(-1), actions[b], old_logp[b], adv[b], ret[b], ag.clip_epsilon,
                           ag.value_coeff, ag.entropy_coeff)
    loss.backward()
    parts = parts.detach().cpu().numpy().astype(np.float64)
    e_parts = float(np.abs(parts[1:] - c["s0_parts"]).max())
    got = _grads64(ag.network.parameters())
    e_total = abs(_total_norm(got) - float(c["s0_total"])) / float(c["s0_total"])
    seen, bad = sr.check_tensors(got, c["s0_gconv"], c["s0_gnorm"], c["s0_gproj"], 1e-4, c["name"] + " step 0")
    print("MEASURED " + json.dumps(dict(case=c["name"], route="mfma" if mfma else "miopen+tail", adv=e_a, ret=e_r,
                                        parts=e_parts, total_norm=e_total, grad_worst=max(seen.values()),
                                        grad=seen)))
    assert e_parts <= 1e-4, parts
    want_loss = c["s0_parts"][0] + ag.value_coeff * c["s0_parts"][1] - ag.entropy_coeff * c["s0_parts"][2]
    assert abs(parts[0] - want_loss) <= 1e-4 * max(1.0, abs(want_loss))
    assert e_total <= 1e-4, e_total
    if force_masks:  # every conv tensor through the fallback's comparison, whether it missed or not
        bad = [(n, seen[n], 1e-4) for n in sr.PARAMS[:sr.N_CONV]]
    if bad:
        _forced_mask_fallback(c, ag.network, x, rows, got, bad, c["name"] + " step 0")


@pytest.mark.parametrize("name", sr.CASES)
def test_update_first_step(gpu_device, name):
    """Step 0 by hand from the fixture's buffers: GAE and normalised advantages within 1e-4, then
    minibatch 0 by the stored shuffle through the training forward, ppo_loss and backward: loss
    parts within 1e-4, pre-clip total norm within 1e-4 relative, every conv gradient within 1e-4 of
    its max, every other gradient's norm within 1e-4 and projections within 4e-4 x norm,
    lstm.weight_hh_l0's gradient exactly zero (zero hidden state).  The MFMA kernels ran at
    20 x 20 and 32 x 32, MIOpen + fused tail at 10 x 10."""
    c = _case(name)
    _first_step(c, gpu_device, mfma=c["R"] in (20, 32))


@pytest.mark.parametrize("name", ["g20", "g32"])
def test_update_first_step_under_gpu_masks(gpu_device, name):
    """The forced-mask comparison itself, which test_update_first_step reaches only when a conv
    gradient misses 1e-4: step 0's six conv gradients against the float64 restatement run under the
    MFMA forward's own ReLU masks, within 1e-4 of each tensor's max, and those masks against
    float64's own (at most 1e-5 of the pre-activations differ)."""
    c = _case(name)
    _first_step(c, gpu_device, mfma=True, force_masks=True)


def test_update_first_step_miopen_route_20(gpu_device, monkeypatch):
    """g20's first step with HEIST_TRAIN_CONV=0: the MIOpen + fused-tail route at the headline
    size, held to the same fixture."""
    monkeypatch.setenv("HEIST_TRAIN_CONV", "0")
    _first_step(_case("g20"), gpu_device, mfma=False)


class _ClipRecorder:
    """Stands in for torch.nn.utils.clip_grad_norm_: counts the optimizer steps and keeps the
    pre-clip gradients of the wanted ones."""

    def __init__(self, monkeypatch, steps):
        self.real, self.steps, self.count, self.grads = torch.nn.utils.clip_grad_norm_, set(steps), 0, {}
        monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", self)

    def __call__(self, parameters, max_norm, *a, **kw):
        parameters = list(parameters)
        if self.count in self.steps:
            self.grads[self.count] = _grads64(parameters)
        self.count += 1
        return self.real(parameters, max_norm, *a, **kw)


def _check_recorded(c, rec, what):
    """The recorded steps' gradients against the fixture: ([(step, total-norm error, its bound, tensors
    over their bound)], the measured figures)."""
    rows, out = [], {}
    for j, s in enumerate(c["rec_steps"]):
        key = "s%d_" % s
        got = rec.grads[s]
        e_total = abs(_total_norm(got) - float(c[key + "total"])) / float(c[key + "total"])
        seen, bad = sr.check_tensors(got, c[key + "gconv"], c[key + "gnorm"], c[key + "gproj"], _bounds(c, j),
                                     "%s step %d" % (what, s))
        out["step%d" % s] = dict(total_norm=e_total, grad_worst=max(seen.values()), grad=seen)
        rows.append((s, e_total, max(1e-4, 10 * float(c["floor_total"][j])), bad))
    return rows, out


def _check_delta(c, net, p0):
    """The parameter change against the fixture: conv tensors in relative L2, the others by norm and
    projections within bound x norm, bound = max(1e-4, 10 x the reference's own error); a case's
    scaled head layers element by element (solver_update_ref.coarse_delta) within 2 float32
    spacings of the weight + 1e-4 of the largest change.  Why 2: both sides run torch's float32
    Adam, so an element rounds differently only where its exact new value lies within the two
    steps' disagreement (at most 1e-4 of a 3e-4 step, the gradient bound) of a rounding boundary,
    a chance of at most 1e-4 x 3e-4 / spacing ~ 1e-3 per element and step: over 768 elements x 9
    steps a handful of one-spacing differences, two on one element practically never."""
    delta = [(p.detach().double() - q.double()).cpu().numpy() for p, q in zip(net.parameters(), p0)]
    bound = np.maximum(1e-4, 10 * c["floor_delta"])
    full = sr.coarse_delta(c, dict(zip(sr.PARAMS, p0)), 2.0)
    for i in full or ():
        bound[i] = 1.0
    seen, bad = sr.check_tensors(delta, c["d_conv"], c["d_norm"], c["d_proj"], bound, c["name"] + " parameter change",
                                 conv_metric=sr.rel_l2, proj_factor=1.0, full=full)
    assert torch.equal(list(net.parameters())[sr.HH], p0[sr.HH]), "lstm.weight_hh_l0 changed"
    return seen, bad, bound


@pytest.mark.parametrize("name,n_steps", [("g20", 9), ("g32", 6), ("g10", 6), ("clip20", 9)])
def test_update_whole(gpu_device, monkeypatch, name, n_steps):
    """SolverAgent.update() on the fixture's buffers with the stored shuffles replayed: the
    number of optimizer steps, the three metrics within 1e-4, the pre-clip gradients at the
    first step, the first tail minibatch (1, 22 or 6 rows) and the last step, and the parameter
    change of every tensor, each within max(1e-4, 10 x the reference's own float32 error there);
    lstm.weight_hh_l0 bit-unchanged; the buffers cleared.

    Measured on an MI355X: see DESIGN.md ("The whole update against the reference")."""
    c = _case(name)
    ag = _agent(c, gpu_device)
    ag.states = list(c["states"])
    ag.actions = [int(a) for a in c["actions"]]
    ag.log_probs = [float(v) for v in c["logp"]]
    ag.values = [float(v) for v in c["values"]]
    ag.rewards = [float(v) for v in c["rewards"]]
    ag.dones = [bool(v) for v in c["dones"]]
    served = []

    def replay(n):
        assert n == c["T"]
        served.append(n)
        return c["perms"][len(served) - 1].astype(np.int64)

    monkeypatch.setattr(np.random, "permutation", replay)
    rec = _ClipRecorder(monkeypatch, c["rec_steps"])
    p0 = [p.detach().clone() for p in ag.network.parameters()]
    m = ag.update()
    assert rec.count == n_steps == c["n_steps"] and len(served) == c["epochs"]
    assert m["solver_updates"] == n_steps
    got_m = np.array([m["solver_policy_loss"], m["solver_value_loss"], m["solver_entropy"]])
    e_m = float(np.abs(got_m - c["metrics"]).max())
    failures = []
    checked, measured = _check_recorded(c, rec, name)
    for s, e_total, b_total, bad in checked:
        if e_total > b_total:
            failures.append(("step %d total norm" % s, e_total, b_total))
        failures += [("step %d %s" % (s, n), e, b) for n, e, b in bad]
    seen, bad, bound = _check_delta(c, ag.network, p0)
    failures += [("parameter change %s" % n, e, b) for n, e, b in bad]
    print("MEASURED " + json.dumps(dict(case=name, whole=True, metrics=e_m, delta_worst=max(seen.values()),
                                        delta=seen, delta_bound=dict(zip(sr.PARAMS, bound.tolist())), **measured)))
    assert e_m <= 1e-4, (got_m, c["metrics"])
    assert not failures, failures
    for buf in (ag.states, ag.actions, ag.log_probs, ag.values, ag.rewards, ag.dones):
        assert len(buf) == 0


def test_update_big_minibatch(gpu_device, monkeypatch):
    """big20 through _ppo_epochs(minibatch=4099, collective=False): one optimizer step over 4,099
    rows.  The linear layers' weight gradients went through _LinearSplitK (counted); gradients and
    the parameter change as in test_update_whole."""
    import heist_amd.networks as nets
    c = _case("big20")
    ag = _agent(c, gpu_device, epochs=1)
    states, actions, old_logp, values, rewards, dones = _dev_buffers(c, gpu_device)
    adv, ret, _, _ = _advantages(c, ag, values, rewards, dones)
    calls = []
    real = nets._wgrad_splitk

    def counted(g, x, *a, **kw):
        calls.append(tuple(g.shape))
        return real(g, x, *a, **kw)

    monkeypatch.setattr(nets, "_wgrad_splitk", counted)
    rec = _ClipRecorder(monkeypatch, [0])
    p0 = [p.detach().clone() for p in ag.network.parameters()]
    m = ag._ppo_epochs(states, actions, old_logp, adv, ret, c["T"], lambda n: c["perms"][0].astype(np.int64),
                       minibatch=c["T"], collective=False)
    assert rec.count == 1 and m["solver_updates"] == 1
    # fc_spatial, the LSTM's two, and two per head
    assert len(calls) == 7 and all(s[0] == c["T"] for s in calls), calls
    got_m = np.array([m["solver_policy_loss"], m["solver_value_loss"], m["solver_entropy"]])
    e_m = float(np.abs(got_m - c["metrics"]).max())
    rows = c["perms"][0].astype(np.int64)
    failures = []
    checked, measured = _check_recorded(c, rec, "big20")
    for s, e_total, b_total, bad in checked:
        if e_total > b_total:
            failures.append(("total norm", e_total, b_total))
        if bad:
            x = states[torch.as_tensor(rows).to(gpu_device)]
            _forced_mask_fallback(c, _agent(c, gpu_device).network, x, rows, rec.grads[0], bad, "big20 step 0")
    seen, bad, bound = _check_delta(c, ag.network, p0)
    failures += [("parameter change %s" % n, e, b) for n, e, b in bad]
    print("MEASURED " + json.dumps(dict(case="big20", whole=True, metrics=e_m, delta_worst=max(seen.values()),
                                        delta=seen, delta_bound=dict(zip(sr.PARAMS, bound.tolist())), **measured)))
    assert e_m <= 1e-4, (got_m, c["metrics"])
    assert not failures, failures
