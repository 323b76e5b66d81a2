"""GPU parity of the fused Solver backbone (heist_solver_features, bf16 MFMA) against
SolverNetwork's conv stack (reference networks.py:93-100).

Two references:
  * an emulation in float64 on the CPU that rounds exactly where the kernel rounds
    (bf16 input, bf16 conv weights, bf16 activations after each ReLU, fp32 biases and
    accumulation): the kernel must agree to accumulation-order noise;
  * the plain fp32 torch forward (what the reference computes): agreement within the
    bf16 precision of the operands (tolerances stated per test).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from heist_amd.agents import SolverAgent
from heist_amd.networks import SolverNetwork
from policy_ref import (TOL_EMU_MAX, TOL_EMU_MEAN, TOL_F32_MAX, _big_heads, _rel, emulate_backbone, emulate_head,
                        env_obs)

pytestmark = pytest.mark.gpu


def torch_backbone(net, obs):
    with torch.no_grad():
        x = F.relu(net.conv1(obs))
        x = F.relu(net.conv2(x))
        x = F.relu(net.conv3(x))
        return net.pool(x).reshape(obs.shape[0], -1)


@pytest.mark.parametrize("R,n", [(20, 64), (20, 1), (20, 300), (10, 77), (32, 64), (32, 1), (32, 300)])
def test_features_match_emulation(gpu_device, R, n):
    torch.manual_seed(R * 1000 + n)
    net = SolverNetwork(R, R).to(gpu_device)
    for conv in (net.conv1, net.conv2, net.conv3):  # non-trivial biases of both signs
        torch.nn.init.uniform_(conv.bias, -0.3, 0.3)
    obs = env_obs(n, R, gpu_device, seed=n)
    got = net.features_fused(obs)
    ref = emulate_backbone(net, obs)
    assert got.shape == (n, 1024) and torch.isfinite(got).all()
    mx, mean = _rel(got, ref)
    assert mx < TOL_EMU_MAX and mean < TOL_EMU_MEAN, (mx, mean)


def test_features_random_inputs_and_weights(gpu_device):
    """Inputs outside the env's value set (normal noise), negative pre-activations."""
    torch.manual_seed(7)
    net = SolverNetwork().to(gpu_device)
    obs = torch.randn(48, 3, 20, 20, device=gpu_device)
    mx, mean = _rel(net.features_fused(obs), emulate_backbone(net, obs))
    assert mx < TOL_EMU_MAX and mean < TOL_EMU_MEAN, (mx, mean)


def test_features_close_to_fp32_full_batch(gpu_device):
    """4096 envs (the bench batch: 16 envs per workgroup) against the fp32 torch path."""
    torch.manual_seed(3)
    net = SolverNetwork().to(gpu_device)
    obs = env_obs(4096, 20, gpu_device, seed=11, steps=3)
    got = net.features_fused(obs)
    ref = torch_backbone(net, obs)
    mx, _ = _rel(got, ref)
    assert mx < TOL_F32_MAX, mx
    # every env row was written (rows are independent: compare a spread of them exactly
    # against the emulation too)
    rows = torch.tensor([0, 1, 255, 256, 257, 1023, 2048, 4095], device=gpu_device)
    mx, mean = _rel(got[rows], emulate_backbone(net, obs[rows]))
    assert mx < TOL_EMU_MAX and mean < TOL_EMU_MEAN, (mx, mean)


def test_features_32x32_full_batch(gpu_device):
    """BASELINE C5's 2048 envs of 32x32 (row-band kernel: 4 bands of 8 rows per env) against
    the fp32 torch path, and a spread of rows against the emulation; random inputs too."""
    torch.manual_seed(13)
    net = SolverNetwork(32, 32).to(gpu_device)
    for conv in (net.conv1, net.conv2, net.conv3):
        torch.nn.init.uniform_(conv.bias, -0.3, 0.3)
    obs = env_obs(2048, 32, gpu_device, seed=21, steps=3)
    got = net.features_fused(obs)
    mx, _ = _rel(got, torch_backbone(net, obs))
    assert mx < TOL_F32_MAX, mx
    rows = torch.tensor([0, 1, 255, 256, 257, 1023, 1024, 2047], device=gpu_device)
    mx, mean = _rel(got[rows], emulate_backbone(net, obs[rows]))
    assert mx < TOL_EMU_MAX and mean < TOL_EMU_MEAN, (mx, mean)
    x = torch.randn(40, 3, 32, 32, device=gpu_device)
    mx, mean = _rel(net.features_fused(x), emulate_backbone(net, x))
    assert mx < TOL_EMU_MAX and mean < TOL_EMU_MEAN, (mx, mean)


def test_repack_after_weight_update(gpu_device):
    torch.manual_seed(5)
    net = SolverNetwork().to(gpu_device)
    obs = env_obs(16, 20, gpu_device)
    a = net.features_fused(obs)
    with torch.no_grad():
        net.conv2.weight.mul_(0.5)  # in-place, as an optimizer step does
    b = net.features_fused(obs)
    assert not torch.allclose(a, b)
    mx, mean = _rel(b, emulate_backbone(net, obs))
    assert mx < TOL_EMU_MAX and mean < TOL_EMU_MEAN, (mx, mean)


def test_forward_fused_matches_forward(gpu_device):
    torch.manual_seed(9)
    net = SolverNetwork().to(gpu_device)
    for m in net.modules():  # larger head weights than the 0.01-gain init so logits are not ~0
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.orthogonal_(m.weight, gain=1.0)
    obs = env_obs(256, 20, gpu_device, seed=4)
    h = torch.randn(1, 256, 128, device=gpu_device) * 0.1
    c = torch.randn(1, 256, 128, device=gpu_device) * 0.1
    with torch.no_grad():
        l_ref, v_ref, (h_ref, c_ref) = net(obs, (h, c))
    l_got, v_got, (h_got, c_got) = net.forward_fused(obs, (h, c))
    for got, ref in ((l_got, l_ref), (v_got, v_ref), (h_got, h_ref), (c_got, c_ref)):
        mx, _ = _rel(got, ref)
        assert mx < TOL_F32_MAX, mx


def test_agent_act_uses_fused_path_and_fallback(gpu_device):
    """act() takes the kernel for 20x20 when bf16 is opted into, and the fp32 torch path
    by default and where the kernel does not apply."""
    torch.manual_seed(1)
    ag0 = SolverAgent(20, 20, device=gpu_device)
    assert ag0.rollout_precision == "fp32"
    ag0.act(env_obs(8, 20, gpu_device))
    assert not hasattr(ag0.network, "_pack_cache")  # parity default: no bf16 kernel
    ag = SolverAgent(20, 20, device=gpu_device, rollout_precision="bf16")
    obs = env_obs(32, 20, gpu_device)
    a, lp, v, (h, c) = ag.act(obs)
    assert a.shape == (32,) and ((a >= 0) & (a < 5)).all() and torch.isfinite(lp).all()
    assert hasattr(ag.network, "_pack_cache")
    ag16 = SolverAgent(16, 16, device=gpu_device, rollout_precision="bf16")
    o16 = torch.rand(4, 3, 16, 16, device=gpu_device)
    a16, lp16, _, _ = ag16.act(o16)
    assert not hasattr(ag16.network, "_pack_cache") and a16.shape == (4,)
    # same logits both ways up to bf16 precision -> log-probs of the taken actions agree
    a_ref, lp_ref, _, _ = ag.act(obs, fused=False)
    logits_f, _, _ = ag.network.forward_fused(obs)
    with torch.no_grad():
        logits_r, _, _ = ag.network(obs)
    assert (F.log_softmax(logits_f, -1) - F.log_softmax(logits_r, -1)).abs().max().item() < 1e-3


def test_unsupported_grid_rejected(gpu_device):
    from heist_amd import _native
    net = SolverNetwork(16, 16).to(gpu_device)
    with pytest.raises(_native.HeistError):
        net.features_fused(torch.zeros(2, 3, 16, 16, device=gpu_device))


# ---------------------------------------------------------------------------------
# fused head: fc_spatial + LSTM cell + heads + Categorical sample (heist_solver_head)
# ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 33, 4096])
def test_head_matches_emulation(gpu_device, n):
    torch.manual_seed(n)
    net = _big_heads(SolverNetwork().to(gpu_device))
    obs = env_obs(n, 20, gpu_device, seed=n + 1)
    feat = net.features_fused(obs)
    h = torch.randn(1, n, 128, device=gpu_device) * 0.5
    c = torch.randn(1, n, 128, device=gpu_device) * 0.5
    a, lp, v, (h1, c1), lg = net.act_fused(obs, (h, c), seed=1, counter=2, want_logits=True)
    rows = torch.arange(n) if n <= 64 else torch.tensor([0, 1, 31, 32, 1000, 2047, 4064, 4095])
    r_lg, r_v, r_h, r_c = emulate_head(net, feat[rows.to(gpu_device)], h[0, rows], c[0, rows])
    for got, ref in ((lg[rows.to(gpu_device)], r_lg), (v[rows.to(gpu_device)], r_v),
                     (h1[0, rows.to(gpu_device)], r_h), (c1[0, rows.to(gpu_device)], r_c)):
        mx, mean = _rel(got, ref)
        assert mx < TOL_EMU_MAX and mean < TOL_EMU_MEAN, (mx, mean)
    # log-prob of the sampled action under Categorical(softmax(logits)) (torch semantics)
    ref_lp = torch.distributions.Categorical(F.softmax(lg, -1)).log_prob(a)
    assert (lp - ref_lp).abs().max().item() < 1e-5
    assert ((a >= 0) & (a < 5)).all()


def test_head_zero_state_and_reference_forward(gpu_device):
    """hidden=None is the zero state; the whole fused act tracks the fp32 forward over a
    3-step LSTM rollout within bf16 precision."""
    torch.manual_seed(21)
    net = _big_heads(SolverNetwork().to(gpu_device))
    obs = [env_obs(128, 20, gpu_device, seed=s) for s in range(3)]
    hid_f = hid_r = None
    for o in obs:
        a, lp, v, hid_f, lg = net.act_fused(o, hid_f, want_logits=True)
        with torch.no_grad():
            l_ref, v_ref, hid_r = net(o, hid_r)
        assert _rel(lg, l_ref)[0] < TOL_F32_MAX
        assert _rel(v, v_ref.reshape(-1))[0] < TOL_F32_MAX
        assert _rel(hid_f[0], hid_r[0])[0] < TOL_F32_MAX and _rel(hid_f[1], hid_r[1])[0] < TOL_F32_MAX


def test_head_sampling_distribution(gpu_device):
    """Actions follow softmax(logits): aggregated counts over 4096 envs x 16 draws match
    the summed probabilities (chi-square, 4 dof); draws are deterministic in (seed,
    counter) and differ across counters."""
    torch.manual_seed(8)
    net = _big_heads(SolverNetwork().to(gpu_device))
    obs = env_obs(4096, 20, gpu_device, seed=3)
    counts = torch.zeros(5, dtype=torch.float64)
    expect = torch.zeros(5, dtype=torch.float64)
    acts = []
    for k in range(16):
        a, lp, v, _, lg = net.act_fused(obs, None, seed=77, counter=k, want_logits=True)
        counts += torch.bincount(a.cpu(), minlength=5).double()
        expect += F.softmax(lg.double(), -1).sum(0).cpu()
        acts.append(a)
    chi2 = (((counts - expect) ** 2) / expect).sum().item()
    assert chi2 < 25.0, (chi2, counts, expect)  # p ~ 5e-5 at 4 dof
    a_again, *_ = net.act_fused(obs, None, seed=77, counter=3)
    assert torch.equal(a_again, acts[3])
    assert not torch.equal(acts[0], acts[1])


def test_fp32_gpu_forward_matches_reference_golden(gpu_device):
    """The default (fp32) rollout forward on the GPU, channels-last as the agent keeps it,
    against the reference's seeded SolverNetwork outputs (networks.py:76-131, nets.npz),
    within the north-star 1e-4."""
    import golden_data as gd
    z = gd.load("nets.npz")
    ag = SolverAgent(20, 20, device=gpu_device)
    sd = {k[len("solver/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("solver/")}
    ag.network.load_state_dict(sd)
    x = torch.from_numpy(z["solver_in"]).to(gpu_device)
    h = (torch.from_numpy(z["solver_h"]).to(gpu_device), torch.from_numpy(z["solver_c"]).to(gpu_device))
    with torch.no_grad():
        lg, v, (h1, c1) = ag.network(x, h)
        lg0, v0, _ = ag.network(x)
    for got, key in ((lg, "solver_logits"), (v, "solver_value"), (h1, "solver_h1"), (c1, "solver_c1"),
                     (lg0, "solver_logits0"), (v0, "solver_value0")):
        np.testing.assert_allclose(got.cpu().numpy(), z[key], rtol=0, atol=1e-4, err_msg=key)
    # act() on the default path: log-prob of the sampled action from the same logits
    torch.manual_seed(5)
    a, lp, val, _ = ag.act(x, h)
    ref = F.log_softmax(torch.from_numpy(z["solver_logits"]), -1).gather(1, a.cpu()[:, None]).reshape(-1)
    np.testing.assert_allclose(lp.cpu().numpy(), ref.numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(val.cpu().numpy(), z["solver_value"].reshape(-1), rtol=0, atol=1e-4)
