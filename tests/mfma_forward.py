"""The Solver backbone's fp32-MFMA forward through the C ABI, for the GPU tests that need its
ReLU masks (tests/test_gpu_train_backbone.py, tests/test_gpu_solver_update_golden.py)."""

import torch


def mfma_forward(net, x):
    """The fp32-MFMA forward through the C ABI (the passes _BackboneMFMA32 runs, deterministic):
    the [n][R][C][P] activations a1, a2, a3."""
    from heist_amd import _native as nat
    from heist_amd.networks import _tc_act, _tc_queues
    L, st, dev = nat.lib(), nat.stream(x.device), x.device
    n, _, R, C = x.shape
    P = lambda t: nat._vp(t.data_ptr())  # noqa: E731
    q = _tc_queues(dev)
    x4 = _tc_act(n, R, C, 3, dev)
    s = x.stride()
    nat.check(L.heist_train_obs_nhwc4(P(x), n, R, C, s[0], s[1], s[2], s[3], P(x4), st), "obs")
    ys, xin = [], x4
    for layer, m, ch in ((1, net.conv1, 32), (2, net.conv2, 64), (3, net.conv3, 64)):
        f = torch.empty(L.heist_train_conv_frag_floats(layer, 0), device=dev)
        nat.check(L.heist_train_conv_pack(layer, 0, P(m.weight.detach().contiguous()), P(f), st), "pack")
        y = _tc_act(n, R, C, ch, dev)
        nat.check(L.heist_train_conv(layer, 0, P(xin), n, R, C, P(f), P(m.bias.detach().contiguous()), None, P(y),
                                     P(q), st), "conv")
        ys.append(y[..., :ch].permute(0, 3, 1, 2))
        xin = y
    torch.cuda.synchronize(dev)
    return ys
