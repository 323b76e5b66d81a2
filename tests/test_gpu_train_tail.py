"""The four fused-tail kernels of the Solver's fp32 training step (csrc/heist_train.hip:
heist_bias_relu_nhwc, heist_bias_relu_pool_nhwc, heist_pool_relu_bwd_nhwc, heist_relu_bwd_nhwc)
called directly through the C ABI on NHWC fp32 tensors, as networks.py _BackboneF32 calls them,
against float64 references (relu(x + b), adaptive_avg_pool2d, its autograd times the ReLU mask,
the masked gradient's sums) at the smallest shapes that reach each code path.

Rules: an output that is one rounding or a select is bit-equal to its fp32 restatement; the zero
pattern of a masked output equals (y > 0); an output that is a sum is within 1e-5 of the max
|float64 reference| of its tensor (fp32 summation order only, the convention of _close in
test_gpu_train_backbone.py).  Every output and in-place buffer carries one extra sample (or row)
of a sentinel after the n the call is given, which must come back untouched.

Inputs: pre-activations roughly half negative, and in every sample a few planted positions (for
the pool pair one in every pool cell) that hold, in both channel halves, a pre-activation of
exactly +0.0 (x == -bias), of -0.0, and of the smallest normal float32; no subnormals."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from heist_amd import _native as nat

pytestmark = pytest.mark.gpu

EINVAL = 100000  # HEIST_EINVAL
TINY = np.float32(1.17549435e-38)  # the smallest normal float32
SENT = -777.25  # negative: relu(SENT + b) != SENT for every bias, so a stray in-place pass shows
SUM_TOL = 1e-5


def _P(t, byte_offset=0):
    return nat._vp(t.data_ptr() + byte_offset)


def _edge_channels(C):
    """(channels planted with x == -bias, with -0.0, with the smallest normal): some in each half."""
    if C >= 8:
        return [0, C // 2], [1, C // 2 + 1], [2, C // 2 + 2]
    return [0, C // 2], [1], [3]


def _bias(C, rng):
    z0, nz, tiny = _edge_channels(C)
    b = rng.normal(0, 0.5, C).astype(np.float32)
    b[nz] = -0.0  # x + b is -0.0 only if both are
    b[tiny] = 0.0
    return b


def _preact(n, P, C, b, rng, planted):
    """x [n, P, C] float32 with the edge pre-activations at the planted positions."""
    z0, nz, tiny = _edge_channels(C)
    x = rng.normal(size=(n, P, C)).astype(np.float32)
    for p in planted:
        x[:, p, z0] = -b[z0]
        x[:, p, nz] = -0.0
        x[:, p, tiny] = TINY
    z = x + b
    assert z.dtype == np.float32
    for p in planted:
        assert (z[:, p, z0] == 0).all() and not np.signbit(z[:, p, z0]).any()
        assert (z[:, p, nz] == 0).all() and np.signbit(z[:, p, nz]).all()
        assert (z[:, p, tiny] == TINY).all()
    assert not ((z != 0) & (np.abs(z) < TINY)).any(), "no subnormal pre-activations"
    neg = float((z < 0).mean())
    assert P * C * n < 256 or 0.3 < neg < 0.7
    return x


def _saved_output(n, P, C, rng, planted):
    """y [n, P, C]: a ReLU output as the forward saves it, with exact 0.0, -0.0 and the smallest
    normal at the planted positions."""
    b = _bias(C, rng)
    y = np.maximum(_preact(n, P, C, b, rng, planted) + b, np.float32(0))
    z0, nz, tiny = _edge_channels(C)
    for p in planted:
        y[:, p, nz] = -0.0
        assert (y[:, p, z0] == 0).all() and (y[:, p, tiny] == TINY).all()
    return y


def _win(i, n):
    """torch's adaptive_avg_pool2d window [start, end) of output cell i of 4 over n inputs."""
    return (i * n) // 4, -((-(i + 1) * n) // 4)


def _cell_corners(R, W):
    return sorted({_win(cy, R)[0] * W + _win(cx, W)[0] for cy in range(4) for cx in range(4)})


def _with_tail(a, dev):
    """a on the device followed, in the same allocation, by one more sample (row) of SENT;
    returns (whole buffer, the view the kernel is given, the tail)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    full = torch.full((t.shape[0] + 1,) + tuple(t.shape[1:]), SENT, dtype=t.dtype)
    full[:-1] = t
    full = full.to(dev)
    return full, full[:-1], full[-1]


def _sentinel_buf(n_used, n_extra, dev):
    full = torch.full((n_used + n_extra,), SENT, dtype=torch.float32, device=dev)
    return full, full[n_used:]


def _untouched(tail):
    return bool((tail == SENT).all())


def _assert_sum_close(got, want64, what):
    scale = float(want64.abs().max())
    err = float((got.detach().cpu().double() - want64).abs().max())
    print("%s: max |diff| %.3g, max |float64 reference| %.3g (ratio %.3g)" % (what, err, scale, err / max(scale, 1e-300)))
    assert err <= SUM_TOL * scale, "%s: max |diff| %.3g vs scale %.3g" % (what, err, scale)


POOL_SHAPES = [(4, 4, 1), (8, 8, 3), (20, 20, 17), (5, 7, 5), (8, 6, 5), (6, 8, 5), (13, 17, 9), (10, 10, 600),
               (64, 64, 3)]


@pytest.mark.parametrize("R,W,n", POOL_SHAPES)
def test_bias_relu_pool(gpu_device, R, W, n):
    """y = relu(x + b) in place, bit-equal to the fp32 restatement, its zero pattern float64's;
    the pooled features within 1e-5 of the max of float64's adaptive_avg_pool2d (bit-equal to y
    at window area 1); nothing written past sample n."""
    C = 64
    rng = np.random.default_rng(R * 100 + W)
    b = _bias(C, rng)
    x = _preact(n, R * W, C, b, rng, _cell_corners(R, W)).reshape(n, R, W, C)
    xfull, xd, xtail = _with_tail(x, gpu_device)
    ffull = torch.full((n + 1, C * 16), SENT, device=gpu_device)
    bd = torch.from_numpy(b).to(gpu_device)
    nat.check(nat.lib().heist_bias_relu_pool_nhwc(_P(xd), _P(bd), n, R, W, C, _P(ffull), nat.stream(gpu_device)),
              "heist_bias_relu_pool_nhwc")
    y = xd.cpu()
    xt, bt = torch.from_numpy(x), torch.from_numpy(b)
    assert torch.equal(y, torch.relu(xt + bt)), "y is not relu(x + b) rounded once"
    y64 = torch.relu(xt.double() + bt.double())
    assert torch.equal(y > 0, y64 > 0)
    want = F.adaptive_avg_pool2d(y64.permute(0, 3, 1, 2), (4, 4)).reshape(n, -1)
    feat = ffull[:n].cpu()
    if (R, W) == (4, 4):
        assert torch.equal(feat, y.permute(0, 3, 1, 2).reshape(n, -1)), "window area 1: the feature is y itself"
    _assert_sum_close(feat, want, "pooled features %dx%d" % (R, W))
    assert _untouched(xtail) and _untouched(ffull[n]), "wrote past sample n"


@pytest.mark.parametrize("R,W,n", POOL_SHAPES)
def test_pool_relu_bwd(gpu_device, R, W, n):
    """d_out = (y > 0) * (the pool's input gradient of dfeat): its zero pattern (y > 0) exactly;
    bit-equal to the single division dfeat / area where the windows are disjoint, else within
    1e-5 of the max of float64 autograd's (at most 4 terms); dbias_out within 1e-5 of the max of
    the float64 sums; partial exactly [n][64] floats; nothing written past sample n."""
    C = 64
    rng = np.random.default_rng(R * 100 + W + 7)
    y = _saved_output(n, R * W, C, rng, _cell_corners(R, W)).reshape(n, R, W, C)
    dfeat = rng.normal(size=(n, C * 16)).astype(np.float32)
    yd = torch.from_numpy(y).to(gpu_device)
    fd = torch.from_numpy(dfeat).to(gpu_device)
    dfull = torch.full((n + 1, R, W, C), SENT, device=gpu_device)
    pfull, ptail = _sentinel_buf(n * C, C, gpu_device)
    bfull, btail = _sentinel_buf(C, C, gpu_device)
    nat.check(nat.lib().heist_pool_relu_bwd_nhwc(_P(fd), _P(yd), n, R, W, C, _P(dfull), _P(pfull), _P(bfull),
                                                  nat.stream(gpu_device)), "heist_pool_relu_bwd_nhwc")
    d = dfull[:n].cpu()
    yt, ft = torch.from_numpy(y), torch.from_numpy(dfeat)
    mask = yt > 0
    assert torch.equal(d != 0, mask), "zero pattern of d_out is not (y > 0)"
    yy = yt.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    F.adaptive_avg_pool2d(yy, (4, 4)).reshape(n, -1).backward(ft.double())
    want = (yy.grad * (yy.detach() > 0)).permute(0, 2, 3, 1)
    if R % 4 == 0 and W % 4 == 0:
        kh, kw = R // 4, W // 4
        g = (ft / torch.tensor(float(kh * kw), dtype=torch.float32)).reshape(n, C, 4, 4)
        g = g.repeat_interleave(kh, 2).repeat_interleave(kw, 3).permute(0, 2, 3, 1)
        assert torch.equal(d, torch.where(mask, g, torch.zeros(()))), "disjoint windows: d_out is one division"
    _assert_sum_close(d, want, "d_out %dx%d" % (R, W))
    _assert_sum_close(bfull[:C], want.sum((0, 1, 2)), "dbias_out %dx%d n=%d" % (R, W, n))
    assert _untouched(dfull[n]) and _untouched(ptail) and _untouched(btail), "wrote past its outputs"
    assert not bool((pfull[:n * C] == SENT).any()), "partial [n][64] is written in full"


@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("P", [1, 7, 16, 221, 400])
@pytest.mark.parametrize("C", [32, 64])
def test_relu_bwd(gpu_device, C, P, n):
    """g = (y > 0) ? g : 0 in place, bit-equal to the select and zero exactly where y <= 0
    (y = 0.0, -0.0 and the smallest normal included); dbias_out within 1e-5 of the max of the
    float64 sums.  P = 7 and 16 leave position lanes idle (32 lanes at 32 channels, 16 at 64)."""
    rng = np.random.default_rng(C * 1000 + P)
    y = _saved_output(n, P, C, rng, sorted({0, P // 2, P - 1}))
    g = rng.normal(size=(n, P, C)).astype(np.float32)
    yd = torch.from_numpy(y).to(gpu_device)
    gfull, gd, gtail = _with_tail(g, gpu_device)
    pfull, ptail = _sentinel_buf(n * C, C, gpu_device)
    bfull, btail = _sentinel_buf(C, C, gpu_device)
    nat.check(nat.lib().heist_relu_bwd_nhwc(_P(gd), _P(yd), n, P, C, _P(pfull), _P(bfull), nat.stream(gpu_device)),
              "heist_relu_bwd_nhwc")
    yt, gt = torch.from_numpy(y), torch.from_numpy(g)
    mask = yt > 0
    got = gd.cpu()
    assert torch.equal(got, torch.where(mask, gt, torch.zeros(()))), "masked g is not the select"
    assert torch.equal(got != 0, mask), "zero pattern of g is not (y > 0)"
    want = (gt.double() * mask).sum((0, 1))
    _assert_sum_close(bfull[:C], want, "dbias_out C=%d P=%d n=%d" % (C, P, n))
    assert _untouched(gtail) and _untouched(ptail) and _untouched(btail), "wrote past its outputs"
    assert torch.equal(yd.cpu(), yt), "y is read-only"


@pytest.mark.parametrize("n_pos", [1, 255, 1031])
@pytest.mark.parametrize("C", [4, 12, 32, 64])
def test_bias_relu(gpu_device, C, n_pos):
    """x = relu(x + b) in place for every channel count the ABI accepts (multiples of 4), bit-equal
    to the fp32 restatement, the zero pattern float64's; nothing written past row n_pos."""
    rng = np.random.default_rng(C * 10000 + n_pos)
    b = _bias(C, rng)
    x = _preact(1, n_pos, C, b, rng, sorted({0, n_pos // 2, n_pos - 1}))[0]
    xfull, xd, xtail = _with_tail(x, gpu_device)
    bd = torch.from_numpy(b).to(gpu_device)
    nat.check(nat.lib().heist_bias_relu_nhwc(_P(xd), _P(bd), n_pos, C, nat.stream(gpu_device)), "heist_bias_relu_nhwc")
    xt, bt = torch.from_numpy(x), torch.from_numpy(b)
    y = xd.cpu()
    assert torch.equal(y, torch.relu(xt + bt)), "y is not relu(x + b) rounded once"
    assert torch.equal(y > 0, (xt.double() + bt.double()) > 0)
    assert _untouched(xtail), "wrote past row n_pos"
    assert torch.equal(bd.cpu(), bt), "the bias is read-only"


def test_bias_relu_past_the_block_clamp(gpu_device):
    """12 channels and n_pos * 12 / 4 = 65,536 * 256 + 77 float4s: past the 65,536-block clamp,
    so every thread takes a second grid-stride step, with a stride (16,777,216) that the 3
    float4s of a position do not divide: the bias quad changes between a thread's steps.  About
    270 MB; the reference is torch's own fp32 relu(x + b) on the device, bit for bit."""
    C = 12
    n4 = 65536 * 256 + 77
    assert n4 % (C // 4) == 0 and (65536 * 256) % (C // 4) != 0
    n_pos = n4 // (C // 4)
    gen = torch.Generator(device=gpu_device).manual_seed(12)
    full = torch.randn((n_pos + 1, C), device=gpu_device, generator=gen)
    full[-1] = SENT
    x = full[:-1]
    b = torch.from_numpy(_bias(C, np.random.default_rng(12))).to(gpu_device)
    z0, nz, tiny = _edge_channels(C)
    for p in (0, 65536 * 256 // 3, 65536 * 256 // 3 + 1, n_pos - 1):  # around the second step's start
        x[p, z0] = -b[z0]
        x[p, nz] = -0.0
        x[p, tiny] = float(TINY)
    want = torch.relu(x + b)
    nat.check(nat.lib().heist_bias_relu_nhwc(_P(x), _P(b), n_pos, C, nat.stream(gpu_device)), "heist_bias_relu_nhwc")
    assert torch.equal(x, want)
    assert bool((want[65536 * 256 // 3 + 2:] > 0).any()) and bool((want[65536 * 256 // 3 + 2:] == 0).any())
    assert _untouched(full[-1]), "wrote past row n_pos"


def _einval_cases():
    """(id, function name, argument builder): each must return HEIST_EINVAL and write nothing."""
    def bias_relu(C=64, off=0):
        return lambda t: ("heist_bias_relu_nhwc", (_P(t["x"], off), _P(t["b"]), 16, C))

    def pool(R=8, C=64, off=0):
        return lambda t: ("heist_bias_relu_pool_nhwc", (_P(t["x"], off), _P(t["b"]), 2, R, 8, C, _P(t["feat"])))

    def pool_bwd(R=8, C=64, off=0):
        return lambda t: ("heist_pool_relu_bwd_nhwc", (_P(t["feat"]), _P(t["y"]), 2, R, 8, C, _P(t["x"], off),
                                                       _P(t["part"]), _P(t["db"])))

    def relu_bwd(C=64, off=0):
        return lambda t: ("heist_relu_bwd_nhwc", (_P(t["x"], off), _P(t["y"]), 2, 64, C, _P(t["part"]), _P(t["db"])))

    return [("bias_relu_6_channels", bias_relu(C=6)), ("pool_48_channels", pool(C=48)),
            ("pool_bwd_48_channels", pool_bwd(C=48)), ("pool_3_rows", pool(R=3)), ("pool_bwd_3_rows", pool_bwd(R=3)),
            ("relu_bwd_16_channels", relu_bwd(C=16)), ("bias_relu_pointer_plus_4", bias_relu(off=4)),
            ("pool_pointer_plus_4", pool(off=4)), ("pool_bwd_pointer_plus_4", pool_bwd(off=4)),
            ("relu_bwd_pointer_plus_4", relu_bwd(off=4))]


@pytest.mark.parametrize("case", _einval_cases(), ids=[c[0] for c in _einval_cases()])
def test_argument_checks_return_einval_and_write_nothing(gpu_device, case):
    sizes = {"x": 2 * 8 * 8 * 64 + 64, "y": 2 * 8 * 8 * 64, "b": 64, "feat": 2 * 1024, "part": 2 * 64, "db": 64}
    t = {k: torch.full((v,), SENT, device=gpu_device) for k, v in sizes.items()}
    name, args = case[1](t)
    rc = getattr(nat.lib(), name)(*args, nat.stream(gpu_device))
    assert rc == EINVAL, (name, rc, nat.lib().heist_last_error())
    torch.cuda.synchronize(gpu_device)
    for k, v in t.items():
        assert _untouched(v), "%s wrote to %s" % (name, k)
