"""Exact checks of the fused bf16 Solver policy kernels (csrc/heist_policy.hip), called
through the C ABI (heist_solver_pack / heist_solver_features / heist_solver_head_pack /
heist_solver_head), not through SolverNetwork's caches.

  * backbone: with the small-integer case of tests/policy_ref.py every product and partial sum
    is an integer far below 2^24, so the kernel must equal the float64 reference bit for bit
    (32 x 32: the pool divides by 64) or within the one ulp that multiplying by fp32 1/area
    instead of dividing costs (20 x 20, 10 x 10);
  * head: every supported action count and partial blocks of 32 envs against the emulation,
    sentinels past row n - 1 of every output, the NULL combinations of the optional
    pointers, and the sampled action per env against the draw as include/heist.h states it.
No expected value comes from the kernels under test."""
import numpy as np
import pytest
import torch

from heist_amd import _native as nat
from heist_amd.networks import SolverNetwork
import policy_ref as pr
from policy_ref import TOL_EMU_MAX, TOL_EMU_MEAN, _big_heads, _rel, emulate_head

pytestmark = pytest.mark.gpu

EINVAL = 100000  # HEIST_EINVAL
SENT_BITS = 0x7FC5A5A5  # a quiet NaN with a payload no kernel produces
SENT_I64 = -0x0123456789ABCDEF
DELTA = 1e-5  # the fp32 __expf softmax and a 7-term running sum keep the CDF within ~1e-6 of float64
MAX_EXCLUDED = 0.005


def _sentinel(dev, *shape):
    return torch.full(shape, SENT_BITS, dtype=torch.int32, device=dev).view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _is_sentinel(t):
    if t.dtype == torch.int64:
        return bool((t == SENT_I64).all())
    return bool((_bits(t) == SENT_BITS).all())


# ---------------------------------------------------------------------------------
# backbone
# ---------------------------------------------------------------------------------

FEAT_PAD = 8


def _pack_backbone(dev, params, packed=None, dst=None):
    """heist_solver_pack of (w1, b1, w2, b2, w3, b3); with dst, the device parameter tensors
    are overwritten in place first and packed from the same addresses again."""
    L = nat.lib()
    if dst is None:
        dst = [p.to(dev).contiguous() for p in params]
    else:
        for d, p in zip(dst, params):
            d.copy_(p)
    if packed is None:
        packed = torch.zeros(L.heist_solver_packed_bytes(), dtype=torch.uint8, device=dev)
    nat.check(L.heist_solver_pack(*(nat.ptr(t) for t in dst), nat.ptr(packed), nat.stream(dev)), "heist_solver_pack")
    return packed, dst


def _features(dev, obs, packed):
    """heist_solver_features into a buffer with FEAT_PAD sentinel rows after row n - 1."""
    n, _, R, C = obs.shape
    x = obs.to(dev).contiguous()
    feat = _sentinel(dev, n + FEAT_PAD, 1024)
    nat.check(nat.lib().heist_solver_features(nat.ptr(x), n, R, C, nat.ptr(packed), nat.ptr(feat), nat.stream(dev)),
              "heist_solver_features")
    torch.cuda.synchronize(dev)
    assert _is_sentinel(feat[n:]), "heist_solver_features wrote past row n - 1"
    return feat[:n].cpu()


def _assert_features_exact(got, sums, area, R, what=""):
    """got [n,1024] float32 against the exact window sums: bit-equal to float32(sum / 64) at
    32 x 32, within one fp32 ulp of the correctly rounded sum / area otherwise."""
    n = got.shape[0]
    assert bool(torch.isfinite(got).all()), what
    gb = got.numpy().view(np.int32).astype(np.int64)
    assert (gb >= 0).all(), "%s sign bit set at (env, channel, cell) %s" % (
        what, [(int(e), int(k) // 16, int(k) % 16) for e, k in zip(*np.nonzero(gb < 0))][:4])
    exp = pr.quotient_f32(sums.numpy(), np.broadcast_to(area.numpy(), (n, 1024)))
    if R == 32:
        assert np.array_equal(exp.astype(np.float64) * 64.0, sums.numpy())  # / 64 is exact
    ulps = np.abs(gb - exp.view(np.int32).astype(np.int64))
    bad = ulps > (0 if R == 32 else 1)
    if bad.any():
        e, k = (int(v[0]) for v in np.nonzero(bad))
        pytest.fail("%s R=%d n=%d: %d of %d elements wrong; first at env %d, channel %d, cell %d (row %d, col %d): "
                    "got %r, expected %r (sum %d / area %d); envs affected %d, channels affected %d"
                    % (what, R, n, int(bad.sum()), bad.size, e, k // 16, k % 16, (k % 16) // 4, k % 4,
                       float(got[e, k]), float(exp[e, k]), int(sums[e, k]), int(area[k]),
                       int(bad.any(1).sum()), int(bad.reshape(n, 64, 16).any((0, 2)).sum())))
    return int(ulps.max())


_cases = {}


def _big_case(R, cu):
    """One reference per grid size for the largest n, sliced by the smaller ones."""
    if R not in _cases:
        _cases[R] = pr.integer_case(R, 2 * cu + 1)
        c = _cases[R].cond
        print("integer_case R=%d n=%d: bound=%s pool_bound=%g fire=%s rounded=%s ties=%s"
              % (R, 2 * cu + 1, c.bound, c.pool_bound, ["%.3f" % v for v in c.fire],
                 ["%.4f" % v for v in c.rounded], c.ties))
        assert all(b < 2 ** 24 for b in c.bound) and c.pool_bound < 2 ** 24
    return _cases[R]


def _n_of(which, cu):
    return {"1": 1, "2": 2, "cu-1": cu - 1, "cu": cu, "cu+1": cu + 1, "2cu+1": 2 * cu + 1}[which]


@pytest.mark.parametrize("which", ["1", "2", "cu-1", "cu", "cu+1", "2cu+1"])
@pytest.mark.parametrize("R", [10, 20, 32])
def test_features_integer_exact(gpu_device, R, which):
    """min(n, cu) persistent workgroups: one env each (n <= cu), exactly one workgroup with a
    prefetched second env under the once-zeroed padding border (cu + 1), a third round
    (2 cu + 1)."""
    cu = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    n = _n_of(which, cu)
    case = _big_case(R, cu)
    packed, _ = _pack_backbone(gpu_device, case.params)
    got = _features(gpu_device, case.obs[:n], packed)
    worst = _assert_features_exact(got, case.sums[:n], case.area, R)
    print("R=%d n=%d (cu=%d): largest distance %d ulp" % (R, n, cu, worst))


@pytest.mark.parametrize("R", [10, 20, 32])
def test_features_integer_exact_after_repack(gpu_device, R):
    """Weights overwritten in place (as an optimizer step does) and packed into the same
    buffer again: the next launch computes with the new ones, exactly."""
    cu = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    a = _big_case(R, cu)
    b = pr.integer_case(R, 3, seed=1)
    assert any(not torch.equal(x, y) for x, y in zip(a.params, b.params))
    packed, dst = _pack_backbone(gpu_device, a.params)
    _assert_features_exact(_features(gpu_device, a.obs[:3], packed), a.sums[:3], a.area, R, "first pack")
    ptrs = [t.data_ptr() for t in dst] + [packed.data_ptr()]
    packed2, dst2 = _pack_backbone(gpu_device, b.params, packed=packed, dst=dst)
    assert [t.data_ptr() for t in dst2] + [packed2.data_ptr()] == ptrs
    _assert_features_exact(_features(gpu_device, b.obs, packed), b.sums, b.area, R, "after re-pack")


# float32 weights whose bf16 rounding tells the modes apart: value -> round-to-nearest-even
RNE_CASES = [
    (1.0 + 2.0 ** -8, 1.0),                            # tie, down to even (half-up: 1 + 2^-7)
    (1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -6),            # tie, up to even (truncation: 1 + 2^-7)
    (1.0 + 2.0 ** -8 + 2.0 ** -16, 1.0 + 2.0 ** -7),   # just above a tie (truncation: 1)
    (1.0 + 3 * 2.0 ** -8 - 2.0 ** -16, 1.0 + 2.0 ** -7),  # just below a tie
    (0.75 + 2.0 ** -9, 0.75),                          # another binade: tie, down to even
    (0.75 + 3 * 2.0 ** -9, 0.75 + 2.0 ** -7),          # tie, up to even
]


@pytest.mark.parametrize("layer", [0, 1, 2])
def test_pack_is_rne(gpu_device, layer):
    """One-hot input, centre-tap weights: channel k of the layer under test carries RNE_CASES[k]
    and the other two layers pass channel k through with weight 1, so feat[0, 16 k + cell] is
    the packed weight / 64 exactly (32 x 32)."""
    R, y, x = 32, 13, 21
    K = len(RNE_CASES)
    vals = torch.tensor([v for v, _ in RNE_CASES], dtype=torch.float32)
    assert vals.double().tolist() == [v for v, _ in RNE_CASES]  # the cases are float32 values
    assert pr._bf(vals).double().tolist() == [r for _, r in RNE_CASES]
    shapes = [(32, 3), (64, 32), (64, 64)]
    params = []
    for li, (co, ci) in enumerate(shapes):
        w = torch.zeros(co, ci, 3, 3)
        for k in range(K):
            w[k, 0 if li == 0 else k, 1, 1] = vals[k] if li == layer else 1.0
        params += [w, torch.zeros(co)]
    obs = torch.zeros(2, 3, R, R)
    obs[0, 0, y, x] = 1.0  # env 1 stays all zero
    packed, _ = _pack_backbone(gpu_device, params)
    got = _features(gpu_device, obs, packed)
    exp = torch.zeros(2, 64, 4, 4, dtype=torch.float64)
    for k, (_, r) in enumerate(RNE_CASES):
        exp[0, k, y // 8, x // 8] = r / 64.0
    exp = exp.reshape(2, 1024).float()
    bad = np.nonzero((_bits(got) != _bits(exp)).numpy())
    assert len(bad[0]) == 0, "layer %d: first mismatch at (env, channel, cell) (%d, %d, %d): got %r * 64, expected %r" % (
        layer, bad[0][0], bad[1][0] // 16, bad[1][0] % 16, float(got[bad[0][0], bad[1][0]]) * 64,
        float(exp[bad[0][0], bad[1][0]]) * 64)


# ---------------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------------

HEAD_PAD = 32


def _head_params(net):
    mods = [net.fc_spatial.weight, net.fc_spatial.bias, net.lstm.weight_ih_l0, net.lstm.weight_hh_l0,
            net.lstm.bias_ih_l0, net.lstm.bias_hh_l0, net.policy_head[0].weight, net.policy_head[0].bias,
            net.value_head[0].weight, net.value_head[0].bias, net.policy_head[2].weight, net.policy_head[2].bias,
            net.value_head[2].weight, net.value_head[2].bias]
    return [t.detach().float().contiguous() for t in mods]


def _pack_head(net, A):
    dev = net.fc_spatial.weight.device
    L = nat.lib()
    packed = torch.zeros(L.heist_solver_head_packed_bytes(), dtype=torch.uint8, device=dev)
    ws = _head_params(net)
    nat.check(L.heist_solver_head_pack(*(nat.ptr(t) for t in ws), A, nat.ptr(packed), nat.stream(dev)),
              "heist_solver_head_pack")
    torch.cuda.synchronize(dev)
    return packed


def _head_outputs(dev, n, A, want_logits=True):
    rows = n + HEAD_PAD
    return dict(logits=_sentinel(dev, rows, A) if want_logits else None, value=_sentinel(dev, rows),
                action=torch.full((rows,), SENT_I64, dtype=torch.int64, device=dev), logp=_sentinel(dev, rows),
                h=_sentinel(dev, rows, 128), c=_sentinel(dev, rows, 128))


def _head(packed, feat, h, c, A, seed=0, counter=0, want_logits=True):
    """heist_solver_head with every output HEAD_PAD sentinel rows longer than n; returns the
    outputs cut to n rows after checking the sentinels."""
    dev, n = feat.device, feat.shape[0]
    out = _head_outputs(dev, n, A, want_logits)
    P = nat.ptr
    nat.check(nat.lib().heist_solver_head(P(feat), P(h), P(c), n, P(packed), A, seed, counter, P(out["logits"]),
                                          P(out["value"]), P(out["action"]), P(out["logp"]), P(out["h"]), P(out["c"]),
                                          nat.stream(dev)), "heist_solver_head")
    torch.cuda.synchronize(dev)
    for k, t in out.items():
        if t is not None:
            assert _is_sentinel(t[n:]), "heist_solver_head wrote past row n - 1 of %s (n=%d, A=%d)" % (k, n, A)
    return {k: (t[:n] if t is not None else None) for k, t in out.items()}


def _head_inputs(dev, n, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    feat = torch.rand(n, 1024, device=dev, generator=g) * 0.5  # pooled ReLU outputs: non-negative
    h = torch.randn(n, 128, device=dev, generator=g) * 0.5
    c = torch.randn(n, 128, device=dev, generator=g) * 0.5
    return feat, h, c


def _assert_matches_emulation(out, net, feat, h, c):
    n = feat.shape[0]
    zeros = torch.zeros(n, 128)
    r_lg, r_v, r_h, r_c = emulate_head(net, feat, zeros if h is None else h, zeros if c is None else c)
    for name, got, ref in (("logits", out["logits"], r_lg), ("value", out["value"], r_v), ("h", out["h"], r_h),
                           ("c", out["c"], r_c)):
        assert bool(torch.isfinite(got).all()), name
        mx, mean = _rel(got, ref)
        assert mx < TOL_EMU_MAX and mean < TOL_EMU_MEAN, (name, mx, mean)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 95])
@pytest.mark.parametrize("A", [1, 2, 3, 5, 7])
def test_head_action_counts(gpu_device, A, n):
    torch.manual_seed(100 * A + n)
    net = _big_heads(SolverNetwork(num_actions=A).to(gpu_device))
    packed = _pack_head(net, A)
    feat, h, c = _head_inputs(gpu_device, n, seed=A * 1000 + n)
    out = _head(packed, feat, h, c, A, seed=5, counter=9)
    assert out["logits"].shape == (n, A)
    _assert_matches_emulation(out, net, feat, h, c)
    a = out["action"].cpu()
    assert bool(((a >= 0) & (a < A)).all()), a
    ref_lp = pr.logp_ref(out["logits"].double().cpu(), a)
    assert (out["logp"].double().cpu() - ref_lp).abs().max().item() < 1e-5
    if A == 1:
        assert bool((a == 0).all())
        one = torch.distributions.Categorical(probs=torch.ones(n, 1)).log_prob(torch.zeros(n, dtype=torch.int64))
        assert one.dtype == torch.float32 and float(one[0]) == float(np.float32(np.log(1.0 - pr.EPS32)))
        assert torch.equal(_bits(out["logp"].cpu()), _bits(one)), (float(out["logp"][0]).hex(), float(one[0]).hex())
    # without logits_out the other five outputs are the same bits
    out0 = _head(packed, feat, h, c, A, seed=5, counter=9, want_logits=False)
    for k in ("value", "logp", "h", "c"):
        assert torch.equal(_bits(out0[k]), _bits(out[k])), k
    assert torch.equal(out0["action"], out["action"])


@pytest.mark.parametrize("use_h,use_c", [(True, False), (False, True), (True, True), (False, False)])
def test_head_null_state_combinations(gpu_device, use_h, use_c):
    """h_in / c_in are independently optional: NULL is the zero state of that input alone."""
    n, A = 33, 5
    torch.manual_seed(41)
    net = _big_heads(SolverNetwork(num_actions=A).to(gpu_device))
    packed = _pack_head(net, A)
    feat, h, c = _head_inputs(gpu_device, n, seed=77)
    h, c = (h if use_h else None), (c if use_c else None)
    out = _head(packed, feat, h, c, A, seed=3, counter=1)
    _assert_matches_emulation(out, net, feat, h, c)
    # and NULL equals an explicit zero state bit for bit
    z = torch.zeros(n, 128, device=gpu_device)
    outz = _head(packed, feat, z if h is None else h, z if c is None else c, A, seed=3, counter=1)
    for k in ("logits", "value", "logp", "h", "c", "action"):
        assert torch.equal(outz[k], out[k]) and (k == "action" or torch.equal(_bits(outz[k]), _bits(out[k]))), k


def _compare_draws(actions, logits64, u, what):
    """actions [n] against sample_ref for every draw at least DELTA from each CDF boundary;
    returns (share excluded, draws compared)."""
    near = pr.near_boundary(logits64, u, DELTA)
    excluded = float(near.mean())
    assert excluded <= MAX_EXCLUDED, (what, excluded)
    ref = pr.sample_ref(logits64, u)
    bad = np.nonzero((actions != ref) & ~near)[0]
    assert len(bad) == 0, "%s: %d of %d draws differ; first at env %d: u=%r, kernel %d, rule %d, CDF %s" % (
        what, len(bad), len(u), bad[0], u[bad[0]], actions[bad[0]], ref[bad[0]],
        np.broadcast_to(pr.cdf_ref(logits64), (len(u), np.shape(logits64)[-1]))[bad[0]].tolist())
    return excluded, int((~near).sum())


KNOWN_BIASES = {2: [0.3, -0.2], 5: [0.5, -0.3, 0.1, -0.7, 0.2], 7: [0.4, -0.6, 0.0, 0.9, -0.2, 0.3, -1.1]}
SEEDS = (0, 2 ** 63 + 12345)
COUNTERS = (0, 1, 2, 3, 2 ** 32 + 5)


def _known_logits_net(dev, A, bias):
    torch.manual_seed(A)
    net = _big_heads(SolverNetwork(num_actions=A).to(dev))
    with torch.no_grad():
        net.policy_head[2].weight.zero_()  # logits = 0 + bias in fp32: the bias itself
        net.policy_head[2].bias.copy_(torch.tensor(bias))
    return net


@pytest.mark.parametrize("A", [2, 5, 7])
def test_head_sample_is_inverse_cdf_known_logits(gpu_device, A):
    """The sampled action of every env, exactly: with a zero last policy layer the CDF is known
    before anything runs, and the draw is a pure function of (seed, counter, env)."""
    n = 4096
    net = _known_logits_net(gpu_device, A, KNOWN_BIASES[A])
    bias32 = net.policy_head[2].bias.detach().cpu()
    logits64 = bias32.double().numpy()
    # the excluded share is a condition on the bias vector, worked out before any launch
    us = {(s, k): pr.head_uniforms(s, k, n) for s in SEEDS for k in COUNTERS}
    share = float(np.mean([pr.near_boundary(logits64, u, DELTA).mean() for u in us.values()]))
    assert share <= MAX_EXCLUDED, share
    packed = _pack_head(net, A)
    feat, h, c = _head_inputs(gpu_device, n, seed=A)
    compared = 0
    for (s, k), u in us.items():
        out = _head(packed, feat, h, c, A, seed=s, counter=k)
        assert torch.equal(out["logits"].cpu(), bias32.expand(n, A))
        a = out["action"].cpu().numpy()
        assert ((a >= 0) & (a < A)).all()
        compared += _compare_draws(a, logits64, u, "A=%d seed=%d counter=%d" % (A, s, k))[1]
        assert (out["logp"].double().cpu() - pr.logp_ref(out["logits"].double().cpu(), a)).abs().max().item() < 1e-5
    print("A=%d: excluded share %.3g (expected about %.3g), %d draws compared"
          % (A, share, 2 * DELTA * (A - 1), compared))


def test_head_sample_is_inverse_cdf_real_logits(gpu_device):
    n, A = 257, 5
    torch.manual_seed(19)
    net = _big_heads(SolverNetwork(num_actions=A).to(gpu_device))
    packed = _pack_head(net, A)
    feat, h, c = _head_inputs(gpu_device, n, seed=23)
    shares = []
    for s in SEEDS:
        for k in COUNTERS:
            out = _head(packed, feat, h, c, A, seed=s, counter=k)
            lg = out["logits"].double().cpu().numpy()
            assert np.ptp(pr.cdf_ref(lg)[:, 0]) > 0.05  # the envs' distributions do differ
            shares.append(_compare_draws(out["action"].cpu().numpy(), lg, pr.head_uniforms(s, k, n),
                                         "seed=%d counter=%d" % (s, k))[0])
    print("real logits: excluded share %.3g over %d draws" % (float(np.mean(shares)), n * len(shares)))


@pytest.mark.parametrize("A", [2, 4])
def test_head_sample_exact_boundaries(gpu_device, A):
    """Equal logits make every p_a = 1/A and every CDF boundary exact in fp32 and float64 alike,
    so no draw is excluded.  (seed 0, counter 210) gives env 1686 u = 0.5 exactly, which sits
    on a boundary and belongs to the action above it (u < CDF is strict); (seed 0, counter 0)
    gives env 0 u = 0.  A -inf logit is a zero-probability action, never drawn even at u = 0."""
    n = 4096
    assert pr.head_uniform(0, 210, 1686) == 0.5 and pr.head_uniform(0, 0, 0) == 0.0
    net = _known_logits_net(gpu_device, A, [0.0] * A)
    packed = _pack_head(net, A)
    feat, h, c = _head_inputs(gpu_device, n, seed=A)
    for counter in (210, 0):
        u = pr.head_uniforms(0, counter, n)
        a = _head(packed, feat, h, c, A, seed=0, counter=counter)["action"].cpu().numpy()
        ref = np.minimum(np.floor(u * A), A - 1).astype(np.int64)  # exact: A is a power of two
        assert np.array_equal(ref, pr.sample_ref(np.zeros(A), u))
        bad = np.nonzero(a != ref)[0]
        assert len(bad) == 0, (counter, bad[:8], u[bad[:8]], a[bad[:8]], ref[bad[:8]])
    u = pr.head_uniforms(0, 0, n)
    assert u[0] == 0.0
    masked = _known_logits_net(gpu_device, A, [float("-inf")] + [0.0] * (A - 1))
    out = _head(_pack_head(masked, A), feat, h, c, A, seed=0, counter=0)
    a = out["action"].cpu().numpy()
    assert np.array_equal(a, pr.sample_ref(np.array([-np.inf] + [0.0] * (A - 1)), u))
    assert a.min() >= 1 and a[0] == 1


def test_head_argument_checks(gpu_device):
    """num_actions outside 1 .. 7 and a NULL required pointer return HEIST_EINVAL from the pack
    and the head and write nothing; n = 0 is a no-op."""
    dev = gpu_device
    L, P = nat.lib(), nat.ptr
    torch.manual_seed(2)
    net = _big_heads(SolverNetwork(num_actions=7).to(dev))
    ws = _head_params(net)
    nbytes = L.heist_solver_head_packed_bytes()
    packed = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    for A in (0, 8, -1):
        assert L.heist_solver_head_pack(*(P(t) for t in ws), A, P(packed), nat.stream(dev)) == EINVAL, A
    for missing in (0, 5, 10, 13):
        args = [None if i == missing else P(t) for i, t in enumerate(ws)]
        assert L.heist_solver_head_pack(*args, 7, P(packed), nat.stream(dev)) == EINVAL, missing
    assert L.heist_solver_head_pack(*(P(t) for t in ws), 7, None, nat.stream(dev)) == EINVAL
    torch.cuda.synchronize(dev)
    assert bool((packed == 0xA5).all())

    good = _pack_head(net, 7)
    n = 8
    feat, h, c = _head_inputs(dev, n, seed=1)

    def call(A=7, n=n, feat=feat, packed=good, drop=None):
        out = _head_outputs(dev, n, 8)
        ptrs = {k: (None if k == drop else P(t)) for k, t in out.items()}
        rc = L.heist_solver_head(P(feat), P(h), P(c), n, P(packed), A, 1, 2, ptrs["logits"], ptrs["value"],
                                 ptrs["action"], ptrs["logp"], ptrs["h"], ptrs["c"], nat.stream(dev))
        torch.cuda.synchronize(dev)
        return rc, out

    for kw in (dict(A=0), dict(A=8), dict(A=-1), dict(n=-1), dict(feat=None), dict(packed=None), dict(drop="value"),
               dict(drop="action"), dict(drop="logp"), dict(drop="h"), dict(drop="c")):
        rc, out = call(**kw)
        assert rc == EINVAL, (kw, rc)
        assert all(_is_sentinel(t) for t in out.values()), kw
    rc, out = call(n=0)
    assert rc == 0 and all(_is_sentinel(t) for t in out.values())
    rc, out = call()  # the same call with nothing wrong runs
    assert rc == 0 and not _is_sentinel(out["value"][:n]) and _is_sentinel(out["value"][n:])
