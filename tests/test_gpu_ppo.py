"""GPU parity of the GAE scan, advantage normalisation and fused clipped-PPO loss.

Floating point: within 1e-4 of the reference (north star), checked against the
reference's golden vectors, the C oracle and a plain PyTorch fp32 autograd
restatement of agents/solver.py:172-193.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_data as gd
from oracle import pyoracle as po
from heist_amd.ppo import compute_gae, normalize_advantages, ppo_loss

pytestmark = pytest.mark.gpu
TOL = 1e-4


def test_gae_golden(gpu_device):
    z = gd.load("ppo.npz")
    for i in range(int(z["n_gae"])):
        r, v, d = (torch.tensor(z["gae%d_%s" % (i, k)], device=gpu_device) for k in "rvd")
        adv, ret = compute_gae(r, v, d)
        np.testing.assert_allclose(adv.cpu().numpy(), z["gae%d_adv" % i], atol=TOL, rtol=0)
        np.testing.assert_allclose(ret.cpu().numpy(), z["gae%d_ret" % i], atol=TOL, rtol=0)
        norm = normalize_advantages(adv)
        np.testing.assert_allclose(norm.cpu().numpy(), z["gae%d_norm" % i], atol=TOL, rtol=0)


def test_gae_columns_vs_oracle(gpu_device):
    rng = np.random.default_rng(0)
    T, N = 203, 4096
    r = rng.normal(size=(T, N)).astype(np.float32)
    v = rng.normal(size=(T, N)).astype(np.float32)
    d = (rng.random((T, N)) < 0.03).astype(np.uint8)
    adv, ret = compute_gae(*(torch.from_numpy(x).to(gpu_device) for x in (r, v, d)))
    adv = adv.cpu().numpy()
    for n in rng.choice(N, 64, replace=False):
        exp = po.gae(r[:, n], v[:, n], d[:, n].astype(np.float32))
        np.testing.assert_array_equal(adv[:, n], exp)  # same float32 op order: bit-exact
    np.testing.assert_array_equal(ret.cpu().numpy(), adv + v)


def test_gae_bootstrap(gpu_device):
    r = torch.zeros(3, 1, device=gpu_device)
    v = torch.zeros(3, 1, device=gpu_device)
    d = torch.zeros(3, 1, dtype=torch.uint8, device=gpu_device)
    lv = torch.ones(1, device=gpu_device)
    adv, _ = compute_gae(r, v, d, last_value=lv)
    g, lam = 0.99, 0.95
    assert abs(float(adv[2, 0]) - g) < 1e-6
    assert abs(float(adv[0, 0]) - g * (g * lam) ** 2) < 1e-6


def test_normalize_large(gpu_device):
    x = torch.randn(1 << 22, device=gpu_device) * 3 + 5
    y = normalize_advantages(x)
    ref = (x - x.mean()) / (x.std() + 1e-8)
    assert float((y - ref).abs().max()) < 1e-4


def _torch_reference_loss(logits, values, actions, old, adv, ret, clip=0.2, vc=0.5, ec=0.05):
    """agents/solver.py:175-193 in plain PyTorch fp32."""
    probs = F.softmax(logits, dim=-1)
    dist = torch.distributions.Categorical(probs)
    nl = dist.log_prob(actions)
    ent = dist.entropy().mean()
    ratio = torch.exp(nl - old)
    pl = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
    vl = F.mse_loss(values.squeeze(), ret)
    return pl + vc * vl - ec * ent, pl, vl, ent


def test_ppo_loss_golden(gpu_device):
    z = gd.load("ppo.npz")
    for i in range(int(z["n_loss"])):
        g = lambda k: torch.tensor(z["loss%d_%s" % (i, k)], device=gpu_device)  # noqa: E731
        logits = g("logits").requires_grad_(True)
        values = g("values").requires_grad_(True)
        loss, parts = ppo_loss(logits, values, g("actions"), g("old"), g("adv"), g("ret"))
        loss.backward()
        p = parts.cpu().numpy()
        assert abs(p[1] - float(z["loss%d_pg" % i])) < TOL
        assert abs(p[2] - float(z["loss%d_vl" % i])) < TOL
        assert abs(p[3] - float(z["loss%d_ent" % i])) < TOL
        np.testing.assert_allclose(logits.grad.cpu().numpy(), z["loss%d_dlogits" % i], atol=1e-6, rtol=TOL)
        np.testing.assert_allclose(values.grad.cpu().numpy(), z["loss%d_dvalues" % i], atol=1e-6, rtol=TOL)


@pytest.mark.parametrize("M", [1, 64, 1000, 65536])
def test_ppo_loss_vs_torch_autograd(M, gpu_device):
    gen = torch.Generator(device="cpu").manual_seed(M)
    logits = (torch.randn(M, 5, generator=gen) * 2).to(gpu_device)
    logits[0, 0] = 40.0  # clamp branch
    values = torch.randn(M, 1, generator=gen).to(gpu_device)
    actions = torch.randint(0, 5, (M,), generator=gen).to(gpu_device)
    with torch.no_grad():
        old = torch.distributions.Categorical(F.softmax(logits, -1)).log_prob(actions) + \
            torch.randn(M, generator=gen).to(gpu_device) * 0.3
    adv = torch.randn(M, generator=gen).to(gpu_device)
    ret = torch.randn(M, generator=gen).to(gpu_device)
    l1, v1 = logits.clone().requires_grad_(True), values.clone().requires_grad_(True)
    loss, parts = ppo_loss(l1, v1, actions, old, adv, ret)
    loss.backward()
    l2, v2 = logits.clone().requires_grad_(True), values.clone().requires_grad_(True)
    ref, pl, vl, ent = _torch_reference_loss(l2, v2, actions, old, adv, ret)
    ref.backward()
    assert abs(float(loss) - float(ref)) < TOL
    assert abs(float(parts[3]) - float(ent)) < TOL
    torch.testing.assert_close(l1.grad, l2.grad, atol=1e-6, rtol=1e-3)
    torch.testing.assert_close(v1.grad, v2.grad, atol=1e-6, rtol=1e-4)


def test_ppo_loss_vs_oracle(gpu_device):
    rng = np.random.default_rng(9)
    M = 4096
    logits = rng.normal(0, 2, (M, 5)).astype(np.float32)
    values = rng.normal(size=M).astype(np.float32)
    actions = rng.integers(0, 5, M)
    old = rng.normal(-1.6, 0.5, M).astype(np.float32)
    adv = rng.normal(size=M).astype(np.float32)
    ret = rng.normal(size=M).astype(np.float32)
    parts_o, dl_o, dv_o = po.ppo_loss(logits, values, actions, old, adv, ret)
    t = lambda a: torch.from_numpy(a).to(gpu_device)  # noqa: E731
    lg = t(logits).requires_grad_(True)
    vv = t(values).requires_grad_(True)
    loss, parts = ppo_loss(lg, vv, t(actions), t(old), t(adv), t(ret))
    loss.backward()
    np.testing.assert_allclose(parts.cpu().numpy(), parts_o, atol=TOL, rtol=0)
    np.testing.assert_allclose(lg.grad.cpu().numpy(), dl_o, atol=1e-7, rtol=1e-4)
    np.testing.assert_allclose(vv.grad.cpu().numpy(), dv_o, atol=1e-7, rtol=1e-5)


# ---------------------------------------------------------------------------------------------
# Edges: the GAE scan's 4-step body and tail, the normalisation's count <= 1 rule and block
# clamp, and the loss over every action count with its clamp branches, each against a plain
# reference written here (not the C oracle's twin of the kernel, not the kernel).

GAMMA, LAM = 0.99, 0.95


def _gae_ref32(r, v, d, lv):
    """agents/solver.py:228-244 per column in float32, the reference's op order:
    delta = (r + (g * nv) * nd) - v;  A = delta + (gl * nd) * A."""
    g, gl = np.float32(GAMMA), np.float32(GAMMA * LAM)
    T, N = r.shape
    nv = np.zeros(N, np.float32) if lv is None else lv.astype(np.float32)
    A = np.zeros(N, np.float32)
    adv = np.empty((T, N), np.float32)
    for t in range(T - 1, -1, -1):
        nd = np.float32(1.0) - d[t].astype(np.float32)
        delta = (r[t] + (g * nv) * nd) - v[t]
        A = delta + (gl * nd) * A
        adv[t] = A
        nv = v[t]
    assert adv.dtype == np.float32
    return adv


def _dones(pattern, T, N, rng):
    d = np.zeros((T, N), np.uint8)
    if pattern == "all":
        d[:] = 1
    elif pattern == "last":
        d[T - 1] = 1
    elif pattern == "random":
        d = (rng.random((T, N)) < 0.3).astype(np.uint8)
    return d


@pytest.mark.parametrize("bootstrap", [False, True], ids=["no_last_value", "last_value"])
@pytest.mark.parametrize("pattern", ["none", "all", "last", "random"])
@pytest.mark.parametrize("N", [1, 255, 257])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 7, 8, 9])
def test_gae_edges_bit_exact(gpu_device, T, N, pattern, bootstrap):
    """Every split of T into the 4-step unrolled body and its tail, one and two blocks of
    columns: adv bit-equal to the float32 loop above, ret bit-equal to adv + v, and a done at
    T - 1 cuts off last_value."""
    rng = np.random.default_rng(1000 * T + N)
    r = rng.normal(size=(T, N)).astype(np.float32)
    v = rng.normal(size=(T, N)).astype(np.float32)
    d = _dones(pattern, T, N, rng)
    lv = rng.normal(size=N).astype(np.float32) * 3 if bootstrap else None
    t = lambda a: None if a is None else torch.from_numpy(a).to(gpu_device)  # noqa: E731
    adv, ret = compute_gae(t(r), t(v), t(d), last_value=t(lv), gamma=GAMMA, lam=LAM)
    adv, ret = adv.cpu().numpy(), ret.cpu().numpy()
    want = _gae_ref32(r, v, d, lv)
    assert adv.shape == (T, N) and adv.dtype == np.float32
    np.testing.assert_array_equal(adv.view(np.int32), want.view(np.int32))
    np.testing.assert_array_equal(ret.view(np.int32), (want + v).view(np.int32))
    if bootstrap:
        cut = d[T - 1] != 0
        np.testing.assert_array_equal(adv[:, cut], _gae_ref32(r, v, d, None)[:, cut])
        if pattern == "none":  # and without a done it is felt in the last step of every column
            assert (adv[T - 1] != _gae_ref32(r, v, d, None)[T - 1]).all()


def test_normalize_single_element_unchanged(gpu_device):
    """len(advantages) == 1 is returned as it is (agents/solver.py:146-147), bit for bit."""
    for val in (3.25, -0.0, 1e-30):
        x = torch.tensor([val], device=gpu_device)
        for inplace in (False, True):
            y = normalize_advantages(x.clone(), inplace=inplace)
            assert torch.equal(y.view(torch.int32), x.view(torch.int32))


@pytest.mark.parametrize("mean,std", [(5.0, 3.0), (100.0, 0.5)])
@pytest.mark.parametrize("n", [2, 255, 257, 2048 * 256 + 3])
def test_normalize_edges_vs_float64(gpu_device, n, mean, std):
    """(x - mean) / (std_unbiased + eps) against float64 within TOL; the largest n is past the
    2,048-block clamp of the reductions (grid-stride loop).  At these moments one float32 ulp of
    the mean or the std moves the result by under 2e-5.  inplace=True writes the same values."""
    rng = np.random.default_rng(n)
    x = rng.normal(mean, std, n).astype(np.float32)
    x64 = x.astype(np.float64)
    want = (x64 - x64.mean()) / (x64.std(ddof=1) + 1e-8)
    xd = torch.from_numpy(x).to(gpu_device)
    y = normalize_advantages(xd)
    assert torch.equal(xd.cpu(), torch.from_numpy(x)), "the copy must leave its input alone"
    err = float(np.abs(y.cpu().numpy().astype(np.float64) - want).max())
    print("n=%d N(%g, %g): max |diff| vs float64 %.3g" % (n, mean, std, err))
    assert err < TOL
    z = xd.clone()
    out = normalize_advantages(z, inplace=True)
    assert out.data_ptr() == z.data_ptr()
    assert torch.equal(z.view(torch.int32), y.view(torch.int32))


def test_normalize_constant_input_gives_exact_zeros(gpu_device):
    x = torch.full((1000,), 3.7, device=gpu_device)
    y = normalize_advantages(x)
    assert not bool(torch.isnan(y).any())
    assert torch.equal(y, torch.zeros_like(y))


F32_EPS = 1.1920929e-07  # torch.finfo(torch.float32).eps, the clamp of Categorical(probs) in float32
_OFFSETS = (0.0, 0.1, -0.1, 0.5, -0.5, 1.5, -1.5)


def _clamped_probs64(logits):
    """float64 softmax, renormalised as Categorical(probs) does, and its log-probabilities with
    the clamp written out at float32's eps."""
    probs = F.softmax(logits, dim=-1)
    pn = probs / probs.sum(-1, keepdim=True)
    return pn, torch.log(pn.clamp(F32_EPS, 1 - F32_EPS))


def _loss_ref64(logits, values, actions, old, adv, ret, clip=0.2, vc=0.5, ec=0.05):
    """agents/solver.py:172-193 in float64 on the float32 inputs, differentiated by autograd."""
    lg = logits.double().clone().requires_grad_(True)
    vv = values.double().clone().requires_grad_(True)
    old, adv, ret = old.double(), adv.double(), ret.double()
    pn, lc = _clamped_probs64(lg)
    nl = lc.gather(1, actions[:, None]).squeeze(1)  # dist.log_prob
    ent = -(lc * pn).sum(-1).mean()  # dist.entropy().mean()
    ratio = torch.exp(nl - old)
    pl = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
    vl = F.mse_loss(vv.reshape(-1), ret)
    loss = pl + vc * vl - ec * ent
    loss.backward()
    return [float(x.detach()) for x in (loss, pl, vl, ent)], lg.grad, vv.grad


def _loss_inputs(M, A, seed):
    """Rows cycle through: ordinary N(0, 2) logits; the chosen action 30 below the rest (its
    probability clamps to eps); 30 above the rest (it clamps to 1 - eps, the others to eps);
    ordinary.  old_logp = the row's clamped float64 log-probability + an offset cycling through
    _OFFSETS (ratios inside the clip range and outside it on both sides); adv standard normal
    with every fifth row exactly 0 (both signs meet both clip sides; s1 == s2 ties)."""
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn(M, A, generator=gen) * 2
    actions = torch.randint(0, A, (M,), generator=gen)
    rows = torch.arange(M)
    if A > 1:
        rest = logits.clone()
        rest[rows, actions] = float("nan")
        lo = torch.where(torch.isnan(rest), torch.full_like(rest, float("inf")), rest).min(1).values
        hi = torch.where(torch.isnan(rest), torch.full_like(rest, -float("inf")), rest).max(1).values
        chosen = logits[rows, actions]
        chosen = torch.where(rows % 4 == 1, lo - 30, chosen)
        chosen = torch.where(rows % 4 == 2, hi + 30, chosen)
        logits[rows, actions] = chosen
    _, lc = _clamped_probs64(logits.double())
    off = torch.tensor(_OFFSETS, dtype=torch.float64)[rows % len(_OFFSETS)]
    old = (lc[rows, actions] + off).float()
    adv = torch.randn(M, generator=gen)
    adv[rows % 5 == 0] = 0.0
    values = torch.randn(M, 1, generator=gen)
    ret = torch.randn(M, generator=gen)
    return logits, values, actions, old, adv, ret


@pytest.mark.parametrize("M", [1, 255, 257, 513])
@pytest.mark.parametrize("A", [1, 2, 5, 7, 16])
def test_ppo_loss_edges_vs_float64_autograd(gpu_device, A, M):
    """Every action count class (1, 2, odd, the kernel's maximum 16) and one to three blocks of
    rows, with the clamp branches in every fourth row, against a float64 autograd restatement
    (no hand-derived backward): loss parts within TOL, dlogits and dvalues within 1e-5 of their
    tensor's max |reference|, and per element against torch's own fp32 autograd at
    test_ppo_loss_vs_torch_autograd's tolerances.

    The 1e-5: torch's own fp32 autograd of the same loss differs from this float64 reference by
    at most 2.4e-7 of the tensor's max over all 20 (A, M) pairs on exactly these inputs (measured
    on the CPU, reference against reference), so 1e-5 leaves a margin of about 40x over fp32
    rounding, while a wrong term of the size that atol = 1e-6 lets through (up to 1e-4 of these
    gradients' max) fails it."""
    logits, values, actions, old, adv, ret = _loss_inputs(M, A, seed=100 * A + M)
    pn, _ = _clamped_probs64(logits.double())
    # no probability within a factor of 4 of either clamp bound: fp32 and float64 decide alike
    assert not bool(((pn > F32_EPS / 4) & (pn < F32_EPS * 4)).any())
    assert not bool(((1 - pn > F32_EPS / 4) & (1 - pn < F32_EPS * 4)).any())
    if A > 1 and M >= 255:
        chosen = pn[torch.arange(M), actions]
        assert bool((chosen < F32_EPS).any()) and bool((chosen > 1 - F32_EPS).any())
    parts64, dl64, dv64 = _loss_ref64(logits, values, actions, old, adv, ret)
    dev = lambda t: t.to(gpu_device)  # noqa: E731
    l1, v1 = dev(logits).requires_grad_(True), dev(values).requires_grad_(True)
    loss, parts = ppo_loss(l1, v1, dev(actions), dev(old), dev(adv), dev(ret))
    loss.backward()
    p = parts.cpu().numpy().astype(np.float64)
    print("A=%d M=%d parts %s vs float64 %s" % (A, M, p, parts64))
    assert float(loss) == float(parts[0])
    for got, want in zip(p, parts64):
        assert abs(got - want) < TOL
    for name, got, want in (("dlogits", l1.grad, dl64), ("dvalues", v1.grad, dv64)):
        assert got.shape == want.shape
        scale = float(want.abs().max())
        err = float((got.cpu().double() - want).abs().max())
        print("A=%d M=%d %s: max |diff| %.3g, max |reference| %.3g" % (A, M, name, err, scale))
        assert err <= 1e-5 * scale, (name, err, scale)
    l2, v2 = dev(logits).requires_grad_(True), dev(values).requires_grad_(True)
    ref, pl, vl, ent = _torch_reference_loss(l2, v2.reshape(-1), dev(actions), dev(old), dev(adv), dev(ret))
    ref.backward()
    assert abs(float(loss) - float(ref)) < TOL
    assert abs(float(parts[3]) - float(ent)) < TOL
    torch.testing.assert_close(l1.grad, l2.grad, atol=1e-6, rtol=1e-3)
    torch.testing.assert_close(v1.grad, v2.grad, atol=1e-6, rtol=1e-4)


@pytest.mark.parametrize("M,A", [(8, 17), (8, 0), (0, 5)], ids=["A17", "A0", "M0"])
def test_ppo_loss_argument_checks(gpu_device, M, A):
    """A outside 1 .. 16 and M = 0 return HEIST_EINVAL and write nothing."""
    from heist_amd import _native as nat
    f = lambda *s: torch.full(s, 7.0, device=gpu_device)  # noqa: E731
    logits, values, old, adv, ret = f(8, 17), f(8), f(8), f(8), f(8)
    actions = torch.zeros(8, dtype=torch.int64, device=gpu_device)
    parts, dl, dv = f(4), f(8, 17), f(8)
    scratch = torch.full((3,), 7.0, dtype=torch.float64, device=gpu_device)
    P = nat.ptr
    rc = nat.lib().heist_ppo_loss(P(logits), P(values), P(actions), P(old), P(adv), P(ret), M, A, 0.2, 0.5, 0.05,
                                  P(parts), P(dl), P(dv), P(scratch), nat.stream(gpu_device))
    assert rc == 100000  # HEIST_EINVAL
    torch.cuda.synchronize(gpu_device)
    for t in (parts, dl, dv, scratch):
        assert bool((t == 7.0).all())
