"""The references of tests/policy_ref.py, checked without a GPU: the exact integer case meets
the conditions under which tests/test_gpu_policy_exact.py may demand bit equality, and the
head's draw is pinned to values worked out with plain Python integers."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import policy_ref as pr


@pytest.mark.parametrize("R", [10, 20, 32])
def test_integer_case_conditions(R):
    case = pr.integer_case(R, 8)
    c = case.cond
    print("integer_case R=%d n=8: bound=%s pool_bound=%g fire=%s rounded=%s ties=%s"
          % (R, c.bound, c.pool_bound, ["%.3f" % v for v in c.fire], ["%.4f" % v for v in c.rounded], c.ties))
    assert case.obs.shape == (8, 3, R, R) and case.sums.shape == (8, 1024) and case.area.shape == (1024,)
    for t in (case.obs,) + case.params:
        assert t.dtype == torch.float32 and torch.equal(t, t.round())
    assert case.obs.abs().max() <= 2 and all(w.abs().max() <= 2 for w in case.params[0::2])
    assert all(b.abs().max() <= 3 for b in case.params[1::2])
    # every product and partial sum is an integer below 2^24: exact in fp32 in any order
    assert all(b < 2 ** 24 for b in c.bound) and c.pool_bound < 2 ** 24
    # both branches of every ReLU are taken
    assert all(0.25 <= f <= 0.75 for f in c.fire), c.fire
    # the bf16 rounding of the activations matters, exact ties included (257 -> 256 is
    # round-to-nearest-even; truncation and round-half-up give other sums)
    assert c.rounded[1] >= 0.01 and c.rounded[2] >= 0.10, c.rounded
    assert c.ties[1] + c.ties[2] >= 1
    assert torch.equal(case.sums, case.sums.round()) and case.sums.min() >= 0
    assert sorted(set(case.area.tolist())) == [{10: 9.0, 20: 25.0, 32: 64.0}[R]]


@pytest.mark.parametrize("R", [10, 20, 32])
def test_integer_case_fp32_torch_is_bit_equal(R):
    """torch's fp32 CPU convolutions (another summation order) reproduce the float64
    reference bit for bit: the case is exact in fp32, not merely close."""
    case = pr.integer_case(R, 8)
    w1, b1, w2, b2, w3, b3 = case.params
    x = case.obs
    for w, b in ((w1, b1), (w2, b2), (w3, b3)):
        x = pr._bf(F.relu(F.conv2d(x, w, b, padding=1)))
    assert x.dtype == torch.float32
    win = pr.pool_windows(R)
    sums = torch.stack([x[:, :, r0:r1, c0:c1].sum((2, 3)) for r0, r1 in win for c0, c1 in win], dim=2)
    assert torch.equal(sums.reshape(8, 1024).double(), case.sums)
    # and torch's own adaptive pool has the same windows
    pooled = F.adaptive_avg_pool2d(x.double(), (4, 4)).reshape(8, 1024)
    assert torch.allclose(pooled, case.sums / case.area, rtol=1e-15, atol=0)


def test_pool_windows_and_quotient():
    assert pr.pool_windows(10) == [(0, 3), (2, 5), (5, 8), (7, 10)]
    assert pr.pool_windows(20) == [(0, 5), (5, 10), (10, 15), (15, 20)]
    assert pr.pool_windows(32) == [(0, 8), (8, 16), (16, 24), (24, 32)]
    from fractions import Fraction
    rng = np.random.default_rng(0)
    s = rng.integers(0, 2 ** 20, 2000).astype(np.float64)
    for a in (9.0, 25.0, 64.0, 6.0):
        q = pr.quotient_f32(s, np.full_like(s, a))
        assert q.dtype == np.float32
        for si, qi in zip(s[:300], q[:300]):
            exact = Fraction(int(si), int(a))
            for other in (np.nextafter(qi, np.float32(-np.inf)), np.nextafter(qi, np.float32(np.inf))):
                assert abs(Fraction(float(qi)) - exact) <= abs(Fraction(float(other)) - exact)


def test_bf16_round_is_nearest_even():
    x = torch.tensor([257.0, 259.0, 258.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)
    assert pr._bf(x).tolist() == [256.0, 260.0, 258.0, 1.0, 1.0 + 2.0 ** -6]
    assert pr._bf16_tie(x, pr._bf(x)).tolist() == [True, True, False, True, True]


# (seed, counter, env) -> the top 24 bits of the hash, worked out with Python integers
HASH_LITERALS = [
    ((0, 0, 0), 0),
    ((0, 0, 1), 14819496),
    ((0, 1, 0), 8522164),
    ((1, 0, 0), 5673494),
    ((77, 3, 4095), 11862359),
    ((2 ** 63 + 12345, 2 ** 32 + 5, 257), 10900410),
    ((0, 210, 1686), 1 << 23),  # u = 0.5 exactly (test_head_sample_exact_boundaries)
]


def test_head_uniform_literals():
    for args, top in HASH_LITERALS:
        assert pr.head_uniform(*args) == top * 2.0 ** -24, args
    assert pr.mix64(1) == 0x5692161D100B05E5  # splitmix64's finaliser itself


def test_head_uniform_vector_form_and_range():
    for seed, counter in ((0, 0), (77, 3), (2 ** 63 + 12345, 2 ** 32 + 5), (2 ** 64 - 1, 2 ** 64 - 1)):
        u = pr.head_uniforms(seed, counter, 300)
        assert u.dtype == np.float64 and (u >= 0).all() and (u < 1).all()
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u)  # 24 bits: exact in fp32
        assert u.tolist() == [pr.head_uniform(seed, counter, e) for e in range(300)]


def test_head_uniform_is_uniform_and_per_env():
    u = np.stack([pr.head_uniforms(77, k, 4096) for k in range(4)])
    counts = np.bincount((u * 16).astype(np.int64).ravel(), minlength=16)
    expect = u.size / 16
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    assert chi2 < 44.3, (chi2, counts)  # p ~ 1e-4 at 15 dof
    assert (u[:, 1:] != u[:, :-1]).all()  # adjacent envs
    assert (u[1:] != u[:-1]).all()        # adjacent counters
    assert len(np.unique(u)) > 0.999 * u.size


def test_sample_ref_rule():
    logits = np.log(np.array([0.25, 0.5, 0.25]))
    u = np.array([0.0, 0.2499, 0.25, 0.7499, 0.75, 0.9999])
    assert pr.sample_ref(logits, u).tolist() == [0, 0, 1, 1, 2, 2]
    assert pr.near_boundary(logits, u, 1e-3).tolist() == [False, True, True, True, True, False]
    # a zero-probability action is never drawn, u = 0 included
    assert pr.sample_ref(np.array([-np.inf, 0.0]), np.array([0.0, 0.5])).tolist() == [1, 1]
    # per-env logits
    lg = np.log(np.array([[0.5, 0.5], [0.1, 0.9]]))
    assert pr.sample_ref(lg, np.array([0.3, 0.3])).tolist() == [0, 1]


def test_logp_ref_matches_torch_categorical():
    torch.manual_seed(0)
    lg = torch.randn(64, 5) * 3
    a = torch.randint(0, 5, (64,))
    ref = torch.distributions.Categorical(F.softmax(lg, -1)).log_prob(a)
    assert (pr.logp_ref(lg.double(), a).float() - ref).abs().max().item() < 1e-6
    # one action: probability 1 clamps to 1 - eps; torch's fp32 value is the rounded float64 one
    one = torch.distributions.Categorical(probs=torch.ones(3, 1)).log_prob(torch.zeros(3, dtype=torch.int64))
    assert one.dtype == torch.float32
    assert one.tolist() == [float(np.float32(np.log(1.0 - pr.EPS32)))] * 3
