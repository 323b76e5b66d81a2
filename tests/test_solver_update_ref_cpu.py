"""tests/solver_update_ref.py (the float64 restatement of the reference Solver's PPO update)
against tests/golden/solver_update_<case>.npz (what the reference itself computed in float32 on
the same buffers): the two agree within twice the reference's own float32-vs-float64 error, which
the generator recorded per tensor in the fixture.  No GPU and no native library involved: this
ties fixture and restatement together before tests/test_gpu_solver_update_golden.py uses both."""
import numpy as np
import pytest
import torch

import solver_update_ref as sr

# a floor of exactly 0 (a bias whose fp32 gradient happened to round like float64's) still
# allows float64's own rounding
TINY = 1e-9


@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.slow) if n == "big20" else n for n in sr.CASES])
def test_restatement_reproduces_fixture(name):
    c = sr.load_case(name)
    assert c["states"].shape == (c["T"], 3, c["R"], c["C"]) and c["perms"].shape == (c["epochs"], c["T"])
    for e in range(c["epochs"]):
        assert np.array_equal(np.sort(c["perms"][e]), np.arange(c["T"]))
    p0 = sr.golden_params(c["head_scale"])
    out = sr.run_update(p0, c["states"], c["actions"], c["logp"], c["values"], c["rewards"],
                        c["dones"].astype(np.float32), c["perms"], c["epochs"], c["batch"], record=c["rec_steps"])
    assert out["n_steps"] == c["n_steps"]
    assert np.abs(out["adv"].numpy() - c["adv"]).max() <= 1e-5
    assert np.abs(out["ret"].numpy() - c["ret"]).max() <= 1e-5
    assert np.abs(out["metrics"] - c["metrics"]).max() <= 2 * c["floor_metrics"].max() + 1e-7
    for j, s in enumerate(c["rec_steps"]):
        st = out["steps"][s]
        key = "s%d_" % s
        assert np.abs(st["parts"] - c[key + "parts"]).max() <= 1e-5
        assert abs(st["total_norm"] - float(c[key + "total"])) <= (2 * c["floor_total"][j] + TINY) * float(c[key + "total"])
        got = [st["grads"][k].numpy() for k in sr.PARAMS]
        bound = np.where(np.arange(len(sr.PARAMS)) < sr.N_CONV, c["floor_grad_max"][j], c["floor_grad_l2"][j])
        seen, bad = sr.check_tensors(got, c[key + "gconv"], c[key + "gnorm"], c[key + "gproj"], 2 * bound + TINY,
                                     "%s step %d gradient" % (name, s))
        assert not bad, bad
    delta = [(out["params"][k] - p0[k].double()).numpy() for k in sr.PARAMS]
    # (projections within 4 x bound x norm here too: the floor IS this comparison's relative L2 error
    # e, and a Gaussian projection of an error vector of that size has standard deviation e x norm.)
    # Scaled head layers: float64 against the stored float32 change, half a spacing per step.
    seen, bad = sr.check_tensors(delta, c["d_conv"], c["d_norm"], c["d_proj"], 2 * c["floor_delta"] + TINY,
                                 "%s parameter change" % name, conv_metric=sr.rel_l2,
                                 full=sr.coarse_delta(c, p0, 0.5 * c["n_steps"]))
    assert ("d_heads" in c) == (c["head_scale"] != 1.0)
    assert not bad, bad
    print("%s: parameter-change measures %s" % (name, {k: "%.2g" % v for k, v in seen.items()}))


def test_state_coding_round_trip():
    """encode_states / decode_states on observation-like planes, bit for bit."""
    rng = np.random.default_rng(3)
    R = C = 12
    T = 9
    s = np.zeros((T, 3, R, C), np.float32)
    s[:, 0] = (rng.integers(0, 6, (1, R, C)) / np.float32(5)).astype(np.float32)
    s[5:, 0] = (rng.integers(0, 6, (1, R, C)) / np.float32(5)).astype(np.float32)
    s[:, 1] = rng.random((T, R, C)) < 0.3
    pos = rng.integers(0, R * C - C - 2, T)
    p = np.zeros((T, R * C), np.float32)
    p[np.arange(T), pos] = 1.0
    p[:, (R - 2) * C + C - 2] = -1.0
    s[:, 2] = p.reshape(T, R, C) + sr.pos_gradient(R, C)
    occ, lay, vis, q = sr.encode_states(s, R, C)
    assert len(occ) == 2 and np.array_equal(q, pos)
    assert np.array_equal(sr.decode_states(occ, lay, vis, q, R, C).view(np.uint32), s.view(np.uint32))


def test_forced_masks_change_only_the_relu_decisions():
    """run_update with a step's own masks forced reproduces the unforced run exactly."""
    c = sr.load_case("g10")
    p0 = sr.golden_params()
    args = (p0, c["states"], c["actions"], c["logp"], c["values"], c["rewards"], c["dones"].astype(np.float32),
            c["perms"], 1, c["batch"])
    a = sr.run_update(*args, record=[0], keep_signs=True)
    b = sr.run_update(*args, record=[0], masks={0: a["signs"][0]})
    for k in sr.PARAMS:
        assert torch.equal(a["steps"][0]["grads"][k], b["steps"][0]["grads"][k]), k
    flipped = [m.clone() for m in a["signs"][0]]
    flipped[2][0, 0] = ~flipped[2][0, 0]
    d = sr.run_update(*args, record=[0], masks={0: flipped})
    assert not torch.equal(a["steps"][0]["grads"]["conv3.weight"], d["steps"][0]["grads"]["conv3.weight"])
