"""heist_plan_masked without a GPU: the reference's own pinned answers (masked_ref: the C oracle on
layouts with the switched-off emitters removed), the pure-torch mask builder and the derived
fields of PlanAblation on hand-made tensors, and the library's symbols."""
import ctypes

import numpy as np
import pytest
import torch

import masked_ref as mr
import plan_ref as pr
from heist_amd import _build, _native
from heist_amd.search import PlanAblation, ablation_masks


# ---- the fixture table, from the oracle search alone

@pytest.mark.parametrize("name", sorted(mr.FIXTURES))
def test_fixture_ticks(name):
    for on, T in mr.TICKS[name].items():
        got = mr.search(name, on)[0]
        print("%s %r: %d" % (name, on, got))
        assert got == T, (name, on)


def test_fixtures_fit_the_budget():
    """Every emitter of every fixture is bought: at a budget that drops one, the table above would
    describe another layout."""
    for name, layout in mr.FIXTURES.items():
        o = pr.po.OracleEnv(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, mr.BUDGET)
        assert o.set_layout(*layout), name
        i = o.info()
        assert (i["n_cams"], i["n_guards"]) == (len(layout[1]), len(layout[2])), name
    walls, cams, guards = mr.FIXTURES["three_same"]
    o = pr.po.OracleEnv(pr.GRID, pr.GRID, pr.MAX_STEPS, pr.START, pr.VAULT, pr.BUDGET)
    o.set_layout(walls, cams, guards)
    assert o.info()["n_cams"] == 2  # plan_ref's 15 drops the third camera without a word


def test_reference_tables_agree_with_the_search():
    """The recurrence on the witness planes gives the search's ticks at the start cell (reference()
    asserts it), a wider set of live emitters never helps, and the all-off variants are one layout."""
    for name in ("cam_guard", "three_same"):
        full = mr.reference(name, mr.variants(name)[0], 1.0)
        for on in mr.variants(name)[1:]:
            r = mr.reference(name, on, 1.0)
            assert r["value"][pr.START] >= full["value"][pr.START]
            assert 0 < r["ticks"] <= full["ticks"]
    a = mr.reference("cam_guard", ((0,), (0,)), 0.99)
    b = mr.reference("three_same", ((0, 0, 0), ()), 0.99)
    np.testing.assert_array_equal(a["value"].view(np.int64), b["value"].view(np.int64))
    np.testing.assert_array_equal(a["togo"], b["togo"])


def test_mask_word():
    assert mr.mask_word(((1, 0, 1), (1,)), 5) == 0b100101
    assert mr.mask_word(((1,), (1,)), 33) == 1 | 1 << 33
    assert mr.mask_word(((1,), ()), 5, garbage=1 << 63) == -(1 << 63) + 1


# ---- ablation_masks

def test_ablation_masks_filled_and_unfilled():
    m = ablation_masks(torch.tensor([2, 0, 3]), torch.tensor([1, 2, 0]), 3, 2)
    assert m.dtype == torch.int64 and m.shape == (3, 6)
    full = [0b01011, 0b11000, 0b00111]
    assert m[:, 0].tolist() == full
    filled = mr.filled_flags([2, 0, 3], [1, 2, 0], 3, 2)
    for e in range(3):
        for j in range(5):
            want = full[e] & ~(1 << j) if filled[e, j] else full[e]  # an unfilled slot: variant 0 again
            assert int(m[e, 1 + j]) == want, (e, j)
    # int32 counts (HeistEnv.export's) and NumPy counts give the same masks
    assert torch.equal(m, ablation_masks(torch.tensor([2, 0, 3], dtype=torch.int32), np.array([1, 2, 0]), 3, 2))


def test_ablation_masks_high_bits():
    """Slots from 32 up, the sign bit included: 33 cameras + 31 guards fill all 64 bits."""
    m = ablation_masks(torch.tensor([33, 1]), torch.tensor([31, 1]), 33, 31)
    assert m.shape == (2, 65)
    assert int(m[0, 0]) == -1                                  # all 64 bits
    assert int(m[0, 1 + 33]) == -1 - (1 << 33)                 # the first guard's bit is 33
    assert int(m[0, 1 + 63]) == (1 << 63) - 1                  # slot 63 is the sign bit
    assert int(m[1, 0]) == 1 | 1 << 33
    assert int(m[1, 1 + 33]) == 1 and int(m[1, 1 + 0]) == 1 << 33
    assert int(m[1, 1 + 40]) == int(m[1, 0])
    with pytest.raises(ValueError):
        ablation_masks(torch.tensor([1]), torch.tensor([1]), 40, 25)
    with pytest.raises(ValueError):
        ablation_masks(torch.tensor([0]), torch.tensor([0]), 0, 0)


# ---- PlanAblation's derived fields

def _hand_made():
    """Four layouts on a handle with 2 camera slots and 1 guard slot.  Row 0: camera + guard (the
    first fixture's ticks).  Row 1: one critical camera.  Row 2: two cameras blocking jointly.
    Row 3: camera 0 matters, camera 1 is redundant, the guard changes the value's last bit only."""
    v = 15.899999999999995
    ticks = torch.tensor([[22, 16, 22, 18], [-1, 14, -1, -1], [-1, -1, -1, -1], [20, 16, 20, 20]], dtype=torch.int16)
    value = torch.tensor([[9.5, 12.25, 9.5, 11.0], [0.5, v, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5],
                          [10.0, 14.0, 10.0, float(np.nextafter(10.0, 11.0))]], dtype=torch.float64)
    filled = torch.tensor([[1, 0, 1], [1, 0, 0], [1, 1, 0], [1, 1, 1]], dtype=torch.bool)
    return ticks, value, filled


def test_plan_ablation_fields():
    ticks, value, filled = _hand_made()
    ab = PlanAblation.from_tables(ticks, value, filled)
    assert ab.ticks is ticks and ab.value is value and torch.equal(ab.filled, filled)
    assert ab.ticks_saved.tolist() == [[6, 0, 4], [0, 0, 0], [0, 0, 0], [4, 0, 0]]
    assert torch.equal(ab.credit, value[:, 1:] - value[:, :1]) and ab.credit.dtype == torch.float64
    assert bool((ab.credit >= 0).all())
    assert ab.critical.tolist() == [[False] * 3, [True, False, False], [False] * 3, [False] * 3]
    # redundant: filled, and neither the ticks nor the value's bits change
    assert ab.redundant.tolist() == [[False] * 3, [False] * 3, [True, True, False], [False, True, False]]
    with pytest.raises(ValueError):
        PlanAblation.from_tables(ticks[:, :3], value, filled)


def test_plan_ablation_metrics():
    ticks, value, filled = _hand_made()
    m = PlanAblation.from_tables(ticks, value, filled).metrics(max_cams=2)
    assert set(m) == {"critical_layout_frac", "redundant_emitter_frac", "camera_credit_mean", "guard_credit_mean"}
    assert m["critical_layout_frac"] == 0.5            # rows 1 and 2 are unsolvable, row 1 has a critical camera
    assert m["redundant_emitter_frac"] == 3 / 8
    cam = [12.25 - 9.5, 15.899999999999995 - 0.5, 0.0, 0.0, 4.0, 0.0]
    assert m["camera_credit_mean"] == pytest.approx(sum(cam) / 6, rel=1e-15)
    assert m["guard_credit_mean"] == pytest.approx((1.5 + (float(np.nextafter(10.0, 11.0)) - 10.0)) / 2, rel=1e-15)
    # nothing to average: zeros, not NaN
    none = PlanAblation.from_tables(ticks[:1, :1].expand(1, 4), value[:1, :1].expand(1, 4),
                                    torch.zeros(1, 3, dtype=torch.bool)).metrics(2)
    assert list(none.values()) == [0.0] * 4


# ---- the library

def test_library_exports_plan_masked():
    if _build.needs_build():
        _build.build()
    lib = ctypes.CDLL(_build.LIB_PATH)
    assert hasattr(lib, "heist_plan_masked") and hasattr(lib, "heist_plan_masked_supported")
    assert {"heist_plan_masked", "heist_plan_masked_supported"} <= set(_native.header_functions())
    assert {"heist_plan_masked", "heist_plan_masked_supported"} <= set(_native.SIGNATURES)
    assert _native.lib().heist_abi_version() == 5
    assert _native.lib().heist_plan_masked_supported(None) == -1  # a bad handle, before any device work
