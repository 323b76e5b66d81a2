"""The planner's references (plan_ref.py) pinned on the 10 x 10 fixtures, and the library's
heist_plan entry points.  No GPU: the oracle search runs the C oracle only."""
import functools

import numpy as np
import pytest

import plan_ref as pr
from heist_amd import _native


@functools.lru_cache(maxsize=None)
def _search(name):
    layout, start, _, _ = pr.CASES[name]
    return pr.oracle_search(pr.GRID, pr.GRID, pr.MAX_STEPS, start, pr.VAULT, layout, pr.BUDGET)


@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_oracle_search_matches_the_table(name):
    _, _, want_T, want_plan = pr.CASES[name]
    T, plan, reach, planes = _search(name)
    assert T == want_T
    assert plan == want_plan
    if name == "wallrow_both":
        assert [int(r.sum()) for r in reach] == pr.BOTH_SIZES
    if name == "wallrow_fixed_cam":  # the set stays at 9 cells until the timeout empties it
        assert len(reach) == pr.MAX_STEPS + 1
        assert [int(r.sum()) for r in reach[9:pr.MAX_STEPS]] == [9] * (pr.MAX_STEPS - 9)
        assert not reach[pr.MAX_STEPS].any()
    if name == "full_wallrow":  # the 3 x 8 interior cells above the wall row, until the timeout
        assert int(reach[-2].sum()) == 3 * 8 and not reach[-1].any()


@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_recurrence_on_the_oracle_planes(name):
    """The NumPy recurrence, fed the oracle's visibility planes, gives the search's sets."""
    layout, start, _, _ = pr.CASES[name]
    T, plan, reach, planes = _search(name)
    from oracle import pyoracle as po
    o = po.OracleEnv(pr.GRID, pr.GRID, pr.MAX_STEPS, start, pr.VAULT, pr.BUDGET)
    o.set_layout(*layout)
    walls = o.grid() == 1  # the layout's walls and the grid's border
    T2, reach2 = pr.plan_from_planes(walls, start, pr.VAULT, planes, 0, pr.MAX_STEPS)
    assert T2 == T and len(reach2) == len(reach)
    for k, (a, b) in enumerate(zip(reach, reach2)):
        np.testing.assert_array_equal(a, b, "tick %d" % k)
    assert pr.backtrack(reach2, T2, pr.VAULT) == plan


def test_plan_follows_its_reach_sets():
    """Replaying the canonical plan in the oracle arrives clean on tick T, never sooner."""
    from oracle import pyoracle as po
    layout, start, T, plan = pr.CASES["wallrow_both"]
    o = po.OracleEnv(pr.GRID, pr.GRID, pr.MAX_STEPS, start, pr.VAULT, pr.BUDGET)
    o.set_layout(*layout)
    o.reset()
    for k, a in enumerate(plan):
        _, done, _ = o.step(a)
        assert done == (k == T - 1)
    i = o.info()
    assert (i["vault_reached"], i["detected"], i["tick"]) == (1, 0, T)


def test_plan_entry_points_exported():
    for name in ("heist_plan", "heist_plan_supported"):
        assert name in _native.SIGNATURES and name in _native.header_functions()
        assert hasattr(_native.lib(), name)
    assert _native.lib().heist_abi_version() == 5
    assert _native.lib().heist_plan_supported(None) == -1  # a bad handle
