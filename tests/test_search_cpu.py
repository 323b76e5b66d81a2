"""The index math of heist_amd.search (no device): the base-5 action table, the assignment of
worker envs to roots, the argument checks and the tie rule of the selection."""
import itertools

import pytest
import torch

from heist_amd import search


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_action_table_is_base5_most_significant_first(depth):
    B = 5 ** depth
    n = B + 3
    w = search.lookahead_workers(n, [0], depth)
    assert w.shape == (1, B) and w.dtype == torch.int64
    table = search.action_table(1, depth, n, w)
    assert table.shape == (depth, n) and table.dtype == torch.int64
    seqs = [tuple(int(a) for a in table[:, int(w[0, j])]) for j in range(B)]
    assert seqs == list(itertools.product(range(5), repeat=depth))  # j is the lexicographic rank
    for j, s in enumerate(seqs):
        assert sum(a * 5 ** (depth - 1 - k) for k, a in enumerate(s)) == j
    used = set(w.reshape(-1).tolist())
    for e in range(n):
        if e not in used:
            assert not table[:, e].any()  # the root and the spare envs wait


def test_blocks_of_workers_per_root():
    depth, roots, n = 2, [7, 0, 30], 90
    B = 25
    w = search.lookahead_workers(n, roots, depth)
    rest = [e for e in range(n) if e not in roots]
    assert w.tolist() == [rest[i * B:(i + 1) * B] for i in range(3)]  # ascending, root i owns block i
    table = search.action_table(3, depth, n, w)
    for i in range(3):
        for j in (0, 1, 7, 24):
            assert table[:, int(w[i, j])].tolist() == [j // 5, j % 5]
    for e in roots + rest[3 * B:]:
        assert not table[:, e].any()
    # the caller's own workers, in the caller's order; surplus ones are left alone
    mine = list(range(89, 9, -1))
    w2 = search.lookahead_workers(n, [1, 2, 3], depth, mine)
    assert w2.reshape(-1).tolist() == mine[:75]
    t2 = search.action_table(3, depth, n, w2)
    assert t2[:, 89].tolist() == [0, 0] and t2[:, 88].tolist() == [0, 1] and t2[:, 89 - 25 - 7].tolist() == [1, 2]
    assert not t2[:, :15].any()
    # a root may be named twice: two blocks with the same source
    assert search.lookahead_workers(60, [4, 4], 2).shape == (2, 25)


def test_value_errors():
    with pytest.raises(ValueError, match="need 50 workers"):
        search.lookahead_workers(51, [0, 1], 2)  # 49 envs left
    assert search.lookahead_workers(52, [0, 1], 2).shape == (2, 25)
    with pytest.raises(ValueError, match="overlap"):
        search.lookahead_workers(40, [3], 1, [1, 2, 3, 4, 5])
    with pytest.raises(ValueError, match="need 5 workers"):
        search.lookahead_workers(40, [3], 1, [1, 2, 4, 5])
    with pytest.raises(ValueError, match="twice"):
        search.lookahead_workers(40, [3], 1, [1, 2, 2, 4, 5])
    with pytest.raises(ValueError, match="outside"):
        search.lookahead_workers(40, [3], 1, [1, 2, 40, 4, 5])
    with pytest.raises(ValueError, match="outside"):
        search.lookahead_workers(40, [40], 1)
    with pytest.raises(ValueError, match="no roots"):
        search.lookahead_workers(40, [], 1)
    with pytest.raises(ValueError, match="depth"):
        search.lookahead_workers(40, [0], 0)
    with pytest.raises(ValueError, match="workers for"):
        search.action_table(2, 1, 40, [1, 2, 3, 4, 5])


def test_best_is_the_lowest_index_among_equal_returns():
    r = torch.tensor([[0.5, 2.0, 2.0, -1.0, 2.0],
                      [-0.03, -0.03, -0.03, -0.03, -0.03],
                      [-1.0, -0.5, -0.75, -0.5, -2.0],
                      [0.0, 0.0, 0.0, 0.0, 1e-300]], dtype=torch.float64)
    best = search.select_best(r)
    assert best.dtype == torch.int64 and best.tolist() == [1, 0, 1, 4]
    assert search.select_best(r.flip(1)).tolist() == [0, 0, 1, 0]
