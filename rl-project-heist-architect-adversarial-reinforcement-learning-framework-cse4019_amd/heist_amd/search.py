"""Exhaustive lookahead on the env kernels: every action sequence of a given length from each root
env, evaluated by forking the roots on the device (HeistEnv.fork_state) and one K-tick launch.

The index math is in three pure functions (no device needed): lookahead_workers picks and checks
the worker envs, action_table builds the launch's actions, select_best picks each root's winner.
"""
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

N_ACTIONS = 5  # WAIT, UP, DOWN, LEFT, RIGHT (environment.py:239-246)


def _digits(depth: int) -> torch.Tensor:
    """[5^depth, depth] int64: row j holds the base-5 digits of j, most significant first, so j
    is the lexicographic rank of its row."""
    j = torch.arange(N_ACTIONS ** depth, dtype=torch.int64)
    return torch.stack([(j // N_ACTIONS ** (depth - 1 - k)) % N_ACTIONS for k in range(depth)], 1)


def lookahead_workers(n_envs: int, roots: Sequence[int], depth: int, workers: Optional[Sequence[int]] = None):
    """The worker envs of a lookahead as int64 [m, 5^depth]: row i is root i's block.  workers:
    at least m 5^depth env ids, the first m 5^depth of which are used in order (default: the envs
    not in roots, ascending).  ValueError for no roots, depth < 1, ids outside [0, n_envs), too
    few workers, a worker named twice or workers that overlap roots."""
    roots = [int(r) for r in roots]
    if not roots:
        raise ValueError("lookahead: no roots")
    if depth < 1:
        raise ValueError("lookahead: depth must be at least 1")
    if any(not 0 <= r < n_envs for r in roots):
        raise ValueError("lookahead: a root outside [0, %d)" % n_envs)
    m, B = len(roots), N_ACTIONS ** depth
    rset = set(roots)
    if workers is None:
        workers = [e for e in range(n_envs) if e not in rset]
    workers = [int(w) for w in workers]
    if len(workers) < m * B:
        raise ValueError("lookahead: %d roots at depth %d need %d workers, got %d" % (m, depth, m * B, len(workers)))
    workers = workers[:m * B]
    if any(not 0 <= w < n_envs for w in workers):
        raise ValueError("lookahead: a worker outside [0, %d)" % n_envs)
    if rset.intersection(workers):
        raise ValueError("lookahead: workers overlap roots")
    if len(set(workers)) != len(workers):
        raise ValueError("lookahead: a worker named twice")
    return torch.tensor(workers, dtype=torch.int64).reshape(m, B)


def action_table(m: int, depth: int, n_envs: int, workers) -> torch.Tensor:
    """The launch's actions, int64 [depth, n_envs]: worker j of root i's block (workers[i][j],
    workers as lookahead_workers gives them) plays the base-5 digits of j, most significant
    first; every other env plays 0 (WAIT)."""
    B = N_ACTIONS ** depth
    w = torch.as_tensor(workers, dtype=torch.int64).reshape(-1)
    if w.numel() != m * B:
        raise ValueError("action_table: %d workers for %d roots at depth %d" % (w.numel(), m, depth))
    table = torch.zeros((depth, n_envs), dtype=torch.int64)
    table[:, w] = _digits(depth).t().repeat(1, m)
    return table


def select_best(returns: torch.Tensor) -> torch.Tensor:
    """int64 [m]: per row of returns [m, B], the lowest index that holds the row's maximum."""
    B = returns.shape[1]
    j = torch.arange(B, dtype=torch.int64, device=returns.device).expand_as(returns)
    top = returns == returns.max(dim=1, keepdim=True).values
    return torch.where(top, j, torch.full_like(j, B)).min(dim=1).values


@dataclass
class LookaheadResult:
    """exhaustive_lookahead's output, tensors on the env's device; B = 5^depth, sequence j of a
    root is the base-5 digits of j, most significant first.
    returns [m, B] float64 -- the sequence's reward64 summed tick by tick in tick order;
    first_reach [m, B] int32 -- the first tick, counted from 1, whose status is vault_reached, -1: none;
    best [m] int64 -- the lowest j with the maximal return;
    best_actions [m, depth] int64 -- its actions;
    workers [m, B] int64 -- the env that played sequence j of root i (it holds the end state)."""
    returns: torch.Tensor
    first_reach: torch.Tensor
    best: torch.Tensor
    best_actions: torch.Tensor
    workers: torch.Tensor


def exhaustive_lookahead(env, roots: Sequence[int], depth: int, workers: Optional[Sequence[int]] = None):
    """Every action sequence of length depth from each env in roots, on env's own kernels: one
    fork_state (root i -> its block of 5^depth workers), one step_multi_records launch of depth
    ticks without auto-reset.  A sequence that ends its episode early collects what the env
    gives afterwards (status already_done).  The launch ticks every env of the handle: the
    workers end in their sequences' final states and every other env, the roots included, has
    played depth WAITs -- keep roots you still need with save_state, or on another handle."""
    from .vec_env import STATUS_CODES
    w = lookahead_workers(env.n_envs, roots, depth, workers)
    m, B = w.shape
    dev = env.device
    src = torch.tensor([int(r) for r in roots], dtype=torch.int32).repeat_interleave(B)
    status = env.fork_state(src, w.reshape(-1))
    if not bool((status != 0).all()):
        raise RuntimeError("exhaustive_lookahead: the device rejected %d forks" % int((status == 0).sum()))
    acts = action_table(m, depth, env.n_envs, w).to(dev)
    _, _, _, st, r64 = env.step_multi_records(acts, auto_reset=False, reward64=True)
    wd = w.to(dev)
    r64, st = r64[:, wd], st[:, wd]  # [depth, m, B]
    returns = r64[0].clone()
    for k in range(1, depth):
        returns = returns + r64[k]
    tick = torch.arange(1, depth + 1, dtype=torch.int32, device=dev).reshape(depth, 1, 1)
    hit = st == STATUS_CODES["vault_reached"]
    first = torch.where(hit, tick, torch.full_like(tick, depth + 1)).min(dim=0).values
    first_reach = torch.where(first <= depth, first, torch.full_like(first, -1))
    best = select_best(returns)
    return LookaheadResult(returns, first_reach, best, _digits(depth).to(dev)[best], wd)
