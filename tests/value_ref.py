"""References for heist_plan_value (HeistEnv.plan_value): the optimal discounted Solver return from
every cell, none of which uses the kernel under test.

* value_from_planes: the backward recurrence of include/heist.h in NumPy, operation for operation
  in the header's order (every NumPy expression below is one IEEE double operation per element),
  on boolean [R, C] planes, given the visibility plane of every tick.
* oracle_returns / brute_force: no planes and no recurrence -- every action sequence of a given
  length played through the C oracle (oracle.pyoracle.OracleEnv) from scratch, its rewards summed
  from the back (Horner: r_k + gamma * (...)).
* greedy_plan / oracle_replay: the recurrence's own plan from a cell, and the rewards the oracle
  pays for it.
* case_value: the plan_ref.CASES fixtures on the oracle's witness planes (field_ref).
"""
import functools
import itertools

import numpy as np

import field_ref as fr
import plan_ref as pr

REWARD_CONSTS = (-0.01, -1.0, 10.0)  # EnvironmentConfig's reward_step, reward_detection, reward_vault


def manhattan(R, C, vault):
    rr, cc = np.meshgrid(np.arange(R), np.arange(C), indexing="ij")
    return (np.abs(rr - vault[0]) + np.abs(cc - vault[1])).reshape(-1).astype(np.int64)


def value_from_planes(walls, vault, planes, initial_dist, tick0=0, max_steps=200, gamma=1.0,
                      reward_consts=REWARD_CONSTS, done=False):
    """(value [R, C] float64, action [R, C] int8, value_ticks [HK, R, C] float64, action_ticks
    [HK, R, C] int8) for the ticks planes[0], planes[1], ... gives the visibility of (planes[k] is
    vis_{k+1}); HK = min(len(planes), max_steps - tick0), 0 when done.  value_ticks[k] is V_k,
    value = V_0 (all 0.0 / -1 when HK is 0)."""
    walls = np.asarray(walls, bool)
    R, C = walls.shape
    r_step, r_detect, r_vault = (np.float64(v) for v in reward_consts)
    gamma = np.float64(gamma)
    D0 = int(initial_dist)
    HK = 0 if done else max(0, min(len(planes), max_steps - tick0))
    mv = fr.moves(walls).reshape(5, -1)
    dist = manhattan(R, C, vault)
    vcell = vault[0] * C + vault[1]
    wall = walls.reshape(-1)
    nxt = np.zeros(R * C, np.float64)  # V_HK
    vt = np.zeros((HK, R, C), np.float64)
    at = np.full((HK, R, C), -1, np.int8)
    for k in range(HK - 1, -1, -1):
        seen_plane = np.asarray(planes[k], bool).reshape(-1)
        last = tick0 + k + 1 >= max_steps
        best = np.zeros(R * C, np.float64)
        act = np.full(R * C, -1, np.int8)
        for a in range(5):
            y = mv[a]
            curr = dist[y]
            rew = np.full(R * C, r_step, np.float64)
            rew = rew + (dist - curr).astype(np.float64) * np.float64(0.1)
            if D0 > 3:
                rew = np.where(curr <= 3, rew + np.float64(0.05) * (3 - curr).astype(np.float64), rew)
            seen = seen_plane[y]
            rew = np.where(seen, rew + r_detect, rew)
            atv = y == vcell
            rew = np.where(atv, rew + r_vault, rew)
            if last:
                frac = np.float64(1.0) - curr.astype(np.float64) / np.float64(max(D0, 1))
                frac = np.where(frac < 0, np.float64(0.0), frac)
                rew = rew + frac * np.float64(2.0)
            q = np.where(seen | atv | last, rew, rew + gamma * nxt[y])
            better = (q > best) if a else np.ones(R * C, bool)  # strict: the first maximum stays
            best = np.where(better, q, best)
            act = np.where(better, a, act).astype(np.int8)
        best[wall] = 0.0
        act[wall] = -1
        vt[k], at[k] = best.reshape(R, C), act.reshape(R, C)
        nxt = best
    if HK:
        return vt[0].copy(), at[0].copy(), vt, at
    return np.zeros((R, C), np.float64), np.full((R, C), -1, np.int8), vt, at


def horner(rewards, gamma):
    """r_0 + gamma * (r_1 + gamma * (...)) over the last axis, from the back, in float64."""
    r = np.asarray(rewards, np.float64)
    acc = r[..., -1].copy()
    for k in range(r.shape[-1] - 2, -1, -1):
        acc = r[..., k] + np.float64(gamma) * acc
    return acc


def greedy_plan(walls, vault, planes, action_ticks, start):
    """The recurrence's own play from `start`: action_ticks[k] at the Solver's cell, moved by the
    walls, up to and including the step that ends on a seen cell, on the vault or on the last row."""
    mv = fr.moves(np.asarray(walls, bool))
    C = walls.shape[1]
    x, plan = start[0] * C + start[1], []
    for k in range(len(action_ticks)):
        a = int(action_ticks[k].reshape(-1)[x])
        assert a >= 0, "no action at step %d" % k
        plan.append(a)
        x = int(mv[a].reshape(-1)[x])
        if np.asarray(planes[k], bool).reshape(-1)[x] or x == vault[0] * C + vault[1]:
            break
    return plan


def oracle_replay(R, C, max_steps, start, vault, layout, budget, actions, reward_consts=REWARD_CONSTS):
    """([reward64 per action], [done per action]) of a fresh OracleEnv fed `actions` (a done env
    pays 0.0)."""
    o = fr.po.OracleEnv(R, C, max_steps, start, vault, budget, *reward_consts)
    o.set_layout(*layout)
    o.reset()
    out = [o.step(int(a))[:2] for a in actions]
    return [r for r, _ in out], [d for _, d in out]


def oracle_returns(R, C, max_steps, start, vault, layout, budget, depth):
    """[5^depth, depth] float64: the oracle's rewards of every action sequence of length depth
    from reset, row j being the base-5 digits of j, most significant first."""
    out = np.empty((5 ** depth, depth), np.float64)
    for j, seq in enumerate(itertools.product(range(5), repeat=depth)):
        out[j] = oracle_replay(R, C, max_steps, start, vault, layout, budget, seq)[0]
    return out


def brute_force(R, C, max_steps, start, vault, layout, budget, depth, gammas):
    """{gamma: the largest Horner-summed return over all 5^depth sequences}."""
    rewards = oracle_returns(R, C, max_steps, start, vault, layout, budget, depth)
    return {g: float(horner(rewards, g).max()) for g in gammas}


def bits(x):
    """float64 -> int64, the comparison every test uses."""
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.int64)


@functools.lru_cache(maxsize=None)
def case_value(name, gamma, initial_dist=None):
    """A plan_ref.CASES fixture from reset, all 40 ticks: (value, action, value_ticks,
    action_ticks) of value_from_planes on field_ref.case_reference's witness planes.  initial_dist
    defaults to the distance from plan_ref.START (what a handle configured with that start holds,
    whatever cell a state edit parks the Solver on).  Computed once; callers must not modify it."""
    planes, walls = fr.case_reference(name)[:2]
    d0 = abs(pr.START[0] - pr.VAULT[0]) + abs(pr.START[1] - pr.VAULT[1]) if initial_dist is None else initial_dist
    return value_from_planes(walls, pr.VAULT, planes, d0, 0, pr.MAX_STEPS, gamma)


def cases_value(names, W, gamma):
    """The reference values of the named fixtures as a CPU heist_amd.PlanValue (H = 40), each with
    the initial_dist of its own start cell."""
    import torch
    from heist_amd import PlanValue
    refs, grids = [], []
    for n in names:
        start = pr.CASES[n][1]
        refs.append(case_value(n, gamma, abs(start[0] - pr.VAULT[0]) + abs(start[1] - pr.VAULT[1])))
        grids.append(fr.case_reference(n)[1].astype(np.int8))  # 1 = wall, which is all follow_value reads
    vis = np.stack([fr.pack_planes(fr.case_reference(n)[0], W) for n in names], 1)
    t = torch.from_numpy
    return PlanValue(t(np.stack([r[0] for r in refs])), t(np.stack([r[1] for r in refs])), t(vis.view(np.int32)),
                     t(np.stack([r[2] for r in refs], 1)), t(np.stack([r[3] for r in refs], 1)), pr.GRID, pr.GRID,
                     pr.VAULT, float(gamma), t(np.stack(grids)))
