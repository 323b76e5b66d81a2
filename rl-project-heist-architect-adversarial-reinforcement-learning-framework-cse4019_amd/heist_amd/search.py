"""Exhaustive lookahead on the env kernels: every action sequence of a given length from each root
env, evaluated by forking the roots on the device (HeistEnv.fork_state) and one K-tick launch.

The index math is in three pure functions (no device needed): lookahead_workers picks and checks
the worker envs, action_table builds the launch's actions, select_best picks each root's winner.

follow_field and expert_labels read a planner field (HeistEnv.plan_field(all_ticks=True)): the
field's own plan from any cell, and the exact ticks to go and optimal action of every state a
rollout visited.  Both are pure torch and run wherever the field's tensors live.

follow_value, value_targets and discounted_return do the same for a planner value
(HeistEnv.plan_value(all_ticks=True)): the return-optimal play from any cell, the exact optimal
return and action of every state a rollout visited, and the return a played rollout collected,
summed in the value's own order.

play_table restates heist_plan_play (HeistEnv.plan_play) in pure torch on CPU tensors: one episode
per env played from per-tick tables, optionally perturbed by counter-hashed uniform actions.
expert_data / expert_rollout turn such a play into exactly labelled decision states (ExpertData)
for SolverAgent.imitation_update.

q_values restates heist_plan_q (HeistEnv.plan_q) in pure torch on any device: the five exact action
values of visited states, their maximum, the set of optimal actions and the gap of the action taken.

camera_candidates, placement_scan, relocation_scan and greedy_cameras ask the Architect's side of
the question with heist_plan_place (HeistEnv.plan_place): what one more camera on any interior cell
would cost the Solver, where else a camera the layout has could have stood, and the exact greedy
adversary built camera by camera.

architect_patrol, guard_candidates, guard_placement_scan and greedy_adversary ask the same of the
guard with heist_plan_place_guard (HeistEnv.plan_place_guard): what one more Architect guard on any
interior tile would cost the Solver, and the exact greedy adversary under the game's own cost table,
cameras at 3 points against guards at 5.

wall_ablation_edits, WallAblation, wall_candidates, wall_placement_scan and greedy_walls ask it of the
third asset with heist_plan_walls (HeistEnv.plan_walls): which wall a layout's difficulty is due to,
which one the Solver hides behind, what one more wall on any interior tile would do, and the exact
greedy wall adversary, every variant cast against its own walls.
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


DELTA = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))  # the actions' (dr, dc)


def _field_action(field, k: int, r: torch.Tensor, c: torch.Tensor):
    """The planner field's rule at tick k for env i's Solver on cell (r[i], c[i]): (togo [N] int64,
    action [N] int64, next r, next c).  action is the lowest a for which y = move(x, a) is not in
    vis_{k+1} and y is the vault or togo_{k+1}[y] == togo_k[x] - 1; -1 (and the cell kept) where
    togo_k[x] is -1.  A move into a wall or off the grid is a stay, which WAIT already covers, so
    only real moves are tried for a = 1 .. 4 (a wall's togo is -1: it never matches)."""
    tg, vis = field.togo_ticks, field.vis
    H, N, R, C = tg.shape
    vr, vc = field.vault
    n = torch.arange(N, device=tg.device)
    r, c = r.long(), c.long()
    cur = tg[k, n, r, c].long()
    act = torch.full_like(cur, -1)
    nr, nc = r.clone(), c.clone()
    for a in range(N_ACTIONS - 1, -1, -1):
        yr, yc = r + DELTA[a][0], c + DELTA[a][1]
        inside = (yr >= 0) & (yr < R) & (yc >= 0) & (yc < C)
        yr, yc = yr.clamp(0, R - 1), yc.clamp(0, C - 1)
        cell = yr * C + yc
        seen = ((vis[k, n, cell >> 5].long() >> (cell & 31)) & 1).bool()
        nxt = tg[k + 1, n, yr, yc].long() if k + 1 < H else torch.full_like(cur, -1)
        ok = inside & ~seen & (cur > 0) & (((yr == vr) & (yc == vc)) | ((nxt > 0) & (nxt == cur - 1)))
        act = torch.where(ok, torch.full_like(act, a), act)
        nr, nc = torch.where(ok, yr, nr), torch.where(ok, yc, nc)
    return cur, act, nr, nc


def _need_all_ticks(field, what):
    if field.togo_ticks is None:
        raise ValueError("%s: the field has no togo_ticks (plan_field(all_ticks=True))" % what)
    if field.vault is None:
        raise ValueError("%s: the field does not name its vault" % what)


def follow_field(field, pos_r, pos_c):
    """The field's own plan from each env's cell (pos_r, pos_c: [N]): (actions [H, N] int64,
    ticks [N] int32).  At tick k the Solver takes the lowest optimal action (_field_action) until
    it stands on the vault; the rows after that, and every row of an env whose cell has no value,
    are 0 -- feed the tensor (or its first rows) to step_multi(auto_reset=False).  ticks is togo_0
    at the start cell.  Pure torch: runs on the device of the field's tensors, CPU included."""
    _need_all_ticks(field, "follow_field")
    tg = field.togo_ticks
    H, N = tg.shape[:2]
    dev = tg.device
    r = torch.as_tensor(pos_r, device=dev).long().reshape(N)
    c = torch.as_tensor(pos_c, device=dev).long().reshape(N)
    actions = torch.zeros((H, N), dtype=torch.int64, device=dev)
    ticks = tg[0, torch.arange(N, device=dev), r, c].to(torch.int32)
    alive = ticks > 0
    vr, vc = field.vault
    for k in range(H):
        if not bool(alive.any()):
            break
        _, act, nr, nc = _field_action(field, k, r, c)
        go = alive & (act >= 0)
        actions[k] = torch.where(go, act, torch.zeros_like(act))
        r, c = torch.where(go, nr, r), torch.where(go, nc, c)
        alive = go & ~((r == vr) & (c == vc))
    return actions, ticks


def expert_labels(field, pos_r, pos_c):
    """Exact labels along a rollout: pos_r, pos_c [K, N] with K <= H, row k the Solver's cell after
    k ticks (row 0 the cell now, rows 1 .. the position word of a step_multi_records launch played
    without auto-reset).  Returns (togo [K, N] int16, action [K, N] int8): the fewest ticks to go
    from that state and the lowest optimal action in it (follow_field's rule), -1 where the vault
    is out of reach.  Pure torch."""
    _need_all_ticks(field, "expert_labels")
    tg = field.togo_ticks
    H, N = tg.shape[:2]
    dev = tg.device
    pr, pc = torch.as_tensor(pos_r, device=dev).long(), torch.as_tensor(pos_c, device=dev).long()
    if pr.dim() != 2 or pr.shape != pc.shape or pr.shape[1] != N or pr.shape[0] > H:
        raise ValueError("expert_labels: cells must be [K, %d] with K <= %d" % (N, H))
    K = pr.shape[0]
    togo = torch.empty((K, N), dtype=torch.int16, device=dev)
    action = torch.empty((K, N), dtype=torch.int8, device=dev)
    for k in range(K):
        cur, act, _, _ = _field_action(field, k, pr[k], pc[k])
        togo[k], action[k] = cur.to(torch.int16), act.to(torch.int8)
    return togo, action


def _need_value_ticks(pv, what, values=False):
    if pv.action_ticks is None or (values and pv.value_ticks is None):
        raise ValueError("%s: the value has no per-tick rows (plan_value(all_ticks=True))" % what)
    if pv.vault is None or pv.grid is None:
        raise ValueError("%s: the value does not name its vault and grid" % what)


def follow_value(pv, pos_r, pos_c):
    """The return-optimal play from each env's cell (pos_r, pos_c: [N]) as actions [H, N] int64:
    at step k the Solver takes pv.action_ticks[k] at its cell and moves by pv.grid's walls (a move
    into a wall or off the grid is a stay).  The rows after the play's terminal step -- the step
    that ends on a seen cell, on the vault or on the env's last tick -- are 0, as is every row of
    an env with nothing to play; feed the tensor (or its first rows) to
    step_multi(auto_reset=False).  Pure torch: runs where pv's tensors live, CPU included."""
    _need_value_ticks(pv, "follow_value")
    at, vis = pv.action_ticks, pv.vis
    H, N, R, C = at.shape
    dev = at.device
    n = torch.arange(N, device=dev)
    r = torch.as_tensor(pos_r, device=dev).long().reshape(N)
    c = torch.as_tensor(pos_c, device=dev).long().reshape(N)
    walls = pv.grid.to(dev) == 1
    vr, vc = pv.vault
    dr = torch.tensor([d[0] for d in DELTA], device=dev)
    dc = torch.tensor([d[1] for d in DELTA], device=dev)
    actions = torch.zeros((H, N), dtype=torch.int64, device=dev)
    alive = torch.ones(N, dtype=torch.bool, device=dev)
    for k in range(H):
        act = at[k, n, r, c].long()
        alive = alive & (act >= 0)  # -1: past the env's ticks (or a wall cell)
        if not bool(alive.any()):
            break
        a = torch.where(alive, act, torch.zeros_like(act))
        actions[k] = a
        yr, yc = r + dr[a], c + dc[a]
        ok = (yr >= 0) & (yr < R) & (yc >= 0) & (yc < C)
        yr, yc = yr.clamp(0, R - 1), yc.clamp(0, C - 1)
        ok = ok & ~walls[n, yr, yc] & alive
        r, c = torch.where(ok, yr, r), torch.where(ok, yc, c)
        cell = r * C + c
        seen = ((vis[k, n, cell >> 5].long() >> (cell & 31)) & 1).bool()
        alive = alive & ~seen & ~((r == vr) & (c == vc))
    return actions


def value_targets(pv, pos_r, pos_c):
    """Exact critic targets along a rollout: pos_r, pos_c [K, N] with K <= H, row k the Solver's
    cell after k ticks (expert_labels' convention).  Returns (value [K, N] float64, action [K, N]
    int8): pv.value_ticks[k] and pv.action_ticks[k] at that cell -- the optimal return still to
    collect from that state and the action that starts it.  Pure torch."""
    _need_value_ticks(pv, "value_targets", values=True)
    vt, at = pv.value_ticks, pv.action_ticks
    H, N = vt.shape[:2]
    dev = vt.device
    pr, pc = torch.as_tensor(pos_r, device=dev).long(), torch.as_tensor(pos_c, device=dev).long()
    if pr.dim() != 2 or pr.shape != pc.shape or pr.shape[1] != N or pr.shape[0] > H:
        raise ValueError("value_targets: cells must be [K, %d] with K <= %d" % (N, H))
    K = pr.shape[0]
    k = torch.arange(K, device=dev).reshape(K, 1).expand(K, N)
    n = torch.arange(N, device=dev).reshape(1, N).expand(K, N)
    return vt[k, n, pr, pc], at[k, n, pr, pc]


def discounted_return(reward64, done, gamma):
    """[N] float64: per env the Horner sum r_k + gamma * (r_{k+1} + gamma * (...)) of reward64
    [K, N], started at the env's first tick with done [K, N] set (row K - 1 when there is none)
    and run backwards to row 0, every operation in float64 and in this order -- the order of
    heist_plan_value's recurrence, so PlanValue.value at the start cell minus this is a regret
    that is exactly 0.0 for the play follow_value gives.  Pure torch."""
    r = torch.as_tensor(reward64).to(torch.float64)
    d = torch.as_tensor(done, device=r.device).bool()
    if r.dim() != 2 or r.shape != d.shape:
        raise ValueError("discounted_return: reward64 and done must both be [K, N]")
    K, N = r.shape
    k = torch.arange(K, device=r.device).reshape(K, 1)
    end = torch.where(d, k, torch.full_like(k, K - 1)).min(dim=0).values  # [N]
    acc = torch.zeros(N, dtype=torch.float64, device=r.device)
    g = float(gamma)
    for i in range(K - 1, -1, -1):
        tail = g * acc
        acc = torch.where(i > end, acc, torch.where(i == end, r[i], r[i] + tail))
    return acc


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


# ---- planner playout (heist_plan_play, include/heist.h) in pure torch

_M64 = (1 << 64) - 1


def _i64(c: int) -> int:
    """A 64-bit constant as the int64 with the same bits."""
    c &= _M64
    return c - (1 << 64) if c >> 63 else c


def _lsr(z: torch.Tensor, s: int) -> torch.Tensor:
    """Logical right shift of int64 bit patterns."""
    return (z >> s) & ((1 << (64 - s)) - 1)


def _mix64(z: torch.Tensor) -> torch.Tensor:
    """The header's mix64 (splitmix64 finaliser) on int64 bit patterns; int64 products wrap mod 2^64."""
    z = z ^ _lsr(z, 30)
    z = z * _i64(0xBF58476D1CE4E5B9)
    z = z ^ _lsr(z, 27)
    z = z * _i64(0x94D049BB133111EB)
    return z ^ _lsr(z, 31)


def play_draws(seed: int, tick: torch.Tensor, env: torch.Tensor) -> torch.Tensor:
    """heist_plan_play's draw z of (seed, absolute tick, env) as int64 bit patterns, broadcast over
    tick and env."""
    key = (tick.to(torch.int64) * _i64(0xD1B54A32D192ED03)) ^ (env.to(torch.int64) * _i64(0x9E3779B97F4A7C15))
    return _mix64(key ^ _i64(int(seed)))


def play_table(table, vis, grid, tick, pos, max_steps, initial_dist, vault, reward_consts=(-0.01, -1.0, 10.0),
               values=None, done=None, noise=0.0, seed=0, records=True, rewards=True):
    """heist_plan_play's contract (include/heist.h) in pure torch on CPU tensors, with the handle's
    share passed in: table [H, N, R, C] int8, vis [H, N, W] int32, grid [N, R, C] int8 (1 = wall),
    tick [N] and done [N] (None: none done) the envs' ticks and done flags, pos [N, 2] the start
    cells, max_steps, initial_dist [N], vault (row, col), reward_consts (step, detection, vault),
    values [H, N, R, C] float64 or None.  Returns a PlanPlay equal to HeistEnv.plan_play's on the
    same tensors, float64 bit for bit (every reward line is one IEEE double operation)."""
    from .vec_env import PlanPlay, STATUS_CODES, noise_q24
    at = torch.as_tensor(table)
    H, N, R, C = at.shape
    RC = R * C
    at = at.reshape(H, N, RC)
    vis = torch.as_tensor(vis)
    W, nvis = int(vis.shape[2]), (RC + 31) // 32
    vt = None if values is None else torch.as_tensor(values).reshape(H, N, RC)
    walls = torch.as_tensor(grid).reshape(N, R, C) == 1
    tick = torch.as_tensor(tick).to(torch.int64).reshape(N)
    D0 = torch.as_tensor(initial_dist).to(torch.int64).reshape(N)
    pos = torch.as_tensor(pos).to(torch.int64).reshape(N, 2)
    fin = torch.zeros(N, dtype=torch.bool) if done is None else torch.as_tensor(done).reshape(N) != 0
    q24 = noise_q24(noise)
    r_step, r_detect, r_vault = (float(v) for v in reward_consts)
    vr, vc = int(vault[0]), int(vault[1])
    n = torch.arange(N)
    HK = torch.clamp(torch.clamp(int(max_steps) - tick, max=H), min=0)
    HK = torch.where(fin, torch.zeros_like(HK), HK)
    r, c = pos[:, 0].clone(), pos[:, 1].clone()
    off = (r < 0) | (r >= R) | (c < 0) | (c >= C)
    r, c = r.clamp(0, R - 1), c.clamp(0, C - 1)
    live = (HK > 0) & ~off
    out = PlanPlay(torch.zeros((H, N), dtype=torch.int64), torch.full((H, N), -1, dtype=torch.int8),
                   None if vt is None else torch.zeros((H, N), dtype=torch.float64),
                   torch.zeros((H, N, W), dtype=torch.int32) if records else None,
                   torch.zeros((H, N), dtype=torch.float64) if rewards else None,
                   torch.ones((H, N), dtype=torch.bool),
                   torch.full((H, N), STATUS_CODES["already_done"], dtype=torch.int8),
                   torch.zeros(N, dtype=torch.int32))
    dr = torch.tensor([d[0] for d in DELTA])
    dc = torch.tensor([d[1] for d in DELTA])
    denom = torch.clamp(D0, min=1).to(torch.float64)
    for k in range(H):
        play = live & (k < HK)
        if not bool(play.any()):
            break
        x = r * C + c
        t = at[k, n, x].to(torch.int64)
        ex = torch.where((t < 0) | (t > 4), torch.full_like(t, -1), t)
        z = play_draws(seed, tick + k, n)
        noisy = _lsr(z, 40) < q24
        a = torch.where(noisy, ((z & 0xFFFFFFFF) * 5) >> 32, ex.clamp(min=0))
        yr, yc = r + dr[a], c + dc[a]
        ok = (yr >= 0) & (yr < R) & (yc >= 0) & (yc < C)
        yr, yc = yr.clamp(0, R - 1), yc.clamp(0, C - 1)
        ok = ok & ~walls[n, yr, yc]
        yr, yc = torch.where(ok, yr, r), torch.where(ok, yc, c)
        y = yr * C + yc
        seen = ((vis[k, n, y >> 5].to(torch.int64) >> (y & 31)) & 1).bool()
        atv = (yr == vr) & (yc == vc)
        last = tick + k + 1 >= int(max_steps)
        dx, curr = (r - vr).abs() + (c - vc).abs(), (yr - vr).abs() + (yc - vc).abs()
        rew = torch.full((N,), r_step, dtype=torch.float64)
        rew = rew + (dx - curr).to(torch.float64) * 0.1
        rew = torch.where((curr <= 3) & (D0 > 3), rew + 0.05 * (3 - curr).to(torch.float64), rew)
        rew = torch.where(seen, rew + r_detect, rew)
        rew = torch.where(atv, rew + r_vault, rew)
        frac = 1.0 - curr.to(torch.float64) / denom
        frac = torch.where(frac < 0, torch.zeros_like(frac), frac)
        rew = torch.where(last, rew + frac * 2.0, rew)
        status = torch.zeros(N, dtype=torch.int8)
        status[seen] = STATUS_CODES["detected"]
        status[atv] = STATUS_CODES["vault_reached"]
        status[last] = STATUS_CODES["timeout"]
        end = seen | atv | last
        out.actions[k, play] = a[play]
        out.expert[k, play] = ex[play].to(torch.int8)
        if vt is not None:
            out.value[k, play] = vt[k, n, x][play]
        if records:
            rec = vis[k].clone()
            rec[:, nvis] = (yr | (yc << 8)).to(torch.int32)
            out.records[k, play] = rec[play]
        if rewards:
            out.reward64[k, play] = rew[play]
        out.done[k, play] = end[play]
        out.status[k, play] = status[play]
        out.length += play.to(torch.int32)
        r, c = torch.where(play, yr, r), torch.where(play, yc, c)
        live = play & ~end
    out.length[off] = -1
    return out


# ---- planner Q (heist_plan_q, include/heist.h) in pure torch

def q_values(values, vis, grid, tick0, pos, max_steps, initial_dist, vault, reward_consts=(-0.01, -1.0, 10.0),
             gamma=1.0, taken=None):
    """heist_plan_q's contract (include/heist.h) in pure torch on any device, with the handle's share
    passed in: values [H, N, R, C] float64, vis [H, N, W] int32, grid [N, R, C] int8 (1 = wall),
    tick0 [N] each env's tick when the tables were made (-1: done then), pos [K, N, 2] the visited
    cells, max_steps, initial_dist [N], vault (row, col), reward_consts (step, detection, vault),
    taken [K, N] or None.  Returns a PlanQ equal to HeistEnv.plan_q's on the same tensors, float64
    bit for bit: every reward line is one IEEE double operation, in the header's order."""
    from .vec_env import PlanQ
    vt = torch.as_tensor(values)
    dev = vt.device
    H, N = int(vt.shape[0]), int(vt.shape[1])
    walls = torch.as_tensor(grid, device=dev).reshape(N, *vt.shape[2:]) == 1
    R, C = int(walls.shape[1]), int(walls.shape[2])
    RC = R * C
    vt, walls = vt.reshape(H, N, RC), walls.reshape(N, RC)
    vis = torch.as_tensor(vis, device=dev)
    pos = torch.as_tensor(pos, device=dev).to(torch.int64)
    if pos.dim() != 3 or tuple(pos.shape[1:]) != (N, 2) or not 1 <= pos.shape[0] <= H:
        raise ValueError("q_values: pos must be [K, %d, 2] with 1 <= K <= %d" % (N, H))
    K = int(pos.shape[0])
    t0 = torch.as_tensor(tick0, device=dev).to(torch.int64).reshape(1, N)
    D0 = torch.as_tensor(initial_dist, device=dev).to(torch.int64).reshape(1, N)
    r_step, r_detect, r_vault = (float(v) for v in reward_consts)
    g = float(gamma)
    vr, vc = int(vault[0]), int(vault[1])
    k = torch.arange(K, device=dev).reshape(K, 1).expand(K, N)
    n = torch.arange(N, device=dev).reshape(1, N).expand(K, N)
    HK = torch.clamp(torch.clamp(int(max_steps) - t0, max=H), min=0)
    HK = torch.where(t0 < 0, torch.zeros_like(HK), HK)
    r, c = pos[..., 0], pos[..., 1]
    inside = (r >= 0) & (r < R) & (c >= 0) & (c < C)
    r, c = torch.where(inside, r, torch.zeros_like(r)), torch.where(inside, c, torch.zeros_like(c))
    x = r * C + c
    live = (k < HK) & inside & ~walls[n, x]
    last = (t0 + k + 1) >= int(max_steps)
    bonus = D0 > 3
    denom = torch.clamp(D0, min=1).to(torch.float64)
    dx = (r - vr).abs() + (c - vc).abs()
    kn = (k + 1).clamp(max=H - 1)
    qs = []
    for a in range(N_ACTIONS):
        yr, yc = r + DELTA[a][0], c + DELTA[a][1]
        ok = (yr >= 0) & (yr < R) & (yc >= 0) & (yc < C)
        yr, yc = yr.clamp(0, R - 1), yc.clamp(0, C - 1)
        ok = ok & ~walls[n, yr * C + yc]
        yr, yc = torch.where(ok, yr, r), torch.where(ok, yc, c)
        y = yr * C + yc
        curr = (yr - vr).abs() + (yc - vc).abs()
        rew = torch.full((K, N), r_step, dtype=torch.float64, device=dev)
        rew = rew + (dx - curr).to(torch.float64) * 0.1
        rew = torch.where((curr <= 3) & bonus, rew + 0.05 * (3 - curr).to(torch.float64), rew)
        seen = ((vis[k, n, y >> 5].to(torch.int64) >> (y & 31)) & 1).bool()
        rew = torch.where(seen, rew + r_detect, rew)
        atv = (yr == vr) & (yc == vc)
        rew = torch.where(atv, rew + r_vault, rew)
        frac = 1.0 - curr.to(torch.float64) / denom
        frac = torch.where(frac < 0, torch.zeros_like(frac), frac)
        rew = torch.where(last, rew + frac * 2.0, rew)
        nxt = torch.where(k + 1 < H, vt[kn, n, y], torch.zeros_like(rew))
        on = rew + g * nxt
        qs.append(torch.where(seen | atv | last, rew, on))
    value, best = qs[0], torch.zeros((K, N), dtype=torch.int8, device=dev)
    for a in range(1, N_ACTIONS):
        better = qs[a] > value  # strict: the first maximum stays
        value = torch.where(better, qs[a], value)
        best = torch.where(better, torch.full_like(best, a), best)
    optimal = torch.zeros((K, N), dtype=torch.uint8, device=dev)
    for a in range(N_ACTIONS):
        optimal = optimal | ((qs[a] == value).to(torch.uint8) << a)
    q = torch.stack(qs, -1)
    zero = torch.zeros_like(value)
    gap = None
    if taken is not None:
        tk = torch.as_tensor(taken, device=dev).to(torch.int64).reshape(K, N)
        tk = torch.where((tk < 0) | (tk > 4), torch.zeros_like(tk), tk)
        gap = torch.where(live, value - q.gather(2, tk.unsqueeze(-1)).squeeze(-1), zero)
    return PlanQ(torch.where(live.unsqueeze(-1), q, torch.zeros_like(q)), torch.where(live, value, zero),
                 torch.where(live, best, torch.full_like(best, -1)),
                 torch.where(live, optimal, torch.zeros_like(optimal)), gap)


@dataclass
class ExpertData:
    """Decision states of a table playout, [H, N] time-major: decision k of env e is the state the
    play's step k was taken from, valid iff k < length[e].
    records [H, N, W] int32 -- decision k's observation record (decision 0: the caller's, decision
        k >= 1: the play's record k - 1);
    expert [H, N] int8 -- the table's action there (-1: none), value [H, N] float64 or None -- the
        table's value there, taken [H, N] int64 -- the action the play took;
    valid [H, N] bool, length [N] int32; grid [N, R, C] int8 -- the tile map the records expand by;
    optimal [H, N] uint8 or None -- the set of optimal actions there as a bit mask (PlanQ.optimal)."""
    records: torch.Tensor
    expert: torch.Tensor
    value: Optional[torch.Tensor]
    taken: torch.Tensor
    valid: torch.Tensor
    length: torch.Tensor
    grid: torch.Tensor
    rows: int
    cols: int
    vault: tuple
    optimal: Optional[torch.Tensor] = None

    def flat(self, mask=None):
        """The valid decisions (of the envs mask [N] bool selects; None: all) as (CompactObs, expert
        int64, value float32 or None, taken int64), env-minor in tick order."""
        from .obs_compact import CompactObs
        H, N = self.valid.shape
        keep = self.valid
        if mask is not None:
            keep = keep & torch.as_tensor(mask, device=keep.device).bool().reshape(1, N)
        idx = keep.reshape(-1).nonzero().reshape(-1)
        env = torch.arange(N, dtype=torch.int32, device=idx.device).repeat(H)[idx]
        obs = CompactObs(self.records.reshape(H * N, -1)[idx], env, self.grid, self.rows, self.cols, self.vault)
        value = None if self.value is None else self.value.reshape(-1)[idx].to(torch.float32)
        return obs, self.expert.reshape(-1)[idx].to(torch.int64), value, self.taken.reshape(-1)[idx]

    def flat_optimal(self, mask=None):
        """flat(mask)'s four values plus the optimal sets of the same decisions, [M] uint8 (None
        when the data has none): SolverAgent.imitation_update's optimal."""
        out = self.flat(mask)
        if self.optimal is None:
            return out + (None,)
        keep = self.valid
        if mask is not None:
            keep = keep & torch.as_tensor(mask, device=keep.device).bool().reshape(1, -1)
        return out + (self.optimal.reshape(-1)[keep.reshape(-1).nonzero().reshape(-1)],)


def expert_data(play, records0, grid, rows, cols, vault) -> ExpertData:
    """The decision states of a PlanPlay that kept its records: records0 [N, W] int32 is the record
    of the observation the first action was chosen from.  Pure torch."""
    if play.records is None:
        raise ValueError("expert_data: the play has no records (plan_play(records=True))")
    H, N = play.actions.shape
    rec = torch.cat([torch.as_tensor(records0, device=play.records.device).reshape(1, N, -1), play.records[:H - 1]], 0)
    k = torch.arange(H, device=play.length.device).reshape(H, 1)
    valid = k < play.length.reshape(1, N).to(torch.int64)
    return ExpertData(rec, play.expert, play.value, play.actions, valid, play.length, torch.as_tensor(grid),
                      int(rows), int(cols), (int(vault[0]), int(vault[1])))


def expert_rollout(env, gamma: float = 1.0, horizon: Optional[int] = None, noise: float = 0.0, seed: int = 0,
                   records0: Optional[torch.Tensor] = None) -> ExpertData:
    """Exactly labelled decision states of every env of a HeistEnv as it stands: one
    plan_value(all_ticks=True) launch and one plan_play launch of its tables, the play perturbed
    with probability noise per step (states off the optimal path, still labelled by the exact
    table).  records0 [N, W] is the record of each env's current observation; it defaults to
    env.pack_obs(env.obs), so env.obs must be current -- it is after reset or step, not after
    step_multi, load_state or fork_state.  Reads the envs only."""
    pv = env.plan_value(horizon=horizon, gamma=gamma, all_ticks=True)
    play = env.plan_play(pv.action_ticks, pv.vis, values=pv.value_ticks, noise=noise, seed=seed)
    if records0 is None:
        records0 = env.pack_obs(env.obs)
    return expert_data(play, records0, pv.grid, env.rows, env.cols, env.config.vault_pos)


# -- emitter ablation (heist_plan_masked, HeistEnv.plan_masked / plan_ablate) -------------------

def ablation_masks(n_cams, n_guards, max_cams: int, max_guards: int) -> torch.Tensor:
    """The leave-one-out emitter masks of heist_plan_masked as int64 [N, 1 + n_slot], n_slot =
    max_cams + max_guards: variant 0 has the bit of every filled slot set (camera j < n_cams[e] is
    slot j, guard g < n_guards[e] is slot max_cams + g), variant 1 + j is variant 0 without slot
    j's bit -- equal to variant 0 where the env does not fill slot j.  Slot 63 is the int64's sign
    bit (the kernel reads the word as uint64).  Pure torch, on the device of n_cams."""
    n_cams = torch.as_tensor(n_cams).reshape(-1).to(torch.int64)
    n_guards = torch.as_tensor(n_guards, device=n_cams.device).reshape(-1).to(torch.int64)
    n_slot = int(max_cams) + int(max_guards)
    if max_cams < 0 or max_guards < 0 or not 1 <= n_slot <= 64:
        raise ValueError("ablation_masks: need 1 <= max_cams + max_guards <= 64")
    j = torch.arange(n_slot, dtype=torch.int64, device=n_cams.device).reshape(1, n_slot)
    filled = torch.where(j < max_cams, j < n_cams.reshape(-1, 1), j - max_cams < n_guards.reshape(-1, 1))
    bit = torch.ones_like(j) << j                                  # [1, n_slot]; 1 << 63 wraps to the sign bit
    own = torch.where(filled, bit, torch.zeros_like(bit))          # [N, n_slot], disjoint bits
    full = own.sum(1, keepdim=True)                                # their OR (two's complement: exact)
    return torch.cat([full, full - own], 1)


@dataclass
class PlanAblation:
    """HeistEnv.plan_ablate's output: what every emitter of every layout costs the Solver, from the
    leave-one-out variants of heist_plan_masked (variant 0: the layout as built; variant 1 + j: slot
    j switched off; slots as in ablation_masks).  Tensors on the tables' device:
    ticks [N, 1 + n_slot] int16, value [N, 1 + n_slot] float64 -- PlanMasked.ticks / value;
    filled [N, n_slot] bool -- the env fills slot j;
    ticks_saved [N, n_slot] int16 -- ticks[:, :1] - ticks[:, 1:] where both are solvable, else 0;
    credit [N, n_slot] float64 -- value[:, 1:] - value[:, :1], one subtraction: what the emitter
        costs the Solver's optimal return; 0.0 for an unfilled slot.  Non-negative on every batch
        measured, but nothing here assumes it: a detection ends the episode, so where playing on
        is worth less than the detection's penalty, an emitter's removal can lower the value;
    critical [N, n_slot] bool -- the full layout has no undetected way to the vault, the layout
        without slot j has one;
    redundant [N, n_slot] bool -- a filled slot without which neither the ticks nor the value's
        bits change."""
    ticks: torch.Tensor
    value: torch.Tensor
    filled: torch.Tensor
    ticks_saved: torch.Tensor
    credit: torch.Tensor
    critical: torch.Tensor
    redundant: torch.Tensor

    @staticmethod
    def from_tables(ticks: torch.Tensor, value: torch.Tensor, filled: torch.Tensor) -> "PlanAblation":
        """The derived fields from the leave-one-out tables.  Pure torch."""
        n_slot = filled.shape[1]
        if ticks.shape != (filled.shape[0], 1 + n_slot) or value.shape != ticks.shape:
            raise ValueError("PlanAblation: ticks and value must be [N, 1 + n_slot] for filled [N, n_slot]")
        filled = filled.bool()
        t0, t1 = ticks[:, :1], ticks[:, 1:]
        v0, v1 = value[:, :1].contiguous(), value[:, 1:].contiguous()
        both = (t0 > 0) & (t1 > 0)
        saved = torch.where(both, t0 - t1, torch.zeros_like(t1))
        same = (t1 == t0) & (v1.view(torch.int64) == v0.view(torch.int64))
        return PlanAblation(ticks, value, filled, saved, v1 - v0, filled & (t0 < 0) & (t1 > 0), filled & same)

    def metrics(self, max_cams: int) -> dict:
        """The trainer's four figures for this batch (AdversarialTrainer(track_emitter_credit=True)):
        critical_layout_frac -- the share of the unsolvable layouts that one emitter's removal makes
        solvable; redundant_emitter_frac -- the share of the filled emitters that are redundant;
        camera_credit_mean / guard_credit_mean -- the mean credit over the filled cameras / guards
        (slots below / from max_cams).  A share or a mean over nothing is 0.0."""
        f = self.filled
        unsolv = self.ticks[:, 0] < 0
        cam = torch.zeros_like(f)
        cam[:, :max_cams] = True
        z = torch.zeros_like(self.credit)
        s = torch.stack([unsolv.sum().double(), (unsolv & self.critical.any(1)).sum().double(),
                         f.sum().double(), self.redundant.sum().double(),
                         (f & cam).sum().double(), torch.where(f & cam, self.credit, z).sum(),
                         (f & ~cam).sum().double(), torch.where(f & ~cam, self.credit, z).sum()]).cpu().tolist()
        div = lambda a, b: a / b if b else 0.0  # noqa: E731
        return {"critical_layout_frac": div(s[1], s[0]), "redundant_emitter_frac": div(s[3], s[2]),
                "camera_credit_mean": div(s[5], s[4]), "guard_credit_mean": div(s[7], s[6])}


# -- camera placement (heist_plan_place, HeistEnv.plan_place) -----------------------------------

def camera_candidates(grid, headings, fov: float, speed: float, vision_range) -> torch.Tensor:
    """One candidate camera per interior cell and heading, for every env of grid [N, R, C] int8
    (HeistEnv.grid_snapshot() or a CPU tensor), as heist_plan_place's cand rows float64
    [N, M, 6] = (row, col, fov, heading, speed, vision_range), M = (R - 2)(C - 2) len(headings):
    cells in row-major order, headings innermost, candidate ((r - 1)(C - 2) + c - 1) len(headings) +
    h stands on (r, c) with headings[h].  Every interior cell is listed whatever stands on it --
    the kernel's `valid` says which are placeable -- so M and the order are the same for every
    env.  Pure torch, on the device of grid."""
    grid = torch.as_tensor(grid)
    if grid.dim() != 3 or grid.shape[1] < 3 or grid.shape[2] < 3:
        raise ValueError("camera_candidates: grid must be [N, R, C] with R, C >= 3")
    n, R, C = (int(v) for v in grid.shape)
    dev = grid.device
    hd = torch.as_tensor(headings, dtype=torch.float64, device=dev).reshape(-1)
    nh = int(hd.numel())
    if nh < 1:
        raise ValueError("camera_candidates: need at least one heading")
    r = torch.arange(1, R - 1, dtype=torch.float64, device=dev).reshape(-1, 1, 1).expand(R - 2, C - 2, nh)
    c = torch.arange(1, C - 1, dtype=torch.float64, device=dev).reshape(1, -1, 1).expand(R - 2, C - 2, nh)
    h = hd.reshape(1, 1, nh).expand(R - 2, C - 2, nh)
    one = torch.ones_like(r)
    rows = torch.stack([r, c, one * float(fov), h, one * float(speed), one * float(vision_range)], -1)
    return rows.reshape(1, -1, 6).expand(n, -1, -1).contiguous()


@dataclass
class PlacementScan:
    """placement_scan's output: what every candidate camera would do to every env, without the
    visibility rows.  Tensors on the tables' device:
    valid [N, M] bool, ticks [N, M] int16, value [N, M] float64, action [N, M] int8 -- PlanPlace's;
    ticks0 [N] int16, value0 [N] float64 -- the baseline: the plan of the base rows alone;
    cands [N, M, 6] float64 -- the candidates as given (a guard_placement_scan's: the tuple of
    paths, meta and fov)."""
    valid: torch.Tensor
    ticks: torch.Tensor
    value: torch.Tensor
    action: torch.Tensor
    ticks0: torch.Tensor
    value0: torch.Tensor
    cands: Optional[object] = None

    def eligible(self) -> torch.Tensor:
        """[N, M] bool: the valid candidates that leave an undetected way to the vault (ticks >= 0).
        One more camera never opens a way, so an env whose baseline has none has no eligible
        candidate."""
        return self.valid.bool() & (self.ticks >= 0)

    def best(self) -> torch.Tensor:
        """[N] int64: per env the eligible candidate of lowest Solver value -- the hardest camera
        that keeps a solvable layout solvable -- the lowest index on ties, -1 where there is none."""
        ok = self.eligible()
        inf = torch.full_like(self.value, float("inf"))
        v = torch.where(ok, self.value, inf)
        low = v.min(1, keepdim=True).values
        m = self.value.shape[1]
        idx = torch.arange(m, device=v.device, dtype=torch.int64).reshape(1, m).expand_as(v)
        first = torch.where(ok & (v == low), idx, torch.full_like(idx, m)).min(1).values
        return torch.where(first < m, first, torch.full_like(first, -1))

    def headroom(self) -> torch.Tensor:
        """[N] float64: value0 - value[best], one subtraction: the optimal return the best camera
        would still take from the Solver; 0.0 where there is no best candidate.  Negative where
        even the hardest candidate raises the value (PlanAblation.credit's note applies)."""
        b = self.best()
        vb = self.value.gather(1, b.clamp(min=0).reshape(-1, 1)).reshape(-1)
        return torch.where(b >= 0, self.value0 - vb, torch.zeros_like(self.value0))

    def blocking(self) -> torch.Tensor:
        """[N] float64: per env the share of its valid candidates that turn a solvable layout
        unsolvable (ticks0 >= 0, the variant's ticks < 0); 0.0 for an env whose baseline is
        unsolvable or that has no valid candidate."""
        va = self.valid.bool()
        blk = (va & (self.ticks < 0) & (self.ticks0 >= 0).reshape(-1, 1)).sum(1).double()
        nv = va.sum(1).double()
        return torch.where(nv > 0, blk / nv.clamp(min=1.0), torch.zeros_like(nv))

    def metrics(self, kind: str = "camera") -> dict:
        """The trainer's three figures for this scan (AdversarialTrainer(track_camera_headroom=True)):
        camera_headroom_envs -- the envs that have a best candidate; camera_headroom_mean -- the
        mean headroom over them; camera_blocking_frac -- the mean of blocking() over the envs whose
        baseline is solvable.  A mean over nothing is 0.0.  kind: the keys' prefix ("guard" for a
        guard_placement_scan, track_guard_headroom's figures)."""
        has = self.best() >= 0
        solv = self.ticks0 >= 0
        z = torch.zeros_like(self.value0)
        s = torch.stack([has.sum().double(), torch.where(has, self.headroom(), z).sum(), solv.sum().double(),
                         torch.where(solv, self.blocking(), z).sum()]).cpu().tolist()
        div = lambda a, b: a / b if b else 0.0  # noqa: E731
        return {kind + "_headroom_mean": div(s[1], s[0]), kind + "_blocking_frac": div(s[3], s[2]),
                kind + "_headroom_envs": int(s[0])}


def placement_scan(env, cands, horizon: Optional[int] = None, gamma: float = 1.0, base: Optional[torch.Tensor] = None,
                   max_bytes: int = 1 << 30) -> PlacementScan:
    """Every candidate camera of cands (float64 [N, M, 6] or [M, 6], camera_candidates' rows) tried
    on every env of a HeistEnv as it stands: HeistEnv.plan_place in chunks of M sized so that a
    chunk's visibility rows (4 H N m W bytes) stay under max_bytes, the rows dropped, the tables
    concatenated.  base: the rows the candidates are added to (plan_place's base; None: one
    plan_field launch supplies them).  The baseline ticks0 / value0 is the plan of those rows
    alone, which is what plan_place gives for a candidate that is not valid (a row of NaNs): with
    plan_field's rows it is plan_field's togo and plan_value's value at the Solver's cell.  Reads
    the envs only."""
    from .obs_compact import record_words
    H = min(int(env.config.max_steps), 1024) if horizon is None else int(horizon)
    cd = torch.as_tensor(cands)
    if cd.dim() == 2:
        cd = cd.unsqueeze(0).expand(env.n_envs, -1, -1)
    cd = cd.to(env.device)
    M = int(cd.shape[1])
    if base is None:
        base = env.plan_field(horizon=H).vis
    per = 4 * max(H, 1) * env.n_envs * record_words(env.rows, env.cols)
    step = max(1, int(max_bytes) // per)
    nan = torch.full((1, 6), float("nan"), dtype=torch.float64, device=env.device)
    p0 = env.plan_place(nan, horizon=H, gamma=gamma, base=base)
    parts = []
    for m0 in range(0, M, step):
        pp = env.plan_place(cd[:, m0:m0 + step], horizon=H, gamma=gamma, base=base)
        parts.append((pp.valid, pp.ticks, pp.value, pp.action))
        del pp
    valid, ticks, value, action = (torch.cat(x, 1) for x in zip(*parts))
    return PlacementScan(valid, ticks, value, action, p0.ticks[:, 0], p0.value[:, 0], cd)


@dataclass
class RelocationScan:
    """relocation_scan's output: scan -- the PlacementScan of the slot's camera on every interior
    cell, over the layout without that camera (its baseline ticks0 / value0 is the layout without
    the camera); ticks_built [N] int16, value_built [N] float64 -- the layout as built;
    rank [N] int64 -- how many valid candidates give the Solver a strictly lower value than the
    layout as built: 0 says the Architect's tile is optimal for this camera (-1: the env does not
    fill the slot)."""
    scan: PlacementScan
    ticks_built: torch.Tensor
    value_built: torch.Tensor
    rank: torch.Tensor


def relocation_scan(env, slot: int, headings=None, horizon: Optional[int] = None, gamma: float = 1.0,
                    max_bytes: int = 1 << 30) -> RelocationScan:
    """Where else could camera `slot` of every env have stood?  One plan_masked launch plans every
    env as built and without the camera; its second variant's rows are the base of a
    placement_scan whose candidates carry the camera's own fov, speed and range
    (HeistEnv.camera_records) on every interior cell, with the heading it has now or, given
    headings, each of those.  Reads the envs only."""
    slot = int(slot)
    if not 0 <= slot < env.max_cams:
        raise ValueError("relocation_scan: slot must be a camera slot, 0 .. %d" % (env.max_cams - 1))
    ex = env.export()
    masks = ablation_masks(ex["n_cams"], ex["n_guards"], env.max_cams, env.max_guards)[:, [0, 1 + slot]].contiguous()
    pm = env.plan_masked(masks, horizon=horizon, gamma=gamma)
    rec = env.camera_records()[:, slot]                                   # [N, 6]
    cd = camera_candidates(env.grid_snapshot(), [0.0] if headings is None else headings, 0.0, 0.0, 0.0)
    own = rec.reshape(-1, 1, 6).expand(-1, cd.shape[1], -1)
    cd[:, :, 2] = own[:, :, 2]
    cd[:, :, 4:] = own[:, :, 4:]
    if headings is None:
        cd[:, :, 3] = own[:, :, 3]
    scan = placement_scan(env, cd, horizon=horizon, gamma=gamma, base=pm.vis[:, :, 1].contiguous(), max_bytes=max_bytes)
    filled = ex["n_cams"] > slot
    lower = (scan.valid & (scan.value < pm.value[:, :1])).sum(1)
    return RelocationScan(scan, pm.ticks[:, 0], pm.value[:, 0], torch.where(filled, lower, torch.full_like(lower, -1)))


def greedy_cameras(env, n: int, headings, fov: float, speed: float, vision_range, horizon: Optional[int] = None,
                   gamma: float = 1.0, max_bytes: int = 1 << 30):
    """The exact greedy adversary, camera by camera: n rounds of placement_scan over every interior
    cell x headings -> PlacementScan.best() -> that camera appended to the env's layout ->
    set_layouts + reset.  The envs must be fresh from set_layout + reset (tick 0): a round's
    prediction is the value of the rebuilt layout's first attempt.  The layouts are read back from
    the handle (HeistEnv.layout_lists) and rebuilt with a budget of what they spent plus 3 per
    camera added; an env stops when its camera slots are full or no candidate is eligible.
    Returns (cameras, predicted): cameras[r] the round's choice per env as float64 [N, 6] rows
    (NaN where the env added none), predicted[r] float64 [N] the Solver's optimal value the scan
    predicted for the rebuilt layout (the env's current value where it added none).  Changes the
    envs' layouts."""
    cams_out, pred_out = [], []
    for _ in range(int(n)):
        layouts, spent = env.layout_lists()
        cd = camera_candidates(env.grid_snapshot(), headings, fov, speed, vision_range)
        scan = placement_scan(env, cd, horizon=horizon, gamma=gamma, max_bytes=max_bytes)
        best = scan.best()
        room = torch.as_tensor([len(l[1]) < env.max_cams for l in layouts], device=best.device)
        best = torch.where(room, best, torch.full_like(best, -1))
        chosen = cd.gather(1, best.clamp(min=0).reshape(-1, 1, 1).expand(-1, 1, 6)).reshape(-1, 6)
        chosen = torch.where((best >= 0).reshape(-1, 1), chosen, torch.full_like(chosen, float("nan")))
        vb = scan.value.gather(1, best.clamp(min=0).reshape(-1, 1)).reshape(-1)
        pred_out.append(torch.where(best >= 0, vb, scan.value0))
        cams_out.append(chosen)
        budget = []
        for e, row in enumerate(chosen.cpu().tolist()):
            walls, cams, guards = layouts[e]
            add = row[0] == row[0]
            if add:
                cams = list(cams) + [{"row": int(row[0]), "col": int(row[1]), "fov_angle": row[2], "heading": row[3],
                                      "rotation_speed": row[4], "vision_range": int(row[5])}]
            layouts[e] = (walls, cams, guards)
            budget.append(int(spent[e]) + (3 if add else 0))
        env.set_layouts(layouts, budget=budget)
        env.reset()
    return cams_out, pred_out


# -- guard placement (heist_plan_place_guard, HeistEnv.plan_place_guard) --------------------------

CAMERA_COST, GUARD_COST = 3, 5   # the Architect's cost table (BUDGET_COSTS; heist_set_layout's purchase)
_PATROL_OFFS = ((0, 0), (0, 1), (0, 2), (1, 2), (2, 2), (2, 1), (2, 0), (1, 0))


def architect_patrol(r: int, c: int, R: int, C: int):
    """The 8-point rectangle patrol the Architect's decode gives a guard on tile (r, c) of an R x C
    grid (arch_decode_kernel, networks.py:324-335): the ring of the 3 x 3 block centred on (r, c),
    clockwise from its top-left tile, every point clamped to the interior.  A list of 8 (row, col)."""
    return [(max(1, min(R - 2, r + dr - 1)), max(1, min(C - 2, c + dc - 1))) for dr, dc in _PATROL_OFFS]


def guard_candidates(grid, speed: int = 1, vision_range: int = 4, fov: float = 90.0):
    """The Architect's guard (architect_patrol's path, speed 1, range 4, fov 90 by default) on every
    interior tile, for every env of grid [N, R, C] int8, as heist_plan_place_guard's three arrays:
    (paths int32 [N, M, 8, 2], meta int32 [N, M, 4] = (len, speed, vision_range, idx 0), fov
    float64 [N, M, 2] = (fov_angle, heading 0.0)), M = (R - 2)(C - 2), tiles in row-major order, so
    M and the order are the same for every env.  A tile whose patrol start is not EMPTY in env e
    carries no candidate there: its len is 0, which the kernel reports as not valid.  Pure torch, on
    the device of grid."""
    grid = torch.as_tensor(grid)
    if grid.dim() != 3 or grid.shape[1] < 3 or grid.shape[2] < 3:
        raise ValueError("guard_candidates: grid must be [N, R, C] with R, C >= 3")
    n, R, C = (int(v) for v in grid.shape)
    dev = grid.device
    pts = torch.tensor([architect_patrol(r, c, R, C) for r in range(1, R - 1) for c in range(1, C - 1)],
                       dtype=torch.int32, device=dev)                                   # [M, 8, 2]
    M = int(pts.shape[0])
    start = grid[:, pts[:, 0, 0].long(), pts[:, 0, 1].long()]                            # [N, M] the start tiles
    meta = torch.zeros((n, M, 4), dtype=torch.int32, device=dev)
    meta[:, :, 0] = torch.where(start == 0, 8, 0).to(torch.int32)
    meta[:, :, 1] = int(speed)
    meta[:, :, 2] = int(vision_range)
    fv = torch.zeros((n, M, 2), dtype=torch.float64, device=dev)
    fv[:, :, 0] = float(fov)
    return pts.unsqueeze(0).expand(n, -1, -1, -1).contiguous(), meta, fv


def guard_placement_scan(env, cands, horizon: Optional[int] = None, gamma: float = 1.0,
                         base: Optional[torch.Tensor] = None, max_bytes: int = 1 << 30) -> PlacementScan:
    """placement_scan for guards: every candidate of cands = (paths, meta, fov) (guard_candidates'
    arrays, [N, M, ...] or [M, ...]) tried on every env of a HeistEnv as it stands, with
    HeistEnv.plan_place_guard in the same chunks of M, the rows dropped, the tables concatenated.
    The baseline ticks0 / value0 is the plan of the base rows alone (a candidate of len 0).
    PlacementScan's best() / headroom() / blocking() / metrics("guard") read the result.  Reads the
    envs only."""
    from .obs_compact import record_words
    H = min(int(env.config.max_steps), 1024) if horizon is None else int(horizon)
    pa, me, fv = (x.to(env.device) for x in env._guard_candidates_arg(*cands))
    M = int(pa.shape[1])
    if base is None:
        base = env.plan_field(horizon=H).vis
    per = 4 * max(H, 1) * env.n_envs * record_words(env.rows, env.cols)
    step = max(1, int(max_bytes) // per)
    none = (torch.zeros((1, 1, 2), dtype=torch.int32), torch.zeros((1, 4), dtype=torch.int32),
            torch.zeros((1, 2), dtype=torch.float64))
    p0 = env.plan_place_guard(*none, horizon=H, gamma=gamma, base=base)
    parts = []
    for m0 in range(0, M, step):
        pp = env.plan_place_guard(pa[:, m0:m0 + step], me[:, m0:m0 + step], fv[:, m0:m0 + step], horizon=H,
                                  gamma=gamma, base=base)
        parts.append((pp.valid, pp.ticks, pp.value, pp.action))
        del pp
    valid, ticks, value, action = (torch.cat(x, 1) for x in zip(*parts))
    return PlacementScan(valid, ticks, value, action, p0.ticks[:, 0], p0.value[:, 0], (pa, me, fv))


def greedy_pick(cam_scan: Optional[PlacementScan], guard_scan: Optional[PlacementScan], remaining,
                cam_ok: Optional[torch.Tensor] = None, guard_ok: Optional[torch.Tensor] = None):
    """greedy_adversary's selection rule on two scans of the same envs over the same base rows.  Per
    env, among the candidates that are eligible (valid, the layout stays solvable), affordable (3
    points for a camera, 5 for a guard, against remaining [N]) and not masked out (cam_ok [N, Mc],
    guard_ok [N, Mg] bool), the one that takes the most optimal return per budget point, gain =
    (value0 - value) / cost in float64; only a gain above 0 counts.  Ties go to the camera, then to
    the lowest index.  Returns (kind [N] int64: 0 camera, 1 guard, -1 none; index [N] int64, -1 for
    none; gain [N] float64, 0.0 for none)."""
    ref = cam_scan if cam_scan is not None else guard_scan
    dev = ref.value0.device
    remaining = torch.as_tensor(remaining, dtype=torch.int64, device=dev).reshape(-1)
    n = int(ref.value0.shape[0])
    best_gain = torch.zeros(n, dtype=torch.float64, device=dev)
    kind = torch.full((n,), -1, dtype=torch.int64, device=dev)
    index = torch.full((n,), -1, dtype=torch.int64, device=dev)
    for k, (sc, cost, ok) in enumerate(((cam_scan, CAMERA_COST, cam_ok), (guard_scan, GUARD_COST, guard_ok))):
        if sc is None or sc.value.shape[1] == 0:
            continue
        el = sc.eligible() & (remaining >= cost).reshape(-1, 1)
        if ok is not None:
            el = el & ok.to(dev)
        # a tensor divisor: one IEEE division on every device (a scalar divisor is multiplied by its reciprocal on the GPU)
        gain = (sc.value0.reshape(-1, 1) - sc.value) / torch.full_like(sc.value, float(cost))
        gain = torch.where(el, gain, torch.full_like(gain, -float("inf")))
        top, arg = gain.max(1)  # the first maximum is not promised by max: take the lowest index by hand
        m = gain.shape[1]
        idx = torch.arange(m, device=dev, dtype=torch.int64).reshape(1, m).expand_as(gain)
        arg = torch.where(gain == top.reshape(-1, 1), idx, torch.full_like(idx, m)).min(1).values
        take = top > best_gain  # strictly: an equal guard does not displace a camera
        best_gain = torch.where(take, top, best_gain)
        kind = torch.where(take, torch.full_like(kind, k), kind)
        index = torch.where(take, arg, index)
    return kind, index, best_gain


@dataclass
class GreedyAdversary:
    """greedy_adversary's output.  Per round r (lists, one entry per round that some env still
    bought in): kind[r] [N] int64 (0 camera, 1 guard, -1 the env bought nothing), index[r] [N]
    int64 into that kind's candidates, value[r] [N] float64 -- the Solver's optimal return the scan
    predicts for the layout with everything bought so far, ticks[r] [N] int16 likewise.
    cameras[e], guards[e]: what env e bought, in order, as heist_set_layout dicts -- appended to the
    env's own lists (HeistEnv.layout_lists) they rebuild the adversary's layout at budget spent0[e]
    + spent[e].  spent [N] int64: the points used.  vis [H, N, W] int32: the final layout's
    visibility rows."""
    kind: list
    index: list
    value: list
    ticks: list
    cameras: list
    guards: list
    spent: torch.Tensor
    vis: torch.Tensor


def greedy_adversary(env, budget, camera_cands=None, guard_cands=None, horizon: Optional[int] = None,
                     gamma: float = 1.0, max_rounds: int = 64, max_bytes: int = 1 << 30) -> GreedyAdversary:
    """The exact greedy adversary under the game's cost table (camera 3, guard 5), without rebuilding
    a layout: each round scans camera_cands (camera_candidates' rows or None) and guard_cands
    (guard_candidates' arrays or None) over the current base rows, takes greedy_pick's choice per env
    within what is left of budget (an int or [N]), and the chosen variant's visibility rows become
    the next round's base (one plan_place and one plan_place_guard launch at M = 1).  A candidate on
    a tile an earlier choice took -- a camera's tile, a guard's start tile -- is no longer offered.
    The envs should be fresh from set_layout + reset, so that the prediction is the value of the
    rebuilt layout's first attempt.  Stops when no env buys, or after max_rounds.  Reads the envs
    only."""
    dev, n = env.device, env.n_envs
    H = min(int(env.config.max_steps), 1024) if horizon is None else int(horizon)
    left = torch.as_tensor(budget, dtype=torch.int64, device=dev).reshape(-1).expand(n).clone()
    cd = None
    if camera_cands is not None:
        cd = torch.as_tensor(camera_cands)
        cd = (cd.unsqueeze(0).expand(n, -1, -1) if cd.dim() == 2 else cd).to(dev).contiguous()
    ga = None
    if guard_cands is not None:
        ga = tuple(x.to(dev).contiguous() for x in env._guard_candidates_arg(*guard_cands))
    if cd is None and ga is None:
        raise ValueError("greedy_adversary: need camera_cands or guard_cands")
    taken = torch.zeros((n, env.rows, env.cols), dtype=torch.bool, device=dev)
    ar = torch.arange(n, device=dev)

    def free(r, c):  # [N, M] bool: the candidate's tile is not taken (tiles outside the grid: the kernel rejects them)
        inside = (r >= 0) & (r < env.rows) & (c >= 0) & (c < env.cols)
        return ~(taken[ar.reshape(-1, 1), r.clamp(0, env.rows - 1), c.clamp(0, env.cols - 1)] & inside)

    base = env.plan_field(horizon=H).vis
    out = GreedyAdversary([], [], [], [], [[] for _ in range(n)], [[] for _ in range(n)],
                          torch.zeros(n, dtype=torch.int64, device=dev), base)
    for _ in range(int(max_rounds)):
        cs = gs = c_ok = g_ok = None
        if cd is not None:
            cs = placement_scan(env, cd, horizon=H, gamma=gamma, base=base, max_bytes=max_bytes)
            fin = torch.isfinite(cd[:, :, 0]) & torch.isfinite(cd[:, :, 1]) & (cd[:, :, :2].abs() < 2.0 ** 31).all(-1)
            rc = torch.where(fin.unsqueeze(-1), cd[:, :, :2], torch.full_like(cd[:, :, :2], -1.0)).long()
            c_ok = free(rc[..., 0], rc[..., 1])
        if ga is not None:
            gs = guard_placement_scan(env, ga, horizon=H, gamma=gamma, base=base, max_bytes=max_bytes)
            g_ok = free(ga[0][:, :, 0, 0].long(), ga[0][:, :, 0, 1].long())
        kind, index, _ = greedy_pick(cs, gs, left, c_ok, g_ok)
        if not bool((kind >= 0).any()):
            break
        ref = cs if cs is not None else gs
        value, ticks = ref.value0.clone(), ref.ticks0.clone()
        if cd is not None:
            is_c = kind == 0
            i1 = torch.where(is_c, index, torch.zeros_like(index))  # an index into the cameras only where one was chosen
            row = cd.gather(1, i1.reshape(-1, 1, 1).expand(-1, 1, 6))
            row = torch.where(is_c.reshape(-1, 1, 1), row, torch.full_like(row, float("nan")))
            pp = env.plan_place(row, horizon=H, gamma=gamma, base=base)
            base = pp.vis[:, :, 0].contiguous()
            value, ticks = torch.where(is_c, pp.value[:, 0], value), torch.where(is_c, pp.ticks[:, 0], ticks)
            for e in torch.nonzero(is_c).reshape(-1).tolist():
                v = row[e, 0].tolist()
                out.cameras[e].append({"row": int(v[0]), "col": int(v[1]), "fov_angle": v[2], "heading": v[3],
                                       "rotation_speed": v[4], "vision_range": int(v[5])})
                taken[e, int(v[0]), int(v[1])] = True
        if ga is not None:
            is_g = kind == 1
            i1 = torch.where(is_g, index, torch.zeros_like(index))  # likewise: a camera's index can lie past the guards
            P = ga[0].shape[2]
            pa = ga[0].gather(1, i1.reshape(-1, 1, 1, 1).expand(-1, 1, P, 2))
            me = ga[1].gather(1, i1.reshape(-1, 1, 1).expand(-1, 1, 4)).clone()
            fv = ga[2].gather(1, i1.reshape(-1, 1, 1).expand(-1, 1, 2))
            me[:, :, 0] = torch.where(is_g.reshape(-1, 1), me[:, :, 0], torch.zeros_like(me[:, :, 0]))
            pp = env.plan_place_guard(pa, me, fv, horizon=H, gamma=gamma, base=base)
            base = pp.vis[:, :, 0].contiguous()
            value, ticks = torch.where(is_g, pp.value[:, 0], value), torch.where(is_g, pp.ticks[:, 0], ticks)
            for e in torch.nonzero(is_g).reshape(-1).tolist():
                ln = int(me[e, 0, 0])
                pts = [(int(r), int(c)) for r, c in pa[e, 0, :ln].tolist()]
                out.guards[e].append({"patrol_path": pts, "speed": int(me[e, 0, 1]), "vision_range": int(me[e, 0, 2]),
                                      "fov_angle": float(fv[e, 0, 0])})
                taken[e, pts[0][0], pts[0][1]] = True
        cost = torch.where(kind == 0, CAMERA_COST, torch.where(kind == 1, GUARD_COST, 0)).to(torch.int64)
        left -= cost
        out.spent += cost
        out.kind.append(kind)
        out.index.append(index)
        out.value.append(value)
        out.ticks.append(ticks)
        out.vis = base
    return out


# -- walls (heist_plan_walls, HeistEnv.plan_walls / plan_wall_ablate) -----------------------------

_EMPTY, _WALL = 0, 1  # tile codes (utils.py)
MAX_WALL_EDITS = 8    # heist_plan_walls: 1 <= E <= 8
WALL_COST = 1         # the Architect's cost table (BUDGET_COSTS; heist_set_layout's purchase)


def wall_ablation_edits(grid, max_walls: int):
    """The leave-one-out wall edits of heist_plan_walls for grid [N, R, C] (a tensor or an array of any
    integer type; HeistEnv.export()["grid"]), as (edits int32 [N, 1 + max_walls, 1, 3], filled bool
    [N, max_walls]): variant 0 is the layout as built (op 0), variant 1 + j removes the env's j-th
    interior WALL tile in row-major order (row, col, 2), and beyond the env's count -- filled False
    -- the variant is op 0 again, equal to variant 0.  Walls past max_walls are left out.  The border
    is not listed: it cannot be removed.  Pure torch, on the device of grid."""
    grid = torch.as_tensor(grid)
    if grid.dim() != 3 or grid.shape[1] < 3 or grid.shape[2] < 3:
        raise ValueError("wall_ablation_edits: grid must be [N, R, C] with R, C >= 3")
    k = int(max_walls)
    if k < 0:
        raise ValueError("wall_ablation_edits: max_walls must be >= 0")
    n, R, C = (int(v) for v in grid.shape)
    dev = grid.device
    w = (grid[:, 1:-1, 1:-1] == _WALL).reshape(n, -1)                    # [N, cells], row-major
    cells = int(w.shape[1])
    order = torch.argsort((~w).to(torch.int8), dim=1, stable=True)       # the wall cells first, in order
    if k > cells:
        order = torch.cat([order, torch.zeros((n, k - cells), dtype=order.dtype, device=dev)], 1)
    cell = order[:, :k]
    filled = torch.arange(k, device=dev).reshape(1, k) < w.sum(1, keepdim=True)
    z = torch.zeros_like(cell)
    row = torch.where(filled, torch.div(cell, C - 2, rounding_mode="floor") + 1, z)
    col = torch.where(filled, cell % (C - 2) + 1, z)
    op = torch.where(filled, torch.full_like(cell, 2), z)
    ed = torch.stack([row, col, op], -1).to(torch.int32)                 # [N, k, 3]
    ed = torch.cat([torch.zeros((n, 1, 3), dtype=torch.int32, device=dev), ed], 1)
    return ed.reshape(n, 1 + k, 1, 3).contiguous(), filled


@dataclass
class WallAblation:
    """HeistEnv.plan_wall_ablate's output: what every interior wall of every layout does to the Solver,
    from the leave-one-out variants of heist_plan_walls (variant 0: the layout as built; variant
    1 + j: wall j removed; walls as in wall_ablation_edits).  PlanAblation's twin, with one more
    flag: a wall stops rays as well as moves, so its removal can hurt.  Tensors on the tables' device:
    ticks [N, 1 + K] int16, value [N, 1 + K] float64 -- PlanWalls.ticks / value;
    filled [N, K] bool -- the env has a wall j;
    ticks_saved [N, K] int16 -- ticks[:, :1] - ticks[:, 1:] where both are solvable, else 0 (negative
        where the way without the wall is longer);
    credit [N, K] float64 -- value[:, 1:] - value[:, :1], one subtraction, signed: what the wall costs
        the Solver's optimal return; 0.0 where there is no wall j;
    critical [N, K] bool -- the layout as built has no undetected way to the vault, the layout
        without wall j has one;
    redundant [N, K] bool -- a wall without which neither the ticks nor the value's bits change;
    shielding [N, K] bool -- credit < 0: the Solver does worse without the wall."""
    ticks: torch.Tensor
    value: torch.Tensor
    filled: torch.Tensor
    ticks_saved: torch.Tensor
    credit: torch.Tensor
    critical: torch.Tensor
    redundant: torch.Tensor
    shielding: torch.Tensor

    @staticmethod
    def from_tables(ticks: torch.Tensor, value: torch.Tensor, filled: torch.Tensor) -> "WallAblation":
        """The derived fields from the leave-one-out tables.  Pure torch."""
        k = filled.shape[1]
        if ticks.shape != (filled.shape[0], 1 + k) or value.shape != ticks.shape:
            raise ValueError("WallAblation: ticks and value must be [N, 1 + K] for filled [N, K]")
        filled = filled.bool()
        t0, t1 = ticks[:, :1], ticks[:, 1:]
        v0, v1 = value[:, :1].contiguous(), value[:, 1:].contiguous()
        both = (t0 > 0) & (t1 > 0)
        saved = torch.where(both, t0 - t1, torch.zeros_like(t1))
        same = (t1 == t0) & (v1.view(torch.int64) == v0.view(torch.int64))
        credit = torch.where(filled, v1 - v0, torch.zeros_like(v1))
        return WallAblation(ticks, value, filled, saved, credit, filled & (t0 < 0) & (t1 > 0), filled & same,
                            filled & (credit < 0))

    def metrics(self) -> dict:
        """The trainer's four figures for this batch (AdversarialTrainer(track_wall_credit=True)):
        critical_wall_layout_frac -- the share of the unsolvable layouts that one wall's removal makes
        solvable; redundant_wall_frac / shielding_wall_frac -- the share of the walls that are
        redundant / shielding; wall_credit_mean -- the mean credit over the walls.  A share or a mean
        over nothing is 0.0."""
        f = self.filled
        unsolv = self.ticks[:, 0] < 0
        s = torch.stack([unsolv.sum().double(), (unsolv & self.critical.any(1)).sum().double(), f.sum().double(),
                         self.redundant.sum().double(), self.shielding.sum().double(),
                         torch.where(f, self.credit, torch.zeros_like(self.credit)).sum().double()]).cpu().tolist()
        div = lambda a, b: a / b if b else 0.0  # noqa: E731
        return {"critical_wall_layout_frac": div(s[1], s[0]), "redundant_wall_frac": div(s[3], s[2]),
                "shielding_wall_frac": div(s[4], s[2]), "wall_credit_mean": div(s[5], s[2])}


def wall_candidates(grid) -> torch.Tensor:
    """One candidate wall per interior cell, for every env of grid [N, R, C], as heist_plan_walls'
    edits int32 [N, M, 1, 3] = (row, col, 1), M = (R - 2)(C - 2), cells in row-major order:
    candidate (r - 1)(C - 2) + c - 1 adds a wall on (r, c).  Every interior cell is listed whatever
    stands on it -- the kernel's `valid` says which are EMPTY and free of the Solver -- so M and the
    order are the same for every env.  Pure torch, on the device of grid."""
    grid = torch.as_tensor(grid)
    if grid.dim() != 3 or grid.shape[1] < 3 or grid.shape[2] < 3:
        raise ValueError("wall_candidates: grid must be [N, R, C] with R, C >= 3")
    n, R, C = (int(v) for v in grid.shape)
    dev = grid.device
    r = torch.arange(1, R - 1, dtype=torch.int32, device=dev).reshape(-1, 1).expand(R - 2, C - 2)
    c = torch.arange(1, C - 1, dtype=torch.int32, device=dev).reshape(1, -1).expand(R - 2, C - 2)
    rows = torch.stack([r, c, torch.ones_like(r)], -1)
    return rows.reshape(1, -1, 1, 3).expand(n, -1, -1, -1).contiguous()


@dataclass
class WallScan:
    """wall_placement_scan's output: what every candidate wall would do to every env, without the
    visibility rows.  Tensors on the tables' device:
    valid [N, M] bool, level [N, M] bool, ticks [N, M] int16, value [N, M] float64, action [N, M]
    int8 -- PlanWalls's; ticks0 [N] int16, value0 [N] float64 -- the baseline: the envs as they
    stand; cands [N, M, E, 3] int32 -- the candidates as given.
    Unlike one more camera, one more wall can raise the Solver's value, open no way but close the
    level, or cut the level off altogether: a wall that invalidates the level is not a buy (set_layout
    would reject the layout), so only candidates with valid & level count below."""
    valid: torch.Tensor
    level: torch.Tensor
    ticks: torch.Tensor
    value: torch.Tensor
    action: torch.Tensor
    ticks0: torch.Tensor
    value0: torch.Tensor
    cands: Optional[torch.Tensor] = None

    def eligible(self) -> torch.Tensor:
        """[N, M] bool: the valid candidates that keep the level valid."""
        return self.valid.bool() & self.level.bool()

    def best(self) -> torch.Tensor:
        """[N] int64: per env the eligible candidate of lowest Solver value, the lowest index on
        ties, -1 where there is none."""
        ok = self.eligible()
        v = torch.where(ok, self.value, torch.full_like(self.value, float("inf")))
        low = v.min(1, keepdim=True).values
        m = self.value.shape[1]
        idx = torch.arange(m, device=v.device, dtype=torch.int64).reshape(1, m).expand_as(v)
        first = torch.where(ok & (v == low), idx, torch.full_like(idx, m)).min(1).values
        return torch.where(first < m, first, torch.full_like(first, -1))

    def headroom(self) -> torch.Tensor:
        """[N] float64: value0 - value[best], one subtraction: the optimal return the best wall would
        still take from the Solver; 0.0 where there is no best candidate, negative where even the
        hardest wall helps."""
        b = self.best()
        vb = self.value.gather(1, b.clamp(min=0).reshape(-1, 1)).reshape(-1)
        return torch.where(b >= 0, self.value0 - vb, torch.zeros_like(self.value0))

    def _share(self, what: torch.Tensor, of: torch.Tensor) -> torch.Tensor:
        a, b = (what & of).sum(1).double(), of.sum(1).double()
        return torch.where(b > 0, a / b.clamp(min=1.0), torch.zeros_like(b))

    def helps(self) -> torch.Tensor:
        """[N] float64: per env the share of its eligible walls that raise the Solver's value (value >
        value0); 0.0 for an env without an eligible wall."""
        return self._share(self.value > self.value0.reshape(-1, 1), self.eligible())

    def blocking(self) -> torch.Tensor:
        """[N] float64: per env the share of its eligible walls that make a solvable layout unsolvable
        (ticks0 >= 0, the variant's ticks < 0) while the level stays valid; 0.0 for an env whose
        baseline is unsolvable or that has no eligible wall."""
        return self._share((self.ticks < 0) & (self.ticks0 >= 0).reshape(-1, 1), self.eligible())

    def invalidating(self) -> torch.Tensor:
        """[N] float64: per env the share of its valid candidates that cut the start off from the
        vault (level False); 0.0 for an env without a valid candidate."""
        return self._share(~self.level.bool(), self.valid.bool())

    def metrics(self) -> dict:
        """wall_headroom_envs -- the envs that have a best candidate; wall_headroom_mean -- the mean
        headroom over them; wall_helps_frac / wall_invalidating_frac -- the means of helps() /
        invalidating() over the envs; wall_blocking_frac -- the mean of blocking() over the envs
        whose baseline is solvable.  A mean over nothing is 0.0."""
        has = self.best() >= 0
        solv = self.ticks0 >= 0
        z = torch.zeros_like(self.value0)
        s = torch.stack([has.sum().double(), torch.where(has, self.headroom(), z).sum(), solv.sum().double(),
                         torch.where(solv, self.blocking(), z).sum(), self.helps().sum(),
                         self.invalidating().sum()]).cpu().tolist()
        n = int(self.value0.shape[0])
        div = lambda a, b: a / b if b else 0.0  # noqa: E731
        return {"wall_headroom_mean": div(s[1], s[0]), "wall_blocking_frac": div(s[3], s[2]),
                "wall_helps_frac": div(s[4], n), "wall_invalidating_frac": div(s[5], n),
                "wall_headroom_envs": int(s[0])}


def _plan_walls_chunked(env, ed, masks, H, gamma, max_bytes):
    """HeistEnv.plan_walls over edits [N, M, E, 3] in chunks of M whose visibility rows stay under
    max_bytes, the rows dropped: (valid, level, ticks, value, action), each [N, M]."""
    from .obs_compact import record_words
    per = 4 * max(H, 1) * env.n_envs * record_words(env.rows, env.cols)
    step = max(1, int(max_bytes) // per)
    parts = []
    for m0 in range(0, int(ed.shape[1]), step):
        mk = None if masks is None else masks[:, m0:m0 + step]
        pw = env.plan_walls(ed[:, m0:m0 + step], masks=mk, horizon=H, gamma=gamma)
        parts.append((pw.valid, pw.level, pw.ticks, pw.value, pw.action))
        del pw
    return tuple(torch.cat(x, 1) for x in zip(*parts))


def wall_placement_scan(env, cands, horizon: Optional[int] = None, gamma: float = 1.0, masks=None,
                        max_bytes: int = 1 << 30) -> WallScan:
    """Every candidate of cands (int32 [N, M, E, 3] or [N, M, 3], wall_candidates' rows) tried on
    every env of a HeistEnv as it stands: HeistEnv.plan_walls in chunks of M sized so that a chunk's
    visibility rows (4 H N m W bytes) stay under max_bytes, the rows dropped, the tables
    concatenated.  masks: plan_walls' emitter masks, int64 [N, M], or None.  The baseline ticks0 /
    value0 is the variant without an edit and with every slot live.  Reads the envs only."""
    H = min(int(env.config.max_steps), 1024) if horizon is None else int(horizon)
    ed = torch.as_tensor(cands)
    if ed.dim() == 3:
        ed = ed.unsqueeze(2)
    ed = ed.to(env.device)
    if masks is not None:
        masks = torch.as_tensor(masks).to(env.device)
        if masks.dim() == 1:
            masks = masks.reshape(1, -1).expand(env.n_envs, -1)
    p0 = env.plan_walls(torch.zeros((env.n_envs, 1, 1, 3), dtype=torch.int32, device=env.device), horizon=H, gamma=gamma)
    valid, level, ticks, value, action = _plan_walls_chunked(env, ed, masks, H, gamma, max_bytes)
    return WallScan(valid, level, ticks, value, action, p0.ticks[:, 0], p0.value[:, 0], ed)


@dataclass
class GreedyWalls:
    """greedy_walls' output, round by round (lists of [N] tensors): index -- the candidate each env
    chose (-1: none); value / ticks -- the Solver's optimal value and fewest ticks with the walls
    chosen so far; and edits int32 [N, rounds, 3] -- the walls as heist_plan_walls edits, (row, col,
    1), or op 0 where the env chose none that round; value0 / ticks0 [N] -- the envs as they stand."""
    index: list
    value: list
    ticks: list
    edits: torch.Tensor
    value0: torch.Tensor
    ticks0: torch.Tensor


def greedy_walls(env, n: int, cands=None, horizon: Optional[int] = None, gamma: float = 1.0,
                 max_bytes: int = 1 << 30) -> GreedyWalls:
    """The exact greedy wall adversary, without rebuilding a layout: n <= 8 rounds, round r planning
    "the walls chosen so far + candidate" as an (r + 1)-edit variant of heist_plan_walls for every
    candidate of cands (single edits int32 [N, M, 3] or [N, M, 1, 3]; None: wall_candidates of the
    envs' grids).  A candidate is eligible when its variant is valid, keeps the level valid and
    leaves an undetected way to the vault (valid & level & ticks >= 0) -- a tile chosen earlier
    names one tile twice and is not valid; each env takes the eligible candidate with the largest
    drop of the Solver's value, a drop above 0 only, the lowest index on ties.  Stops early when no
    env chooses.  Reads the envs only."""
    n = int(n)
    if not 1 <= n <= MAX_WALL_EDITS:
        raise ValueError("greedy_walls: need 1 <= n <= %d rounds (heist_plan_walls takes 8 edits)" % MAX_WALL_EDITS)
    dev, N = env.device, env.n_envs
    H = min(int(env.config.max_steps), 1024) if horizon is None else int(horizon)
    cd = wall_candidates(env.grid_snapshot()) if cands is None else torch.as_tensor(cands)
    cd = cd.to(dev).reshape(N, -1, 3).to(torch.int32)
    M = int(cd.shape[1])
    p0 = env.plan_walls(torch.zeros((N, 1, 1, 3), dtype=torch.int32, device=dev), horizon=H, gamma=gamma)
    out = GreedyWalls([], [], [], torch.zeros((N, 0, 3), dtype=torch.int32, device=dev), p0.value[:, 0], p0.ticks[:, 0])
    value, ticks = p0.value[:, 0].clone(), p0.ticks[:, 0].clone()
    idx = torch.arange(M, device=dev, dtype=torch.int64).reshape(1, M)
    for _ in range(n):
        r = int(out.edits.shape[1])
        ed = torch.cat([out.edits.reshape(N, 1, r, 3).expand(N, M, r, 3), cd.reshape(N, M, 1, 3)], 2).contiguous()
        valid, level, tk, val, _ = _plan_walls_chunked(env, ed, None, H, gamma, max_bytes)
        gain = value.reshape(-1, 1) - val
        ok = valid & level & (tk >= 0) & (gain > 0)
        g = torch.where(ok, gain, torch.full_like(gain, -1.0))
        top = g.max(1, keepdim=True).values
        first = torch.where(ok & (g == top), idx.expand_as(g), torch.full_like(idx.expand_as(g), M)).min(1).values
        pick = torch.where(first < M, first, torch.full_like(first, -1))
        if not bool((pick >= 0).any()):
            break
        i1 = pick.clamp(min=0).reshape(-1, 1)
        chosen = cd.gather(1, i1.reshape(-1, 1, 1).expand(-1, 1, 3)).reshape(N, 3)
        chosen = torch.where((pick >= 0).reshape(-1, 1), chosen, torch.zeros_like(chosen))
        value = torch.where(pick >= 0, val.gather(1, i1).reshape(-1), value)
        ticks = torch.where(pick >= 0, tk.gather(1, i1).reshape(-1), ticks)
        out.edits = torch.cat([out.edits, chosen.reshape(N, 1, 3)], 1)
        out.index.append(pick)
        out.value.append(value.clone())
        out.ticks.append(ticks.clone())
    return out
