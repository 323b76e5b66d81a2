"""heist_plan_q's contract restated in torch (heist_amd.search.q_values) against the NumPy reference
tables (value_ref), the torch playout (play_table) and the C oracle, and its consumer
(SolverAgent.imitation_update(optimal=...)) on CPU tensors.  No GPU.  Every float64 comparison is
equality of the bits (through int64) unless a bound is stated."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import field_ref as fr
import plan_ref as pr
import value_ref as vr
from heist_amd import _native
from heist_amd.obs_compact import record_cells, record_words
from heist_amd.search import discounted_return, play_table, q_values

VALID = [n for n in pr.CASES if n != "full_wallrow"]  # test_plan_play_cpu's cases
H, G, N = pr.MAX_STEPS, pr.GRID, len(VALID)
RC = G * G
NVIS = (RC + 31) // 32
STARTS = np.array([pr.CASES[n][1] for n in VALID])
D0 = np.array([abs(int(s[0]) - pr.VAULT[0]) + abs(int(s[1]) - pr.VAULT[1]) for s in STARTS])
SEED = 3  # test_plan_play_cpu's: at noise 0.25 it leaves the expert's action and ends a play detected
REGRET_TOL = 1e-9  # rounding alone: <= 1,024 steps x a few operations x 2^-53 x |q| <= 25 is ~1e-11


def _pv(gamma):
    return vr.cases_value(VALID, record_words(G, G), gamma)


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int64)


def _q(pv, pos, taken=None, tick0=None, values=None, vis=None, gamma=None):
    return q_values(pv.value_ticks if values is None else values, pv.vis if vis is None else vis, pv.grid,
                    torch.zeros(N, dtype=torch.int64) if tick0 is None else tick0, pos, H, torch.from_numpy(D0),
                    pr.VAULT, gamma=pv.gamma if gamma is None else gamma, taken=taken)


def _cell_pos(x, K=H):
    """[K, N, 2]: every env on cell x at every k."""
    return torch.tensor([x // G, x % G]).reshape(1, 1, 2).expand(K, N, 2)


def _q_ref(i, k, gamma, tick0=0):
    """[5, RC] float64: the header's q of env i, step k, for every cell, in NumPy from the
    fixtures' planes and value_ref's table -- no line of search.py."""
    planes, walls = fr.case_reference(VALID[i])[:2]
    vt = vr.case_value(VALID[i], gamma, int(D0[i]))[2]
    mv = fr.moves(np.asarray(walls, bool)).reshape(5, -1)
    dist = vr.manhattan(G, G, pr.VAULT)
    seen_plane = np.asarray(planes[k], bool).reshape(-1)
    last = tick0 + k + 1 >= H
    nxt = vt[k + 1].reshape(-1) if k + 1 < H else np.zeros(RC)
    out = np.empty((5, RC), np.float64)
    for a in range(5):
        y = mv[a]
        curr = dist[y]
        rew = np.full(RC, vr.REWARD_CONSTS[0], np.float64)
        rew = rew + (dist - curr).astype(np.float64) * np.float64(0.1)
        if D0[i] > 3:
            rew = np.where(curr <= 3, rew + np.float64(0.05) * (3 - curr).astype(np.float64), rew)
        seen = seen_plane[y]
        rew = np.where(seen, rew + np.float64(vr.REWARD_CONSTS[1]), rew)
        atv = y == pr.VAULT[0] * G + pr.VAULT[1]
        rew = np.where(atv, rew + np.float64(vr.REWARD_CONSTS[2]), rew)
        if last:
            frac = np.float64(1.0) - curr.astype(np.float64) / np.float64(max(int(D0[i]), 1))
            rew = rew + np.where(frac < 0, np.float64(0.0), frac) * np.float64(2.0)
        out[a] = np.where(seen | atv | last, rew, rew + np.float64(gamma) * nxt[y])
    return out, mv


def _play(pv, noise):
    return play_table(pv.action_ticks, pv.vis, pv.grid, torch.zeros(N, dtype=torch.int64), torch.from_numpy(STARTS),
                      H, torch.from_numpy(D0), pr.VAULT, values=pv.value_ticks, noise=noise, seed=SEED)


def _play_states(p):
    """(pos [H, N, 2], valid [H, N]) of a play: row 0 the start cells, row k the cell of record k - 1."""
    pos = torch.cat([torch.from_numpy(STARTS).to(torch.int32).reshape(1, N, 2), record_cells(p.records, G, G)[:H - 1]])
    return pos, torch.arange(H).reshape(H, 1) < p.length.reshape(1, N)


# ---- 1. registration

def test_plan_q_entry_point_exported():
    import heist_amd
    assert "heist_plan_q" in _native.SIGNATURES and "heist_plan_q" in _native.header_functions()
    lib = _native.lib()
    assert hasattr(lib, "heist_plan_q") and lib.heist_abi_version() == 5
    assert lib.heist_plan_q(None, 4, 4, 1.0, *([None] * 11)) == 100000  # a bad handle
    for name in ("PlanQ", "q_values", "record_cells"):
        assert hasattr(heist_amd, name), name
    assert hasattr(heist_amd.HeistEnv, "plan_q")
    from heist_amd.training import AdversarialTrainer
    assert hasattr(AdversarialTrainer, "dagger_solver")
    pv = heist_amd.PlanValue(*([None] * 5), G, G)  # the new field is last and optional
    assert pv.tick is None and pv.grid is None
    assert heist_amd.ExpertData(*([None] * 7), G, G, pr.VAULT).optimal is None


# ---- 2. every cell and tick of the fixtures against the reference tables

@pytest.mark.parametrize("gamma", (1.0, 0.99))
def test_q_values_every_cell(gamma):
    pv = _pv(gamma)
    walls = pv.grid.reshape(N, RC) == 1
    for x in range(RC):
        out = _q(pv, _cell_pos(x))
        assert out.q.shape == (H, N, 5) and out.q.dtype == out.value.dtype == torch.float64
        assert out.best.dtype == torch.int8 and out.optimal.dtype == torch.uint8 and out.gap is None
        # max_a q is V_k[x], the first argmax is the table's action (walls: the fill is the table's 0.0 / -1)
        assert torch.equal(_bits(out.value), _bits(pv.value_ticks.reshape(H, N, RC)[:, :, x])), x
        assert torch.equal(out.best, pv.action_ticks.reshape(H, N, RC)[:, :, x]), x
        live = ~walls[:, x].reshape(1, N).expand(H, N)
        assert bool((out.best[live] >= 0).all()) and bool((out.best[~live] == -1).all())
        assert bool((((out.optimal[live].long() >> out.best[live].long()) & 1) == 1).all()), x
        assert not out.optimal[~live].any() and not _bits(out.q[~live]).any()
        assert torch.equal(_bits(out.q.max(-1).values[live]), _bits(out.value[live]))


@pytest.mark.parametrize("gamma", (1.0, 0.99))
def test_q_values_against_numpy(gamma):
    """The five values themselves, env 3 (walls, a camera and a guard) and the empty env, all cells."""
    pv = _pv(gamma)
    for i in (VALID.index("wallrow_both"), VALID.index("empty")):
        walls = (pv.grid[i].reshape(RC) == 1).numpy()
        ref = np.stack([_q_ref(i, k, gamma)[0] for k in range(H)])  # [H, 5, RC]
        for x in np.flatnonzero(~walls):
            got = _q(pv, _cell_pos(int(x))).q[:, i].numpy()
            assert (vr.bits(got) == vr.bits(ref[:, :, x])).all(), (i, x)


# ---- 3. along plays: the taken action's value, the gap, the regret

@pytest.mark.parametrize("gamma", (1.0, 0.99))
@pytest.mark.parametrize("noise", (0.0, 0.25, 1.0))
def test_q_values_along_plays(noise, gamma):
    pv = _pv(gamma)
    p = _play(pv, noise)
    pos, valid = _play_states(p)
    out = _q(pv, pos, taken=p.actions)
    qt = out.q.gather(2, p.actions.unsqueeze(-1)).squeeze(-1)
    k = torch.arange(H).reshape(H, 1)
    term = valid & (k == (p.length.reshape(1, N) - 1))
    cont = valid & ~term
    assert int(term.sum()) == N and int(cont.sum()) >= N
    nxt = torch.cat([p.value[1:], torch.zeros(1, N, dtype=torch.float64)])
    boot = p.reward64 + float(gamma) * nxt  # multiply, then add
    assert torch.equal(_bits(qt[cont]), _bits(boot[cont]))
    assert torch.equal(_bits(qt[term]), _bits(p.reward64[term]))
    assert torch.equal(_bits(out.value[valid]), _bits(p.value[valid]))
    assert torch.equal(out.best[valid], p.expert[valid])
    assert torch.equal(_bits(out.gap), _bits(out.value - qt))
    assert bool((out.gap[valid] >= 0.0).all())
    assert torch.equal(out.gap[valid] == 0.0, ((out.optimal[valid].long() >> p.actions[valid]) & 1) == 1)
    if noise == 0.0:
        assert not _bits(out.gap[valid]).any()  # exactly 0.0
    else:
        assert bool((out.gap[valid] > 0.0).any())
    # the regret: V_0[start] - the play's return is the discounted sum of its gaps
    regret = out.value[0] - discounted_return(p.reward64, p.done, gamma)
    disc = torch.tensor([float(gamma) ** j for j in range(H)], dtype=torch.float64).reshape(H, 1)
    total = (torch.where(valid, out.gap, torch.zeros_like(out.gap)) * disc).sum(0)
    print("noise %r gamma %r: regret %s, sum of gaps off by %.3g" % (noise, gamma, regret.tolist(),
                                                                    float((regret - total).abs().max())))
    assert float((regret - total).abs().max()) <= REGRET_TOL
    if noise == 0.0:
        assert not _bits(regret).any()


# ---- 4. optimal sets that are not trivial, found from the reference alone

def test_q_values_nontrivial_sets():
    gamma = 0.99
    pv = _pv(gamma)
    tie = worse = None
    for i in range(N):
        walls = (pv.grid[i].reshape(RC) == 1).numpy()
        for k in range(H):
            ref, mv = _q_ref(i, k, gamma)
            top = ref.max(0)
            for x in np.flatnonzero(~walls):
                best = np.flatnonzero(ref[:, x] == top[x])
                if tie is None and len(set(mv[best, x].tolist())) >= 2:
                    tie = (i, k, int(x))
                if worse is None and (ref[:, x] < top[x]).any():
                    worse = (i, k, int(x))
            if tie and worse:
                break
    # the precondition: both kinds of state exist in the fixtures
    assert tie is not None, "no fixture state with two optimal actions that lead to different cells"
    assert worse is not None, "no fixture state with a non-optimal action"
    for i, k, x in (tie, worse):
        ref, mv = _q_ref(i, k, gamma)
        want = sum(1 << a for a in range(5) if ref[a, x] == ref[:, x].max())
        for a in range(5):
            out = _q(pv, _cell_pos(x), taken=torch.full((H, N), a))
            assert int(out.optimal[k, i]) == want
            assert vr.bits(out.gap[k, i].item()) == vr.bits(ref[:, x].max() - ref[a, x])
            assert (float(out.gap[k, i]) == 0.0) == bool(want >> a & 1)
    i, k, x = tie
    ref, mv = _q_ref(i, k, gamma)
    assert len({int(mv[a, x]) for a in range(5) if ref[a, x] == ref[:, x].max()}) >= 2
    i, k, x = worse
    ref, _ = _q_ref(i, k, gamma)
    a = int(ref[:, x].argmin())
    assert float(_q(pv, _cell_pos(x), taken=torch.full((H, N), a)).gap[k, i]) > 0.0
    print("tie at (env, k, cell) %s, non-optimal action at %s" % (tie, worse))


# ---- 5. edges

def _assert_fill(out, k, i):
    assert not _bits(out.q[k, i]).any() and not _bits(out.value[k, i]).any() and int(out.best[k, i]) == -1
    assert int(out.optimal[k, i]) == 0 and (out.gap is None or not _bits(out.gap[k, i]).any())


def test_q_values_edges():
    gamma = 0.99
    pv = _pv(gamma)
    p = _play(pv, 0.25)
    pos, valid = _play_states(p)
    full = _q(pv, pos, taken=p.actions)
    names = ("q", "value", "best", "optimal", "gap")

    def same(a, b, rows=slice(None)):
        for f in names:
            x, y = getattr(a, f), getattr(b, f)[rows]
            assert torch.equal(_bits(x) if x.dtype == torch.float64 else x, _bits(y) if y.dtype == torch.float64 else y), f
    # K < horizon: the first rows
    same(_q(pv, pos[:5], taken=p.actions[:5]), full, slice(0, 5))
    # tick0 = k0 on the tables' later rows: the full call's rows k0 ..
    k0 = 3
    mid = _q(pv, pos[k0:], taken=p.actions[k0:], tick0=torch.full((N,), k0), values=pv.value_ticks[k0:], vis=pv.vis[k0:])
    same(mid, full, slice(k0, H))
    # ... and with tick0 left at 0 the last rows differ (the timeout comes k0 ticks later)
    # (on the start cells: the play's rows after its end are the zero record's cell (0, 0), a border wall)
    stay = torch.from_numpy(STARTS).to(torch.int32).reshape(1, N, 2).expand(H, N, 2)
    late0 = _q(pv, stay[k0:], values=pv.value_ticks[k0:], vis=pv.vis[k0:])
    late3 = _q(pv, stay[k0:], values=pv.value_ticks[k0:], vis=pv.vis[k0:], tick0=torch.full((N,), k0))
    assert torch.equal(_bits(late3.q), _bits(_q(pv, stay).q[k0:]))
    assert torch.equal(_bits(late0.q[:H - k0 - 1]), _bits(late3.q[:H - k0 - 1]))
    assert not torch.equal(_bits(late0.q[H - k0 - 1]), _bits(late3.q[H - k0 - 1]))
    # tick0 = -1: nothing is live; one env alone
    t0 = torch.zeros(N, dtype=torch.int64)
    t0[1] = -1
    dead = _q(pv, pos, taken=p.actions, tick0=t0)
    for k in (0, 7, H - 1):
        _assert_fill(dead, k, 1)
    assert torch.equal(_bits(dead.q[:, 0]), _bits(full.q[:, 0]))
    # k + 1 == horizon: V_{k+1} is 0.0 -- a table cut to 5 rows equals one whose row 5 is zeroed
    cut = _q(pv, pos[:5], taken=p.actions[:5], values=pv.value_ticks[:5], vis=pv.vis[:5])
    zeroed = pv.value_ticks[:6].clone()
    zeroed[5] = 0.0
    z = _q(pv, pos[:5], taken=p.actions[:5], values=zeroed, vis=pv.vis[:6])
    same(cut, z)
    assert torch.equal(_bits(cut.q[:4]), _bits(full.q[:4])) and not torch.equal(_bits(cut.q[4]), _bits(full.q[4]))
    # tick = max_steps - 1: one step, against the oracle after 39 WAITs, every action
    e = VALID.index("empty")
    start = torch.from_numpy(STARTS).to(torch.int32).reshape(1, N, 2)
    lastq = _q(pv, start, taken=torch.zeros((1, N), dtype=torch.int64), tick0=torch.full((N,), H - 1),
               values=pv.value_ticks[H - 1:], vis=pv.vis[H - 1:])
    for a in range(5):
        layout, st = pr.CASES["empty"][:2]
        o = fr.oracle_env(G, G, H, st, pr.VAULT, layout, pr.BUDGET)[0]
        for _ in range(H - 1):
            o.step(0)
        r, d, s = o.step(a)
        assert (d, s) == (True, 3) and vr.bits(lastq.q[0, e, a].item()) == vr.bits(r), a
    assert vr.bits(lastq.value[0, e].item()) == vr.bits(pv.value_ticks[H - 1, e][tuple(STARTS[e])].item())
    # a wall cell, cells off the grid
    w = VALID.index("wallrow_cam")
    cells = pos.clone()
    cells[:, w] = torch.tensor(pr.WALLROW[0], dtype=torch.int32)
    cells[:, 0] = torch.tensor([G, 0], dtype=torch.int32)
    cells[:, 2] = torch.tensor([0, -1], dtype=torch.int32)
    odd = _q(pv, cells, taken=p.actions)
    for k in (0, H - 1):
        for i in (w, 0, 2):
            _assert_fill(odd, k, i)
    assert torch.equal(_bits(odd.q[:, 3]), _bits(full.q[:, 3]))
    # taken outside 0 .. 4 counts as WAIT
    for bad in (-1, 5, 7):
        g = _q(pv, pos, taken=torch.full((H, N), bad)).gap
        assert torch.equal(_bits(g), _bits(_q(pv, pos, taken=torch.zeros((H, N), dtype=torch.int64)).gap))
    with pytest.raises(ValueError):
        _q(pv, pos[:, :2])


def test_record_cells():
    rec = torch.zeros((3, N, record_words(G, G)), dtype=torch.int32)
    rec[..., NVIS] = 7 | 9 << 8
    rec[1, 2, NVIS] = 0 | 3 << 8
    cells = record_cells(rec, G, G)
    assert cells.shape == (3, N, 2) and cells.dtype == torch.int32
    assert cells[0, 0].tolist() == [7, 9] and cells[1, 2].tolist() == [0, 3]


def test_expert_data_flat_optimal():
    from heist_amd.search import expert_data
    pv = _pv(0.99)
    p = _play(pv, 0.25)
    pos, valid = _play_states(p)
    rec0 = torch.zeros((N, record_words(G, G)), dtype=torch.int32)
    rec0[:, NVIS] = torch.from_numpy(STARTS[:, 0] | STARTS[:, 1] << 8).to(torch.int32)
    data = expert_data(p, rec0, pv.grid, G, G, pr.VAULT)
    assert data.optimal is None and data.flat_optimal()[4] is None and len(data.flat()) == 4
    data.optimal = _q(pv, pos).optimal
    obs, expert, value, taken, opt = data.flat_optimal()
    assert torch.equal(opt, data.optimal[data.valid]) and opt.shape == expert.shape
    assert bool((((opt.long() >> expert) & 1) == 1).all())  # the single label is in its set
    mask = torch.zeros(N, dtype=torch.bool)
    mask[2] = True
    assert len(data.flat_optimal(mask)[4]) == int(p.length[2])


# ---- 6. the supervised step on sets

def test_imitation_update_optimal_sets_cpu():
    from heist_amd.agents.solver import SolverAgent
    torch.manual_seed(0)
    agent = SolverAgent(grid_rows=G, grid_cols=G, device="cpu")
    obs = torch.rand(64, 3, G, G)
    sets = torch.randint(1, 32, (64,), dtype=torch.int64).to(torch.uint8)
    sets[::9] = 0  # left out
    value = torch.randn(64)
    keep = sets != 0
    twin = copy.deepcopy(agent.network)
    twin.train()
    with torch.no_grad():
        logits, v, _ = twin(obs[keep])
        prob = F.softmax(logits.double(), -1)  # an independent form: -log of the set's probability
        member = ((sets[keep].long().reshape(-1, 1) >> torch.arange(5)) & 1).bool()
        nll = float(-(prob * member).sum(-1).log().mean())
        agree = float(member.gather(1, logits.argmax(-1, keepdim=True)).float().mean())
        mse = float(F.mse_loss(v.reshape(-1), value[keep]))
    before = [q.detach().clone() for q in agent.network.parameters()]
    m = agent.imitation_update(obs, None, value, minibatch=64, optimal=sets)
    assert m["imitation_samples"] == int(keep.sum()) and m["imitation_updates"] == 1
    assert abs(m["imitation_ce"] - nll) < 1e-6 and abs(m["imitation_value_loss"] - mse) < 1e-5 * max(1.0, mse)
    assert abs(m["imitation_agreement"] - agree) < 1e-6
    assert any(not torch.equal(a, b) for a, b in zip(before, agent.network.parameters()))
    for _ in range(19):
        last = agent.imitation_update(obs, None, value, minibatch=64, optimal=sets)
    print("set loss first %r, after 20 updates %r" % (m["imitation_ce"], last["imitation_ce"]))
    assert last["imitation_ce"] < m["imitation_ce"]


def test_imitation_update_one_hot_sets_cpu():
    """One-hot sets are the cross-entropy form: the same loss and the same step."""
    from heist_amd.agents.solver import SolverAgent
    torch.manual_seed(0)
    a = SolverAgent(grid_rows=G, grid_cols=G, device="cpu")
    b = copy.deepcopy(a)
    obs = torch.rand(64, 3, G, G)
    expert = torch.randint(0, 5, (64,))
    expert[::9] = -1
    sets = torch.where(expert >= 0, 1 << expert.clamp(min=0), torch.zeros_like(expert)).to(torch.uint8)
    value = torch.randn(64)
    torch.manual_seed(1)
    ma = a.imitation_update(obs, expert, value, minibatch=64)
    torch.manual_seed(1)
    mb = b.imitation_update(obs, expert, value, minibatch=64, optimal=sets)
    assert ma["imitation_samples"] == mb["imitation_samples"] == int((expert >= 0).sum())
    assert abs(ma["imitation_ce"] - mb["imitation_ce"]) < 1e-6  # test_imitation_update_cpu's tolerance
    assert ma["imitation_agreement"] == mb["imitation_agreement"]
    assert abs(ma["imitation_value_loss"] - mb["imitation_value_loss"]) < 1e-5 * max(1.0, ma["imitation_value_loss"])
    # every set empty: nothing to do
    m0 = b.imitation_update(obs, expert, value, minibatch=64, optimal=torch.zeros(64, dtype=torch.uint8))
    assert m0["imitation_samples"] == 0 and m0["imitation_updates"] == 0
