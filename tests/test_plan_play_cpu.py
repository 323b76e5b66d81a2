"""heist_plan_play's contract restated in torch (heist_amd.search.play_table) against the C oracle,
and its consumers (ExpertData, SolverAgent.imitation_update) on CPU tensors.  No GPU: the tables
are value_ref's (the NumPy recurrence on the oracle's witness planes), the replays run the C
oracle, the draws are recomputed in NumPy uint64.  Every float64 comparison is equality of the
bits (through int64)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import field_ref as fr
import plan_ref as pr
import value_ref as vr
from heist_amd import _native
from heist_amd.obs_compact import record_words
from heist_amd.search import expert_data, play_table

VALID = [n for n in pr.CASES if n != "full_wallrow"]  # the fixtures whose layout passes the BFS check
H, G, N = pr.MAX_STEPS, pr.GRID, len(VALID)
NVIS = (G * G + 31) // 32
STARTS = np.array([pr.CASES[n][1] for n in VALID])
FILL_STATUS = 4  # HEIST_ALREADY_DONE
# the noisy plays' seed: on these fixtures, at noise 0.25, it makes steps leave the expert's action
# and ends at least one play detected (both asserted below)
SEED = 3


def _dist(cell):
    return abs(int(cell[0]) - pr.VAULT[0]) + abs(int(cell[1]) - pr.VAULT[1])


D0 = np.array([_dist(s) for s in STARTS])


def _pv(gamma=0.99):
    return vr.cases_value(VALID, record_words(G, G), gamma)


def _play(pv, **kw):
    args = dict(tick=torch.zeros(N, dtype=torch.int64), pos=torch.from_numpy(STARTS), values=pv.value_ticks)
    args.update(kw)
    table, vis = args.pop("table", pv.action_ticks), args.pop("vis", pv.vis)
    d0 = args.pop("initial_dist", torch.from_numpy(D0))
    return play_table(table, vis, pv.grid, max_steps=H, initial_dist=d0, vault=pr.VAULT, **args)


def _bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int64)


def _assert_fill(p, i, k0):
    """Rows k0 .. of env i hold the after-the-end fill."""
    assert not p.actions[k0:, i].any() and bool((p.expert[k0:, i] == -1).all()), i
    assert not _bits(p.value[k0:, i]).any() and not _bits(p.reward64[k0:, i]).any(), i
    assert not p.records[k0:, i].any() and bool(p.done[k0:, i].all()), i
    assert bool((p.status[k0:, i] == FILL_STATUS).all()), i


def _oracle(i):
    layout, start = pr.CASES[VALID[i]][:2]
    return fr.oracle_env(G, G, H, start, pr.VAULT, layout, pr.BUDGET)[0]


def _np_mix64(z):
    z = z.astype(np.uint64)
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def _np_draws(seed, tick0, q24):
    """(noisy [H, N] bool, uniform action [H, N]) of the header's draw, independent of search.py."""
    with np.errstate(over="ignore"):
        t = (np.asarray(tick0, np.uint64).reshape(1, N) + np.arange(H, dtype=np.uint64).reshape(H, 1))
        key = np.uint64(seed) ^ (t * np.uint64(0xD1B54A32D192ED03)) ^ \
            (np.arange(N, dtype=np.uint64).reshape(1, N) * np.uint64(0x9E3779B97F4A7C15))
        z = _np_mix64(key)
        return (z >> np.uint64(40)) < np.uint64(q24), (((z & np.uint64(0xFFFFFFFF)) * np.uint64(5)) >> np.uint64(32))


# ---- 1. registration

def test_plan_play_entry_point_exported():
    import heist_amd
    assert "heist_plan_play" in _native.SIGNATURES and "heist_plan_play" in _native.header_functions()
    lib = _native.lib()
    assert hasattr(lib, "heist_plan_play") and lib.heist_abi_version() == 5
    none = [None] * 8
    assert lib.heist_plan_play(None, 4, None, None, None, None, 0, 0, *none, None) == 100000  # a bad handle, no outputs
    for name in ("PlanPlay", "ExpertData", "play_table", "expert_rollout", "expert_data"):
        assert hasattr(heist_amd, name), name
    assert hasattr(heist_amd.HeistEnv, "plan_play")
    from heist_amd.agents.solver import SolverAgent
    from heist_amd.training import AdversarialTrainer
    assert hasattr(SolverAgent, "imitation_update")
    assert hasattr(AdversarialTrainer, "pretrain_solver")


# ---- 2. without noise: the table's own play, the oracle's rewards, the value

@pytest.mark.parametrize("gamma", (1.0, 0.99))
def test_play_table_expert(gamma):
    pv = _pv(gamma)
    p = _play(pv)
    assert p.actions.shape == (H, N) and p.actions.dtype == torch.int64 and p.expert.dtype == torch.int8
    assert p.records.shape == (H, N, record_words(G, G)) and p.records.dtype == torch.int32
    assert p.value.dtype == p.reward64.dtype == torch.float64 and p.done.dtype == torch.bool
    assert p.status.dtype == torch.int8 and p.length.dtype == torch.int32
    for i, n in enumerate(VALID):
        planes, walls = fr.case_reference(n)[:2]
        plan = vr.greedy_plan(walls, pr.VAULT, planes, pv.action_ticks[:, i].numpy(), tuple(STARTS[i]))
        T = len(plan)
        assert int(p.length[i]) == T and p.actions[:T, i].tolist() == plan, n
        assert p.expert[:T, i].tolist() == plan, n
        o = _oracle(i)
        out = [o.step(a) for a in plan]
        assert vr.bits(p.reward64[:T, i].numpy()).tolist() == vr.bits([r for r, _, _ in out]).tolist(), n
        assert p.done[:T, i].tolist() == [d for _, d, _ in out], n
        assert p.status[:T, i].tolist() == [s for _, _, s in out], n
        got = vr.horner(p.reward64[:T, i].numpy(), gamma)
        v0 = pv.value[i][tuple(STARTS[i])]
        assert vr.bits(got) == vr.bits(v0.item()) == vr.bits(p.value[0, i].item()), (n, float(got), float(v0))
        _assert_fill(p, i, T)
    # the optional outputs
    q = _play(pv, values=None, records=False, rewards=False)
    assert q.value is None and q.records is None and q.reward64 is None
    assert torch.equal(q.actions, p.actions) and torch.equal(q.status, p.status) and torch.equal(q.length, p.length)


# ---- 3. with noise: the draws, the oracle's replay, the labels

@pytest.mark.parametrize("noise", (0.25, 1.0))
def test_play_table_noisy(noise):
    pv = _pv()
    p = _play(pv, noise=noise, seed=SEED)
    noisy, uni = _np_draws(SEED, np.zeros(N), int(round(noise * 2 ** 24)))
    if noise == 1.0:
        assert noisy.all()
    off_expert, detected = 0, 0
    at, vt = pv.action_ticks.numpy(), pv.value_ticks.numpy()
    for i, n in enumerate(VALID):
        T = int(p.length[i])
        assert 1 <= T <= H
        o = _oracle(i)
        for k in range(T):
            inf = o.info()
            cell = (inf["pos_r"], inf["pos_c"])
            ex, a = int(p.expert[k, i]), int(p.actions[k, i])
            assert ex == at[k, i][cell] and ex >= 0, (n, k)
            assert vr.bits(p.value[k, i].item()) == vr.bits(vt[k, i][cell]), (n, k)
            assert a == (int(uni[k, i]) if noisy[k, i] else ex), (n, k)
            off_expert += a != ex
            r, d, s = o.step(a)
            assert vr.bits(p.reward64[k, i].item()) == vr.bits(r), (n, k, float(p.reward64[k, i]), r)
            assert (bool(p.done[k, i]), int(p.status[k, i])) == (d, s), (n, k)
            assert d == (k == T - 1), (n, k)
            inf = o.info()
            rec = p.records[k, i].numpy().view(np.uint32)
            assert rec[NVIS] == inf["pos_r"] | inf["pos_c"] << 8 and not rec[NVIS + 1:].any(), (n, k)
            assert (rec[:NVIS] == pv.vis[k, i].numpy().view(np.uint32)[:NVIS]).all(), (n, k)
        detected += int(p.status[T - 1, i]) == 1
        _assert_fill(p, i, T)
    print("noise %r: %d steps off the expert's action, %d plays detected" % (noise, off_expert, detected))
    assert off_expert >= 1 and detected >= 1


# ---- 4. edges

def test_play_table_edges():
    pv = _pv()
    full = _play(pv, noise=0.25, seed=SEED)
    # horizon 5: the first five rows; a play the horizon cuts has no fill rows
    p5 = _play(pv, table=pv.action_ticks[:5], vis=pv.vis[:5], values=pv.value_ticks[:5], noise=0.25, seed=SEED)
    assert torch.equal(p5.length, full.length.clamp(max=5))
    for name in ("actions", "expert", "value", "records", "reward64", "done", "status"):
        assert torch.equal(getattr(p5, name), getattr(full, name)[:5]), name
    assert int((p5.length == 5).sum()) >= 1 and not bool(p5.done[4][full.length > 5].any())
    # tick0 > 0: a play started from the full play's cell after k0 steps, on the tables' later rows, draws the same
    k0 = 3
    word = full.records[k0 - 1, :, NVIS]
    pos = torch.stack([word & 0xFF, (word >> 8) & 0xFF], 1).to(torch.int64)
    live = full.length > k0
    assert int(live.sum()) >= 3
    pos[~live] = torch.from_numpy(STARTS)[~live]
    mid = _play(pv, table=pv.action_ticks[k0:], vis=pv.vis[k0:], values=pv.value_ticks[k0:], noise=0.25, seed=SEED,
                tick=torch.full((N,), k0, dtype=torch.int64), pos=pos)
    assert torch.equal(mid.length[live], full.length[live] - k0)
    for name in ("actions", "expert", "records", "done", "status"):
        assert torch.equal(getattr(mid, name)[:, live], getattr(full, name)[k0:, live]), name
    assert torch.equal(_bits(mid.reward64[:, live]), _bits(full.reward64[k0:, live]))
    assert torch.equal(_bits(mid.value[:, live]), _bits(full.value[k0:, live]))
    # tick = max_steps - 1: one step, the timeout's share of the reward, against the oracle after 39 WAITs
    e = VALID.index("empty")
    o = _oracle(e)
    for _ in range(H - 1):
        o.step(0)
    late = _play(pv, table=pv.action_ticks[H - 1:], vis=pv.vis[H - 1:], values=pv.value_ticks[H - 1:],
                 tick=torch.full((N,), H - 1, dtype=torch.int64))
    r, d, s = o.step(int(late.actions[0, e]))
    assert (d, s) == (True, 3) and int(late.status[0, e]) == 3 and bool(late.done[0, e]) and int(late.length[e]) == 1
    assert vr.bits(late.reward64[0, e].item()) == vr.bits(r) == vr.bits(late.value[0, e].item())
    # a done env; a start cell outside the grid
    done = torch.zeros(N, dtype=torch.bool)
    done[1] = True
    pos = torch.from_numpy(STARTS).clone()
    pos[2] = torch.tensor([G, 0])
    pos[3] = torch.tensor([0, -1])
    pd = _play(pv, done=done, pos=pos)
    clean = _play(pv)
    assert pd.length.tolist()[1:4] == [0, -1, -1]
    for i in (1, 2, 3):
        _assert_fill(pd, i, 0)
    for i in (0, 4, 5):
        assert torch.equal(pd.actions[:, i], clean.actions[:, i]) and pd.length[i] == clean.length[i]
    # another start cell: the labels are the table's there and the play collects exactly its value
    pos = torch.from_numpy(STARTS).clone()
    pos[e] = torch.tensor([3, 3])
    po = _play(pv, pos=pos, initial_dist=torch.from_numpy(D0))
    T = int(po.length[e])
    assert int(po.expert[0, e]) == int(pv.action_ticks[0, e, 3, 3])
    assert vr.bits(vr.horner(po.reward64[:T, e].numpy(), 0.99)) == vr.bits(pv.value_ticks[0, e, 3, 3].item())
    assert vr.bits(po.value[0, e].item()) == vr.bits(pv.value_ticks[0, e, 3, 3].item())
    # a table entry of -1 (and one of 7) at a live state is played as WAIT and labelled -1
    for bad in (-1, 7):
        table = pv.action_ticks.clone()
        table[0, e, 1, 1] = bad
        pb = _play(pv, table=table)
        assert (int(pb.expert[0, e]), int(pb.actions[0, e])) == (-1, 0)
        assert int(pb.records[0, e, NVIS]) == 1 | 1 << 8 and int(pb.status[0, e]) == 0
        assert int(pb.length[e]) >= 2 and int(pb.expert[1, e]) == int(pv.action_ticks[1, e, 1, 1])
    with pytest.raises(ValueError):
        _play(pv, noise=1.5)


# ---- 5. the decision states

def test_expert_data():
    pv = _pv()
    p = _play(pv, noise=0.25, seed=SEED)
    rec0 = torch.zeros((N, record_words(G, G)), dtype=torch.int32)
    rec0[:, NVIS] = torch.from_numpy(STARTS[:, 0] | STARTS[:, 1] << 8).to(torch.int32)
    data = expert_data(p, rec0, pv.grid, G, G, pr.VAULT)
    assert data.valid.shape == (H, N) and int(data.valid.sum()) == int(p.length.sum())
    at = pv.action_ticks.numpy()
    for i in range(N):
        for k in range(int(p.length[i])):
            w = int(data.records[k, i, NVIS])
            assert int(data.expert[k, i]) == at[k, i, w & 0xFF, (w >> 8) & 0xFF], (i, k)
    obs, expert, value, taken = data.flat()
    n = int(p.length.sum())
    assert len(obs) == n and expert.shape == value.shape == taken.shape == (n,)
    assert expert.dtype == taken.dtype == torch.int64 and value.dtype == torch.float32
    assert torch.equal(expert, p.expert.to(torch.int64)[data.valid]) and torch.equal(taken, p.actions[data.valid])
    assert torch.equal(obs.rec_env.long(), torch.arange(N).repeat(H)[data.valid.reshape(-1)])
    mask = torch.zeros(N, dtype=torch.bool)
    mask[2] = True
    assert len(data.flat(mask)[0]) == int(p.length[2])
    with pytest.raises(ValueError):
        expert_data(_play(pv, records=False), rec0, pv.grid, G, G, pr.VAULT)


# ---- 6. the supervised step

def test_imitation_update_cpu():
    from heist_amd.agents.solver import SolverAgent
    torch.manual_seed(0)
    agent = SolverAgent(grid_rows=G, grid_cols=G, device="cpu")
    obs = torch.rand(64, 3, G, G)
    expert = torch.randint(0, 5, (64,))
    expert[::9] = -1  # left out
    value = torch.randn(64)
    keep = expert >= 0
    twin = copy.deepcopy(agent.network)
    twin.train()
    with torch.no_grad():
        logits, v, _ = twin(obs[keep])
        ce = float(F.cross_entropy(logits, expert[keep]))
        mse = float(F.mse_loss(v.reshape(-1), value[keep]))
    before = [q.detach().clone() for q in agent.network.parameters()]
    m = agent.imitation_update(obs, expert, value, minibatch=64)
    assert m["imitation_samples"] == int(keep.sum()) and m["imitation_updates"] == 1
    assert abs(m["imitation_ce"] - ce) < 1e-6 and abs(m["imitation_value_loss"] - mse) < 1e-5 * max(1.0, mse)
    assert 0.0 <= m["imitation_agreement"] <= 1.0
    assert any(not torch.equal(a, b) for a, b in zip(before, agent.network.parameters()))
    for _ in range(19):
        last = agent.imitation_update(obs, expert, value, minibatch=64)
    print("imitation_ce first %r, after 20 updates %r" % (m["imitation_ce"], last["imitation_ce"]))
    assert last["imitation_ce"] < m["imitation_ce"]
    # without value labels: the cross-entropy alone
    m2 = agent.imitation_update(obs, expert, minibatch=64)
    assert m2["imitation_value_loss"] == 0.0
