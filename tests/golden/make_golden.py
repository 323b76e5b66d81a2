"""Generate the golden parity fixtures by running the Python reference.

Runs ONLY in the build container (it imports /root/reference, which never
travels to the GPU box).  Everything it writes under tests/golden/ is data:
layouts, action sequences and the reference's outputs for them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py

Fixture files (all numpy .npz, loaded with allow_pickle=False):
  env_traces.npz  layouts + action/reset sequences replayed through
                  HeistEnvironment.set_layout/reset/step/get_state_tensor
                  (environment.py:102-374): per-op reward (f64), done, status,
                  position, tick, camera headings, guard idx/headings,
                  visibility bits, state tensors for the first ops.
  env_traces_offcorner.npz  (key `offcorner`) the same format on 16 traces whose start and
                  vault are away from the grid corners: every lane of the observation's
                  float4 under the vault, solver and vault in one float4, start == vault,
                  the vault on the border ring, the start at (0, 0), assets named on the
                  start and vault cells; actions steered towards the vault.
  bfs_edges.npz   (key `bfs_edges`) bfs_path_exists on 64-wide / 64-high / thin grids:
                  endpoints in the last row or column, walls under the endpoints,
                  grid-filling corridors and their plugged twins, dense random fills.
  cones.npz       Camera.get_vision_cone_tiles / Guard.get_visible_tiles
                  sweeps (security.py:53-101, :161-192).
  cone_order.npz  the same methods' LIST order (first visit by ray index, then
                  distance) on 600 more cases: ordered flat tile indices.
  bfs.npz         bfs_path_exists on random grids (utils.py:52-85).
  ppo.npz         SolverAgent._compute_gae (agents/solver.py:228-244) and the
                  clipped-PPO loss + d(loss)/d(logits, values) of
                  SolverAgent.update (agents/solver.py:112-204), captured
                  through a stub network.
  nets.npz        seeded SolverNetwork / ArchitectNetwork weights and forward
                  outputs (networks.py:13-239) + ArchitectNetwork
                  .generate_layout decode cases (networks.py:241-335).
  kat.json        the numbers test_sanity.py / test_fixes.py print.
  arch_update.npz ArchitectAgent.update (agents/architect.py:91-155) from the
                  nets.npz seed-32 ArchitectNetwork: per case the buffered
                  (log_prob, value, reward) transitions in, the returned losses,
                  and per parameter tensor the gradient left after the update
                  (clipped) and the parameter change, as L2 norms plus 4 fixed
                  random projections (proj_vectors(): data, not weights).
  solver_update_<case>.npz  (key `update`, or `update:g20,clip20` for some cases)
                  SolverAgent.update (agents/solver.py:112-217) from the nets.npz
                  Solver weights on buffers filled by reference episodes on
                  Architect layouts (select_action / store_transition), cases
                  g20, g32, g10, clip20, big20 (UPDATE_CASES): the buffers (states
                  as occupancy codes per layout + visibility bits + position
                  index, bit-exact), the replayed shuffles, normalised advantages
                  and returns, the metrics; at the first step, the first short
                  minibatch and the last step the loss parts, the pre-clip total
                  norm and gradients (conv tensors in full, the others as L2 norm
                  + 4 projections); the parameter change likewise; and the
                  reference's own float32 error against the float64 restatement
                  tests/solver_update_ref.py per tensor (the tests' noise floor).
                  One file per case: each stays under 1 MiB.
"""
import json
import os
import sys

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

import torch  # noqa: E402

from heist_architect.environment import HeistEnvironment, EnvironmentConfig  # noqa: E402
from heist_architect.components.security import Camera, Guard  # noqa: E402
from heist_architect.utils import bfs_path_exists, create_empty_grid, TileType  # noqa: E402
from heist_architect.agents.solver import SolverAgent  # noqa: E402
from heist_architect.agents.architect import ArchitectAgent  # noqa: E402
from heist_architect.networks import SolverNetwork, ArchitectNetwork  # noqa: E402
from heist_architect.rewards import RewardCalculator  # noqa: E402

STATUS = {"running": 0, "detected": 1, "vault_reached": 2, "timeout": 3, "already_done": 4, "reset": 5}


# ---------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------

def f32(x):
    return float(np.float32(x))


def synth_layout(rng, R, C, budget, n_cams=None, n_guards=None, int_params=False):
    """Direct synthetic generator."""
    walls, cams, guards = [], [], []
    interior = [(r, c) for r in range(1, R - 1) for c in range(1, C - 1)
                if (r, c) not in ((1, 1), (R - 2, C - 2))]
    if n_cams is None:
        n_cams = int(rng.integers(0, budget // 3 + 1))
    if n_guards is None:
        n_guards = int(rng.integers(0, budget // 5 + 1))
    left = budget - 3 * n_cams - 5 * n_guards
    n_walls = max(0, left + int(rng.integers(-1, 3)))
    picks = rng.permutation(len(interior))
    k = 0
    for _ in range(n_walls):
        walls.append(interior[picks[k]]); k += 1
    for _ in range(n_cams):
        r, c = interior[picks[k % len(interior)]]; k += 1
        if int_params:
            fov, head, spd = float(rng.choice([30, 45, 60, 75, 90, 120])), float(rng.integers(0, 24) * 15), float(rng.choice([5, 10, 15, 20, 30, -15]))
        else:
            fov, head, spd = f32(rng.uniform(30, 120)), f32(rng.uniform(0, 360)), f32(rng.uniform(5, 35))
        cams.append({"row": r, "col": c, "fov_angle": fov, "heading": head,
                     "rotation_speed": spd, "vision_range": int(rng.choice([6, 6, 6, 4, 8]))})
    for _ in range(n_guards):
        r, c = interior[picks[k % len(interior)]]; k += 1
        guards.append({"patrol_path": ArchitectNetwork._generate_patrol(None, r, c, R, C),
                       "speed": 1, "vision_range": 4, "fov_angle": 90.0})
    return walls, cams, guards


def hand_layouts():
    """(R, C, max_steps, budget, walls, cams, guards, name) quirk layouts."""
    L = []
    # test_sanity.py:20-29
    L.append((10, 10, 200, 15, [(3, 3), (3, 4), (3, 5)],
              [{"row": 5, "col": 5, "fov_angle": 60, "heading": 0, "rotation_speed": 15, "vision_range": 4}],
              [{"patrol_path": [(7, 2), (7, 3), (7, 4), (7, 5)], "speed": 1, "vision_range": 3, "fov_angle": 90}],
              "sanity"))
    # test_fixes.py: empty 10x10
    L.append((10, 10, 200, 15, [], [], [], "empty10"))
    # guard start on a wall, on START, on VAULT, on a camera (environment.py:138-149)
    L.append((12, 12, 60, 40, [(4, 4), (4, 5), (2, 6)],
              [{"row": 6, "col": 6, "fov_angle": 90.0, "heading": 45.0, "rotation_speed": 10.0, "vision_range": 5}],
              [{"patrol_path": [(4, 4), (4, 5), (5, 5), (5, 4)], "speed": 1},
               {"patrol_path": [(1, 1), (1, 2)], "speed": 1},
               {"patrol_path": [(6, 6), (7, 6), (7, 7)], "speed": 2, "vision_range": 3, "fov_angle": 120.0}],
              "guard_overwrites"))
    # duplicates, out-of-interior placements and over budget (budget.py:48-58)
    L.append((10, 10, 50, 9, [(2, 2), (2, 2), (0, 3), (9, 9), (1, 1), (3, 3), (8, 8)],
              [{"row": 2, "col": 2, "fov_angle": 60.0}, {"row": 5, "col": 3, "fov_angle": 33.3, "heading": 359.5, "rotation_speed": -7.25},
               {"row": 6, "col": 6}],
              [{"patrol_path": [(7, 7), (7, 8)]}],
              "placement_rules"))
    # vault reachable exactly on the last tick (status overwritten by timeout)
    L.append((6, 6, 6, 0, [], [], [], "vault_last_tick"))
    # single-point patrol, empty patrol, speed 3 wrap, negative speed
    L.append((14, 14, 120, 40, [(5, 5), (5, 6), (5, 7)], [],
              [{"patrol_path": [(8, 8)]}, {"patrol_path": []},
               {"patrol_path": [(2, 9), (2, 10), (2, 11), (3, 11), (4, 11)], "speed": 3, "vision_range": 5, "fov_angle": 70.0},
               {"patrol_path": [(10, 2), (10, 3), (11, 3), (11, 2)], "speed": -1, "vision_range": 4, "fov_angle": 90.0}],
              "patrol_variants"))
    # wide and narrow cameras near walls, integer headings, range 8
    L.append((16, 16, 150, 40, [(7, 7), (7, 8), (8, 7), (3, 10), (10, 3)],
              [{"row": 8, "col": 8, "fov_angle": 120.0, "heading": 0.0, "rotation_speed": 15.0, "vision_range": 8},
               {"row": 3, "col": 3, "fov_angle": 30.0, "heading": 270.0, "rotation_speed": 30.0, "vision_range": 6},
               {"row": 12, "col": 12, "fov_angle": 75.0, "heading": 135.0, "rotation_speed": 22.5, "vision_range": 6}],
              [], "cameras_integer"))
    # blocked level (BFS false)
    L.append((10, 10, 50, 40, [(2, 1), (2, 2), (1, 2)], [], [], "blocked"))
    return L


def architect_layouts(n, R, C, budget, seed, allow_cams=True, allow_guards=True, temps=(1.0, 1.5, 0.5, 2.0)):
    torch.manual_seed(seed)
    arch = ArchitectAgent(grid_rows=R, grid_cols=C, budget=budget)
    out = []
    for i in range(n):
        w, c, g = arch.generate_layout(temps[i % len(temps)])
        if not allow_cams:
            c = []
        if not allow_guards:
            g = []
        out.append((w, c, g))
    return out


# ---------------------------------------------------------------------------
# env traces
# ---------------------------------------------------------------------------

def gen_ops(rng, n_ops, R, C):
    """Action sequence (0-4) with -1 = reset().  Biased toward the vault."""
    ops = [-1]
    for _ in range(n_ops):
        u = rng.random()
        if u < 0.35:
            ops.append(int(rng.choice([2, 4])))
        else:
            ops.append(int(rng.integers(0, 5)))
    return ops


def run_trace(cfg, layout, ops, n_state, budget, policy=None):
    """Replay ops through the reference env.  With a policy, op k is policy(env, k, ops[k]) (an
    action chosen from the env's state as it stands before the op); rec["ops"] holds the ops run."""
    env = HeistEnvironment(cfg)
    env.budget.scale_budget(budget)
    walls, cams, guards = layout
    valid = env.set_layout(walls, cams, guards)
    rec = {"valid": valid, "grid": env.grid.copy(), "n_walls": len(env.walls),
           "n_cams": len(env.cameras), "n_guards": len(env.guards), "spent": env.budget.spent,
           "reward": [], "done": [], "status": [], "pos": [], "tick": [], "cam_h": [],
           "g_idx": [], "g_h": [], "vis": [], "state": [], "ops": []}
    done = False
    for k, op in enumerate(ops):
        if policy is not None:
            op = policy(env, k, op)
        rec["ops"].append(op)
        if op == -1:
            env.reset()
            r, d, st = 0.0, env.done, STATUS["reset"]
        else:
            _, r, d, info = env.step(op)
            st = STATUS[info["status"]]
        rec["reward"].append(float(r)); rec["done"].append(bool(d)); rec["status"].append(st)
        rec["pos"].append(env.solver_pos); rec["tick"].append(env.tick)
        rec["cam_h"].extend(cm.heading for cm in env.cameras)
        rec["g_idx"].extend(g.current_idx for g in env.guards)
        rec["g_h"].extend(g.heading for g in env.guards)
        rec["vis"].append(env.visibility_map.visibility > 0.5)
        if k < n_state:
            rec["state"].append(env.get_state_tensor())
    return rec


def pack_layouts(items):
    """Flatten (walls, cams, guards) lists into padded arrays + offsets."""
    W, Wo, Cm, Co, Gp, Gi, Gf, Go, Pp = [], [0], [], [0], [], [], [], [0], []
    for walls, cams, guards in items:
        for r, c in walls:
            W.append((r, c))
        Wo.append(len(W))
        for cd in cams:
            Cm.append((cd["row"], cd["col"], cd.get("fov_angle", 60.0), cd.get("heading", 0.0),
                       cd.get("rotation_speed", 15.0), cd.get("vision_range", 6)))
        Co.append(len(Cm))
        for gd in guards:
            path = gd["patrol_path"]
            Gi.append((len(Pp), len(path), gd.get("speed", 1), gd.get("vision_range", 4)))
            Gf.append(gd.get("fov_angle", 90.0))
            Pp.extend(path)
        Go.append(len(Gi))
    return dict(walls=np.array(W, np.int32).reshape(-1, 2), walls_off=np.array(Wo, np.int64),
                cams=np.array(Cm, np.float64).reshape(-1, 6), cams_off=np.array(Co, np.int64),
                guards_i=np.array(Gi, np.int64).reshape(-1, 4), guards_fov=np.array(Gf, np.float64),
                guards_off=np.array(Go, np.int64), paths=np.array(Pp, np.int32).reshape(-1, 2))


def make_env_traces():
    rng = np.random.default_rng(20260215)
    cases = []  # (name, R, C, max_steps, budget, layout, n_ops)
    for (R, C, ms, b, w, c, g, name) in hand_layouts():
        cases.append((name, R, C, ms, b, (w, c, g), 400))
    for i, lay in enumerate(architect_layouts(6, 20, 20, 15, 101)):
        cases.append(("arch20_b15_%d" % i, 20, 20, 200, 15, lay, 420))
    for i, lay in enumerate(architect_layouts(3, 20, 20, 40, 102)):
        cases.append(("arch20_b40_%d" % i, 20, 20, 200, 40, lay, 300))
    for i, lay in enumerate(architect_layouts(3, 20, 20, 8, 103, allow_guards=False)):
        cases.append(("arch20_b8_cams_%d" % i, 20, 20, 200, 8, lay, 300))
    for i, lay in enumerate(architect_layouts(2, 20, 20, 5, 104, allow_cams=False, allow_guards=False)):
        cases.append(("arch20_walls_%d" % i, 20, 20, 200, 5, lay, 300))
    for i, lay in enumerate(architect_layouts(2, 10, 10, 5, 105)):
        cases.append(("arch10_b5_%d" % i, 10, 10, 200, 5, lay, 300))
    for i, lay in enumerate(architect_layouts(2, 32, 32, 27, 106)):
        cases.append(("arch32_b27_%d" % i, 32, 32, 200, 27, lay, 250))
    for i in range(6):
        R = C = 20
        lay = synth_layout(rng, R, C, 15, int_params=(i % 2 == 0))
        cases.append(("synth20_%d" % i, R, C, 200, 15, lay, 400))
    for i in range(2):
        lay = synth_layout(rng, 32, 32, 40, n_cams=4, n_guards=3)
        cases.append(("synth32_%d" % i, 32, 32, 200, 40, lay, 250))
    lay = synth_layout(rng, 24, 17, 25, n_cams=3, n_guards=2)
    cases.append(("synth24x17", 24, 17, 80, 25, lay, 300))

    n_state = 24
    runs = []
    for (name, R, C, ms, b, lay, n_ops) in cases:
        cfg = EnvironmentConfig(grid_rows=R, grid_cols=C, max_steps=ms, architect_budget=b)
        ops = gen_ops(rng, n_ops, R, C)
        if name == "vault_last_tick":
            ops = [-1, 2, 2, 4, 4, 0, 4, 0]  # vault on tick 6 == max_steps
        if name == "sanity":
            ops = [-1, 4, 4, 4, 4, 4, 4, -1] + ops[1:]
        if name == "empty10":
            ops = [-1] + [2] * 7 + [4] * 7 + [3, -1] + ops[1:]
        rec = run_trace(cfg, lay, ops, n_state, b)
        runs.append((name, cfg, b, lay, ops, rec))
        print("trace %-20s %dx%d valid=%s cams=%d guards=%d ops=%d" % (name, R, C, rec["valid"], rec["n_cams"], rec["n_guards"], len(ops)), flush=True)
    write_traces("env_traces.npz", runs, n_state)


def write_traces(fname, runs, n_state):
    """The env_traces.npz format from (name, cfg, budget, layout, ops, run_trace record) tuples."""
    names, cfgs, valid, layouts, grids, nacc = [], [], [], [], [], []
    ops_all, ops_off = [], [0]
    out = {k: [] for k in ("reward", "done", "status", "pos", "tick", "cam_h", "g_idx", "g_h")}
    vis_bits, state = [], []
    for (name, cfg, b, lay, ops, rec) in runs:
        R, C, ms = cfg.grid_rows, cfg.grid_cols, cfg.max_steps
        names.append(name)
        cfgs.append((R, C, ms, cfg.start_pos[0], cfg.start_pos[1], cfg.vault_pos[0], cfg.vault_pos[1], b))
        valid.append(rec["valid"]); layouts.append(lay); grids.append(rec["grid"].reshape(-1).astype(np.int8))
        nacc.append((rec["n_walls"], rec["n_cams"], rec["n_guards"], rec["spent"]))
        ops_all.extend(ops); ops_off.append(len(ops_all))
        for k in out:
            out[k].extend(rec[k])
        vis_bits.append(np.packbits(np.array(rec["vis"]).reshape(len(ops), -1), axis=1).reshape(-1))
        state.append(np.array(rec["state"], np.float32).reshape(-1))
    arrs = pack_layouts(layouts)
    arrs.update(
        names=np.array(names), cfg=np.array(cfgs, np.int64), valid=np.array(valid, bool),
        grid=np.concatenate(grids), accepted=np.array(nacc, np.int64),
        ops=np.array(ops_all, np.int8), ops_off=np.array(ops_off, np.int64),
        reward=np.array(out["reward"], np.float64), done=np.array(out["done"], bool),
        status=np.array(out["status"], np.int8), pos=np.array(out["pos"], np.int16).reshape(-1, 2),
        tick=np.array(out["tick"], np.int32), cam_h=np.array(out["cam_h"], np.float64),
        g_idx=np.array(out["g_idx"], np.int32), g_h=np.array(out["g_h"], np.float64),
        vis_bits=np.concatenate(vis_bits), state=np.concatenate(state), n_state=np.int64(n_state))
    np.savez_compressed(os.path.join(OUT, fname), **arrs)


# ---------------------------------------------------------------------------
# env traces with start and vault away from the grid corners
# ---------------------------------------------------------------------------

CHOOSE = 9  # an op the policy fills in

# name: (R, C, max_steps, budget, start, vault, layout spec, forced first ops, n_ops, seed)
# layout spec: None = empty, "list" = the placement-rule lists, else synth_layout keywords.
# Vault lane = (vault_r * C + vault_c) & 3: the lane of the observation's float4 the vault is patched into.
OFFCORNER_CASES = [
    ("lane0_mid", 20, 20, 200, 15, (11, 13), (5, 8), {}, [], 120, 1),
    ("lane1_bottom_left", 20, 20, 30, 20, (17, 2), (4, 9), {}, [], 120, 8002),
    ("lane2_top_right", 20, 20, 200, 25, (2, 17), (14, 10), {}, [], 120, 2803),
    ("lane3_adjacent", 20, 20, 200, 15, (8, 11), (7, 11), {}, [], 120, 4),
    ("g32_lane0", 32, 32, 200, 40, (10, 20), (20, 12), {"n_cams": 4, "n_guards": 3}, [], 120, 605),
    ("g32_lane3", 32, 32, 200, 40, (22, 14), (9, 23), {"n_cams": 4, "n_guards": 3}, [], 120, 6),
    ("g13x17", 13, 17, 200, 20, (9, 3), (3, 12), {}, [], 120, 2407),
    ("g16x20", 16, 20, 200, 20, (2, 14), (12, 5), {}, [], 120, 1108),
    ("quad_from_left", 20, 20, 200, 15, (6, 8), (6, 9), None, [4], 60, 9),
    ("quad_from_right", 20, 20, 200, 15, (9, 7), (9, 6), None, [3], 60, 10),
    ("quad_from_above", 20, 20, 200, 15, (10, 4), (11, 4), None, [2], 60, 11),
    ("quad_from_below", 20, 20, 200, 15, (5, 15), (4, 15), None, [1], 60, 12),
    ("start_is_vault", 20, 20, 200, 15, (7, 6), (7, 6), {}, [], 40, 13),
    ("vault_on_border", 20, 20, 200, 15, (15, 9), (19, 5), {}, [], 100, 14),
    ("start_at_origin", 20, 20, 30, 15, (0, 0), (3, 2), {}, [], 80, 15),
    ("placement_lists", 20, 20, 200, 40, (4, 7), (13, 10), "list", [], 100, 916),
]


def offcorner_layout(rng, R, C, budget, start, vault, spec):
    if spec is None:
        return [], [], []
    if spec == "list":
        # walls, cameras and guard patrol starts on the start and vault cells (refused for walls and
        # cameras, environment.py:160-167; guards overwrite the tile, :148) and on (1, 1) and
        # (R-2, C-2), which are ordinary cells here
        walls = [start, vault, (1, 1), (5, 5), (9, 12), (1, 1), (0, 4)]
        cams = [{"row": start[0], "col": start[1], "fov_angle": 60.0},
                {"row": vault[0], "col": vault[1], "fov_angle": 90.0, "heading": 180.0},
                {"row": R - 2, "col": C - 2, "fov_angle": 45.0, "heading": 225.0, "rotation_speed": 10.0},
                {"row": 1, "col": 2, "fov_angle": 75.0, "heading": 90.0, "rotation_speed": 20.0, "vision_range": 5},
                {"row": 1, "col": 1, "fov_angle": 60.0}]
        guards = [{"patrol_path": [start, (start[0], start[1] - 1), (start[0] - 1, start[1] - 1)], "speed": 1,
                   "vision_range": 2, "fov_angle": 60.0},
                  {"patrol_path": [vault, (vault[0] + 1, vault[1]), (vault[0] + 2, vault[1])], "speed": 1,
                   "vision_range": 2, "fov_angle": 60.0},
                  {"patrol_path": [(1, 1), (2, 1)], "speed": 1, "vision_range": 3, "fov_angle": 90.0}]
        return walls, cams, guards
    return synth_layout(rng, R, C, budget, **spec)


def offcorner_policy(rng, vault):
    """Fixed ops stand; a CHOOSE op is, on a finished env, a reset() or (half the time) one more
    step, else steered_action (golden_data.py)."""
    sys.path.insert(0, os.path.dirname(OUT))
    from golden_data import steered_action

    def policy(env, k, op):
        if op != CHOOSE:
            return op
        if env.done:
            return -1 if rng.random() < 0.5 else int(rng.integers(0, 5))
        return steered_action(rng, env.solver_pos, vault)
    return policy


def make_env_traces_offcorner():
    n_state = 24
    runs, seen = [], {}
    for (name, R, C, ms, b, start, vault, spec, first, n_ops, seed) in OFFCORNER_CASES:
        rng = np.random.default_rng(20261000 + seed)
        lay = offcorner_layout(rng, R, C, b, start, vault, spec)
        cfg = EnvironmentConfig(grid_rows=R, grid_cols=C, max_steps=ms, start_pos=start, vault_pos=vault,
                                architect_budget=b)
        assert n_ops <= 120
        template = [-1] + first + [CHOOSE] * (n_ops - 1 - len(first))
        rec = run_trace(cfg, lay, template, n_state, b, policy=offcorner_policy(rng, vault))
        ops = rec["ops"]
        st = np.array(rec["status"])
        counts = {k: int((st == v).sum()) for k, v in STATUS.items()}
        for k, v in counts.items():
            if v:
                seen.setdefault(k, []).append(name)
        runs.append((name, cfg, b, lay, ops, rec))
        print("trace %-18s %dx%d start=%s vault=%s lane=%d valid=%s walls=%d cams=%d guards=%d ops=%d | vault_reached %d "
              "detected %d timeout %d already_done %d resets %d"
              % (name, R, C, start, vault, (vault[0] * C + vault[1]) & 3, rec["valid"], rec["n_walls"], rec["n_cams"],
                 rec["n_guards"], len(ops), counts["vault_reached"], counts["detected"], counts["timeout"],
                 counts["already_done"], counts["reset"]), flush=True)
        if rec["valid"] and start != vault and ms > 30:
            assert counts["vault_reached"] >= 1, name + ": the vault was never reached, choose another seed"
    for k in ("vault_reached", "detected", "timeout"):
        print("status %-13s in %d traces: %s" % (k, len(seen.get(k, [])), " ".join(seen.get(k, []))), flush=True)
        assert len(seen.get(k, [])) >= 2, k
    write_traces("env_traces_offcorner.npz", runs, n_state)
    size = os.path.getsize(os.path.join(OUT, "env_traces_offcorner.npz"))
    print("env_traces_offcorner.npz: %d bytes" % size, flush=True)
    assert size < 1 << 20


# ---------------------------------------------------------------------------
# cone sweeps and BFS
# ---------------------------------------------------------------------------

def make_cones():
    rng = np.random.default_rng(7)
    rows = []  # kind, R, C, r, c, fov, heading, range, wall_density, seed
    vis = []
    walls_all = []
    for i in range(1500):
        R, C = [(20, 20), (32, 32), (10, 10), (13, 21)][i % 4]
        dens = [0.0, 0.1, 0.25][i % 3]
        wm = rng.random((R, C)) < dens
        wm[0, :] = wm[-1, :] = wm[:, 0] = wm[:, -1] = True
        r, c = int(rng.integers(1, R - 1)), int(rng.integers(1, C - 1))
        wm[r, c] = False
        kind = i % 3  # 0 camera f32 params, 1 camera integer params, 2 guard
        if kind == 0:
            fov, head = f32(rng.uniform(30, 120)), f32(rng.uniform(0, 360))
            rngv = int(rng.choice([4, 6, 8]))
        elif kind == 1:
            fov = float(rng.choice([30, 45, 60, 75, 90, 120]))
            head = float(rng.integers(0, 72) * 5) - (360.0 if rng.random() < 0.1 else 0.0)
            rngv = int(rng.choice([4, 6, 8]))
        else:
            fov = float(rng.choice([90.0, 60.0, 120.0, 45.0]))
            head = float(rng.choice([0.0, 90.0, 180.0, 270.0, 135.0, 26.565051177077994]))
            rngv = int(rng.choice([3, 4, 5]))
        if kind < 2:
            tiles = Camera(row=r, col=c, fov_angle=fov, heading=head, vision_range=rngv).get_vision_cone_tiles(R, C, wm)
        else:
            tiles = Guard(patrol_path=[(r, c)], vision_range=rngv, fov_angle=fov, heading=head).get_visible_tiles(R, C, wm)
        v = np.zeros((R, C), bool)
        for (tr, tc) in tiles:
            v[tr, tc] = True
        rows.append((kind, R, C, r, c, rngv))
        vis.append((fov, head))
        walls_all.append(np.packbits(wm.reshape(-1)))
        walls_all[-1] = (walls_all[-1], np.packbits(v.reshape(-1)))
    np.savez_compressed(os.path.join(OUT, "cones.npz"), meta=np.array(rows, np.int64), params=np.array(vis, np.float64),
                        walls=np.concatenate([w for w, _ in walls_all]), tiles=np.concatenate([t for _, t in walls_all]))


def make_cone_order():
    """The LIST order of get_vision_cone_tiles / get_visible_tiles (first visit by ray, then
    by distance): per case the ordered flat tile indices r * C + c."""
    rng = np.random.default_rng(17)
    rows, vis, walls, order, lens = [], [], [], [], []
    for i in range(600):
        R, C = [(20, 20), (32, 32), (10, 10), (13, 21)][i % 4]
        dens = [0.0, 0.1, 0.25][i % 3]
        wm = rng.random((R, C)) < dens
        wm[0, :] = wm[-1, :] = wm[:, 0] = wm[:, -1] = True
        r, c = int(rng.integers(1, R - 1)), int(rng.integers(1, C - 1))
        wm[r, c] = False
        kind = i % 3  # 0 camera f32 params, 1 camera integer params, 2 guard
        if kind == 0:
            fov, head = f32(rng.uniform(30, 120)), f32(rng.uniform(0, 360))
            rngv = int(rng.choice([4, 6, 8]))
        elif kind == 1:
            fov = float(rng.choice([30, 45, 60, 75, 90, 120]))
            head = float(rng.integers(0, 72) * 5)
            rngv = int(rng.choice([4, 6]))
        else:
            fov = float(rng.choice([90.0, 60.0, 120.0]))
            head = float(rng.choice([0.0, 90.0, 180.0, 270.0, 135.0]))
            rngv = int(rng.choice([3, 4, 5]))
        if kind < 2:
            tiles = Camera(row=r, col=c, fov_angle=fov, heading=head, vision_range=rngv).get_vision_cone_tiles(R, C, wm)
        else:
            tiles = Guard(patrol_path=[(r, c)], vision_range=rngv, fov_angle=fov, heading=head).get_visible_tiles(R, C, wm)
        rows.append((1 if kind == 2 else 0, R, C, r, c, rngv))
        vis.append((fov, head))
        walls.append(np.packbits(wm.reshape(-1)))
        order.extend(tr * C + tc for tr, tc in tiles)
        lens.append(len(tiles))
    np.savez_compressed(os.path.join(OUT, "cone_order.npz"), meta=np.array(rows, np.int64),
                        params=np.array(vis, np.float64), walls=np.concatenate(walls),
                        order=np.array(order, np.int32), lens=np.array(lens, np.int32))


def make_bfs():
    rng = np.random.default_rng(11)
    meta, grids, res = [], [], []
    for i in range(3000):
        R, C = [(20, 20), (10, 10), (32, 32), (7, 19)][i % 4]
        g = create_empty_grid(R, C)
        dens = rng.uniform(0.05, 0.55)
        m = rng.random((R, C)) < dens
        g[m] = TileType.WALL
        g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = TileType.WALL
        start, goal = (1, 1), (R - 2, C - 2)
        if i % 10 == 0:
            start = goal
        if i % 7 == 0:
            g[rng.integers(1, R - 1), rng.integers(1, C - 1)] = TileType.GUARD
        g[start] = TileType.START if i % 5 else TileType.WALL  # start tile itself never checked
        g[goal] = TileType.VAULT
        meta.append((R, C, start[0], start[1], goal[0], goal[1]))
        grids.append(g.reshape(-1).astype(np.int8))
        res.append(bfs_path_exists(g, start, goal))
    np.savez_compressed(os.path.join(OUT, "bfs.npz"), meta=np.array(meta, np.int64), grids=np.concatenate(grids), valid=np.array(res, bool))


def serpentine(R, C, by_rows, far_end_first):
    """Every odd line (row if by_rows, else column) but the last is a wall with one gap, at
    alternating ends: one corridor that sweeps the whole grid.  Returns (grid, gap cells)."""
    g = np.zeros((R, C) if by_rows else (C, R), np.int8)
    n_lines, length = g.shape
    gaps = []
    for k, line in enumerate(range(1, n_lines - 1, 2)):
        g[line, :] = TileType.WALL
        at = length - 1 if (k % 2 == 0) == far_end_first else 0
        g[line, at] = TileType.EMPTY
        gaps.append((line, at) if by_rows else (at, line))
    return (g if by_rows else np.ascontiguousarray(g.T)), gaps


def make_bfs_edges():
    """bfs_path_exists where bfs.npz does not go: 64-wide and 64-high grids (bit 63, lane 63), thin
    grids, endpoints in the last row or column, wall tiles under the endpoints, corridors far
    longer than 4 (R + C) and their plugged twins, dense random fills with nearby endpoints."""
    rng = np.random.default_rng(23)
    meta, grids, res, kinds = [], [], [], []

    def add(kind, g, start, goal):
        R, C = g.shape
        meta.append((R, C, start[0], start[1], goal[0], goal[1]))
        grids.append(g.reshape(-1).astype(np.int8))
        res.append(bool(bfs_path_exists(g, tuple(start), tuple(goal))))
        kinds.append(kind)

    for (R, C) in ((64, 64), (33, 64), (3, 64), (64, 3)):
        for by_rows in (True, False):
            if (by_rows and R < 5) or (not by_rows and C < 5):
                continue
            for far in (True, False):
                g, gaps = serpentine(R, C, by_rows, far)
                # the corridor's two ends: the first line's closed end, the last line's far end
                last = (R - 1) if by_rows else (C - 1)
                n_gaps = len(gaps)
                end_far = (n_gaps % 2 == 1) == far  # the side the last gap is on
                if by_rows:
                    a, b = (0, 0 if far else C - 1), (last, 0 if end_far else C - 1)
                else:
                    a, b = (0 if far else R - 1, 0), (0 if end_far else R - 1, last)
                add("serpentine", g, a, b)
                add("serpentine", g, b, a)
                for _ in range(2):
                    h = g.copy()
                    h[gaps[int(rng.integers(0, n_gaps))]] = TileType.WALL
                    s, t = (a, b) if rng.random() < 0.5 else (b, a)
                    add("plugged", h, s, t)
    n_serp = len(meta)
    for i in range(152):
        R, C = [(64, 64), (3, 64), (64, 3), (33, 64)][i % 4]
        g = np.zeros((R, C), np.int8)
        g[rng.random((R, C)) < rng.uniform(0.35, 0.45)] = TileType.WALL
        other = rng.random((R, C)) < 0.03  # cameras, guards: walkable
        g[other & (g == 0)] = rng.choice([TileType.CAMERA, TileType.GUARD])
        if i % 3 == 0:  # an endpoint in the last row or column
            start = (R - 1, int(rng.integers(0, C))) if i % 2 else (int(rng.integers(0, R)), C - 1)
        else:
            start = (int(rng.integers(0, R)), int(rng.integers(0, C)))
        reach = int(rng.integers(1, 9))
        goal = start
        while goal == start:
            goal = (int(np.clip(start[0] + rng.integers(-reach, reach + 1), 0, R - 1)),
                    int(np.clip(start[1] + rng.integers(-reach, reach + 1), 0, C - 1)))
        g[start] = TileType.START
        g[goal] = TileType.VAULT
        kind = "random"
        if i % 10 == 3:
            g[goal] = TileType.WALL
            kind = "goal_wall"
        elif i % 10 == 5:
            g[start] = TileType.WALL  # the start tile itself is never checked
            kind = "start_wall"
        elif i % 10 == 7:
            goal = start
            g[start] = TileType.WALL if i % 20 == 7 else TileType.START
            kind = "start_is_goal"
        if i % 6 == 1:
            start, goal = goal, start
        add(kind, g, start, goal)
    res_a = np.array(res, bool)
    for k in sorted(set(kinds)):
        sel = np.array([x == k for x in kinds])
        print("bfs_edges %-14s %3d grids, %3d reachable" % (k, sel.sum(), res_a[sel].sum()), flush=True)
    share = res_a.mean()
    print("bfs_edges: %d grids (%d serpentine), reachable share %.2f" % (len(res), n_serp, share), flush=True)
    assert 0.25 <= share <= 0.75
    long_paths = 0
    for (R, C, *_), k, v in zip(meta, kinds, res):
        long_paths += int(k == "serpentine" and v and (R // 2) * C > 4 * (R + C) and (C // 2) * R > 4 * (R + C))
    assert long_paths >= 8
    assert all(res_a[np.array([x == "serpentine" for x in kinds])]) and not any(res_a[np.array([x == "plugged" for x in kinds])])
    path = os.path.join(OUT, "bfs_edges.npz")
    np.savez_compressed(path, meta=np.array(meta, np.int64), grids=np.concatenate(grids), valid=res_a)
    print("bfs_edges.npz: %d bytes" % os.path.getsize(path), flush=True)
    assert os.path.getsize(path) < 1 << 20


# ---------------------------------------------------------------------------
# GAE and PPO loss
# ---------------------------------------------------------------------------

class _StubNet(torch.nn.Module):
    """Returns fixed per-sample logits/values; state[:,0,0,0] is the sample id."""

    def __init__(self, logits, values):
        super().__init__()
        self.L = torch.nn.Parameter(torch.tensor(logits))
        self.V = torch.nn.Parameter(torch.tensor(values).reshape(-1, 1))

    def forward(self, states, hidden=None):
        idx = states[:, 0, 0, 0].long()
        return self.L[idx], self.V[idx], hidden


def make_ppo():
    rng = np.random.default_rng(5)
    agent = SolverAgent(grid_rows=4, grid_cols=4)
    gae_cases = []
    for T in (1, 2, 7, 64, 200, 513):
        r = rng.normal(0, 1, T).astype(np.float32)
        r[rng.random(T) < 0.05] += 10.0
        v = rng.normal(0, 1, T).astype(np.float32)
        d = (rng.random(T) < 0.08).astype(np.float32)
        d[-1] = 1.0 if T % 2 else 0.0
        adv = agent._compute_gae(torch.tensor(r), torch.tensor(v), torch.tensor(d)).numpy()
        ret = adv + v
        an = torch.tensor(adv)
        norm = ((an - an.mean()) / (an.std() + 1e-8)).numpy() if T > 1 else adv
        gae_cases.append((r, v, d, adv, ret, norm))
    loss_cases = []
    for M, scale, clipmix in ((64, 1.0, 0.0), (64, 3.0, 0.5), (17, 0.1, 0.9), (1, 1.0, 0.0), (200, 8.0, 0.3)):
        logits = (rng.normal(0, scale, (M, 5))).astype(np.float32)
        if M > 20:
            logits[0] = [60.0, -60.0, 0.0, 1.0, -1.0]  # forces the probability clamp
        values = rng.normal(0, 1, M).astype(np.float32)
        actions = rng.integers(0, 5, M)
        p = torch.softmax(torch.tensor(logits), -1)
        logp = torch.log(torch.clamp(p.gather(1, torch.tensor(actions)[:, None])[:, 0], 1.1920929e-07, 1 - 1.1920929e-07)).numpy()
        old = (logp + rng.normal(0, 0.3, M) * (rng.random(M) < clipmix + 0.5)).astype(np.float32)
        rewards = rng.normal(0, 1, M).astype(np.float32)
        dones = (rng.random(M) < 0.1)
        dones[-1] = True
        vals_roll = rng.normal(0, 1, M).astype(np.float32)
        # Drive the reference update() with a stub network: one epoch, one minibatch
        # of everything, lr 0 and no clipping so .grad holds d(loss)/d(logits, values).
        ag = SolverAgent(grid_rows=1, grid_cols=1, lr=0.0, max_grad_norm=1e30, ppo_epochs=1, batch_size=10 ** 6)
        ag.network = _StubNet(logits, values)
        ag.optimizer = torch.optim.SGD(ag.network.parameters(), lr=0.0)
        for i in range(M):
            ag.states.append(np.full((1, 1, 1), float(i), np.float32))
            ag.actions.append(int(actions[i])); ag.log_probs.append(float(old[i]))
            ag.values.append(float(vals_roll[i])); ag.rewards.append(float(rewards[i])); ag.dones.append(bool(dones[i]))
        np.random.seed(0)
        m = ag.update()
        adv = ag._compute_gae(torch.tensor(rewards), torch.tensor(vals_roll), torch.tensor(dones.astype(np.float32)))
        ret = (adv + torch.tensor(vals_roll)).numpy()
        adv_n = ((adv - adv.mean()) / (adv.std() + 1e-8)).numpy() if M > 1 else adv.numpy()
        loss_cases.append(dict(logits=logits, values=values, actions=actions.astype(np.int64), old=old,
                               rewards=rewards, dones=dones, vals_roll=vals_roll, adv=adv_n.astype(np.float32),
                               ret=ret.astype(np.float32), pg=m["solver_policy_loss"], vl=m["solver_value_loss"],
                               ent=m["solver_entropy"], dlogits=ag.network.L.grad.numpy().copy(),
                               dvalues=ag.network.V.grad.numpy().reshape(-1).copy()))
    arrs = {}
    for i, (r, v, d, adv, ret, norm) in enumerate(gae_cases):
        arrs.update({"gae%d_r" % i: r, "gae%d_v" % i: v, "gae%d_d" % i: d, "gae%d_adv" % i: adv,
                     "gae%d_ret" % i: ret, "gae%d_norm" % i: norm})
    for i, c in enumerate(loss_cases):
        for k, val in c.items():
            arrs["loss%d_%s" % (i, k)] = np.asarray(val)
    arrs["n_gae"] = np.int64(len(gae_cases)); arrs["n_loss"] = np.int64(len(loss_cases))
    np.savez_compressed(os.path.join(OUT, "ppo.npz"), **arrs)


# ---------------------------------------------------------------------------
# networks and architect decode
# ---------------------------------------------------------------------------

def make_nets():
    arrs = {}
    torch.manual_seed(31)
    sn = SolverNetwork(grid_rows=20, grid_cols=20)
    for k, v in sn.state_dict().items():
        arrs["solver/" + k] = v.numpy()
    x = torch.randn(6, 3, 20, 20)
    h = (torch.randn(1, 6, 128) * 0.5, torch.randn(1, 6, 128) * 0.5)
    with torch.no_grad():
        lg, val, (h1, c1) = sn(x, h)
        lg0, val0, (h0, c0) = sn(x)
    arrs.update({"solver_in": x.numpy(), "solver_h": h[0].numpy(), "solver_c": h[1].numpy(),
                 "solver_logits": lg.numpy(), "solver_value": val.numpy(), "solver_h1": h1.numpy(), "solver_c1": c1.numpy(),
                 "solver_logits0": lg0.numpy(), "solver_value0": val0.numpy()})
    torch.manual_seed(32)
    an = ArchitectNetwork(grid_rows=20, grid_cols=20)
    for k, v in an.state_dict().items():
        arrs["architect/" + k] = v.numpy()
    gs = np.zeros((1, 1, 20, 20), np.float32)
    gs[0, 0, 1, 1] = TileType.START / 5.0
    gs[0, 0, 18, 18] = TileType.VAULT / 5.0
    with torch.no_grad():
        pl, av, cp = an(torch.tensor(gs))
    arrs.update({"arch_in": gs, "arch_logits": pl.numpy(), "arch_value": av.numpy(),
                 "arch_fov": cp["fov"].numpy(), "arch_speed": cp["speed"].numpy(), "arch_heading": cp["heading"].numpy()})
    # decode cases: record the sampled class map by re-running the sampler with the same seed
    dec_meta, dec_maps, dec_out = [], [], []
    rng = np.random.default_rng(3)
    for i in range(40):
        R = C = [20, 10, 32, 20][i % 4]
        budget = int([5, 8, 15, 22, 40, 27][i % 6])
        temp = float([1.0, 0.5, 2.0, 1.3][i % 4])
        net = ArchitectNetwork(grid_rows=R, grid_cols=C)
        with torch.no_grad():
            for p in net.parameters():
                p.add_(torch.randn_like(p) * 0.3)
        g = np.zeros((1, 1, R, C), np.float32)
        seed = 1000 + i
        torch.manual_seed(seed)
        with torch.no_grad():
            walls, cams, guards, tlp, val = net.generate_layout(torch.tensor(g), budget, temp)
        torch.manual_seed(seed)
        with torch.no_grad():
            pl, _, cp = net(torch.tensor(g))
            probs = torch.softmax(pl / temp, dim=1)
            flat = probs.view(1, 4, -1).permute(0, 2, 1)
            sampled = torch.distributions.Categorical(flat).sample()
        amap = sampled.view(R, C).numpy().astype(np.int8)
        dec_meta.append((R, C, budget, len(walls), len(cams), len(guards)))
        dec_maps.append(amap.reshape(-1))
        cam_p = (float(cp["fov"].item()), float(cp["speed"].item()), float(cp["heading"].item()))
        lay = [list(w) for w in walls], [(c["row"], c["col"]) for c in cams], [g_["patrol_path"] for g_ in guards]
        dec_out.append({"cam_params": cam_p, "walls": lay[0], "cams": lay[1], "guards": lay[2],
                        "total_log_prob": float(tlp.item()), "temperature": temp})
    arrs["dec_meta"] = np.array(dec_meta, np.int64)
    arrs["dec_maps"] = np.concatenate(dec_maps)
    np.savez_compressed(os.path.join(OUT, "nets.npz"), **arrs)
    with open(os.path.join(OUT, "architect_decode.json"), "w") as f:
        json.dump(dec_out, f)


def make_kat():
    kat = {}
    cfg = EnvironmentConfig(grid_rows=10, grid_cols=10, start_pos=(1, 1), vault_pos=(8, 8))
    env = HeistEnvironment(cfg)
    valid = env.set_layout([(3, 3), (3, 4), (3, 5)],
                           [{"row": 5, "col": 5, "fov_angle": 60, "heading": 0, "rotation_speed": 15, "vision_range": 4}],
                           [{"patrol_path": [(7, 2), (7, 3), (7, 4), (7, 5)], "speed": 1, "vision_range": 3, "fov_angle": 90}])
    env.reset()
    rews = []
    for _ in range(5):
        _, r, d, info = env.step(4)
        rews.append(r)
        if d:
            break
    kat["sanity"] = {"valid": bool(valid), "pos": list(env.solver_pos), "tick": env.tick, "status": info["status"],
                     "rewards": rews, "surveilled": int(np.sum(env.visibility_map.visibility > 0.5)),
                     "render": env.render_text()}
    env = HeistEnvironment(EnvironmentConfig(grid_rows=10, grid_cols=10))
    env.set_layout([], [], [])
    env.reset()
    tot = 0.0
    for _ in range(7):
        _, r, d, info = env.step(2)
        tot += r
    kat["fixes_down"] = tot
    for _ in range(7):
        _, r, d, info = env.step(4)
        tot += r
        if d:
            break
    kat["fixes_right"] = tot
    kat["fixes_status"] = info["status"]
    env2 = HeistEnvironment(EnvironmentConfig(grid_rows=10, grid_cols=10))
    env2.set_layout([], [], [])
    env2.reset()
    st = env2.get_state_tensor()
    kat["pos_channel_min"] = float(st[2].min())
    kat["pos_channel_max"] = float(st[2].max())
    kat["params"] = {"architect": sum(p.numel() for p in ArchitectNetwork(10, 10).parameters()),
                     "solver": sum(p.numel() for p in SolverNetwork(10, 10).parameters())}
    kat["architect_reward"] = {str(s): RewardCalculator().calculate_architect_reward(env2, s)
                               for s in (0.0, 0.1, 0.2, 0.5, 0.6, 0.7, 0.8, 0.81, 1.0)}
    with open(os.path.join(OUT, "kat.json"), "w") as f:
        json.dump(kat, f, indent=1)


def proj_vectors(i, n, k=4):
    """The fixed projection vectors of parameter tensor i (also used by the tests)."""
    return np.random.default_rng(7000 + i).standard_normal((k, n))


ARCH_CASES = [  # (log_probs, values, rewards) per update; consecutive updates of one agent
    [([-52.5], [0.02], [1.0])],
    [([-61.25], [-0.013], [-1.0])],
    [([-50.0, -55.5, -48.25, -60.0, -51.0], [0.01, 0.01, 0.01, 0.01, 0.01], [1.0, -1.0, 0.7, 0.2, -0.5])],
    [([-53.0], [0.015], [0.6]), ([-58.0], [0.011], [-0.5]), ([-49.5, -50.5], [0.012, 0.012], [1.2, 0.3])],
]


def make_arch_update():
    from heist_architect.agents.architect import ArchitectAgent
    z = np.load(os.path.join(OUT, "nets.npz"), allow_pickle=False)
    sd = {k[len("architect/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("architect/")}
    arrs = {"n_cases": np.int64(len(ARCH_CASES))}
    for ci, case in enumerate(ARCH_CASES):
        ag = ArchitectAgent(grid_rows=20, grid_cols=20, budget=15)
        ag.network.load_state_dict(sd)
        for ui, (lps, vals, rews) in enumerate(case):
            p0 = [p.detach().clone() for p in ag.network.parameters()]
            ag.log_probs = [torch.tensor(x) for x in lps]
            ag.values = [torch.tensor([[x]]) for x in vals]
            ag.rewards = []
            for r in rews:
                ag.store_reward(r)
            m = ag.update()
            key = "c%d_u%d_" % (ci, ui)
            arrs[key + "lp"] = np.array(lps, np.float32)
            arrs[key + "v"] = np.array(vals, np.float32)
            arrs[key + "r"] = np.array(rews, np.float64)
            arrs[key + "loss"] = np.array([m["architect_policy_loss"], m["architect_value_loss"],
                                           m["architect_total_loss"]], np.float64)
            gn, gp, dn, dp = [], [], [], []
            for i, (p, q) in enumerate(zip(ag.network.parameters(), p0)):
                g = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().reshape(-1).numpy()
                d = (p.detach() - q).double().reshape(-1).numpy()
                P = proj_vectors(i, g.size)
                gn.append(np.linalg.norm(g))
                dn.append(np.linalg.norm(d))
                gp.append(P @ g)
                dp.append(P @ d)
            arrs[key + "gnorm"] = np.array(gn)
            arrs[key + "gproj"] = np.array(gp)
            arrs[key + "dnorm"] = np.array(dn)
            arrs[key + "dproj"] = np.array(dp)
        arrs["c%d_n" % ci] = np.int64(len(case))
    np.savez_compressed(os.path.join(OUT, "arch_update.npz"), **arrs)


# ---------------------------------------------------------------------------
# the Solver's whole PPO update
# ---------------------------------------------------------------------------

# name: (grid, transitions, epochs, batch, architect budget, max_steps, layouts, seed, head scale)
UPDATE_CASES = {
    "g20": (20, 129, 3, 64, 15, 14, 4, 410, 1.0),
    "g32": (32, 86, 3, 64, 27, 14, 3, 411, 1.0),
    "g10": (10, 70, 3, 64, 5, 9, 3, 412, 1.0),
    "clip20": (20, 129, 3, 64, 15, 14, 4, 413, 2.8e5),
    "big20": (20, 4099, 1, 4099, 15, 30, 16, 414, 1.0),
}


def _fill_solver_buffer(ag, R, T, budget, max_steps, n_layouts, seed):
    """Reference episodes on Architect layouts through select_action / store_transition until
    the buffer holds T transitions (the last episode is cut there)."""
    lays = architect_layouts(n_layouts, R, R, budget, seed)
    torch.manual_seed(seed + 1000)
    envs = []
    for lay in lays:
        env = HeistEnvironment(EnvironmentConfig(grid_rows=R, grid_cols=R, max_steps=max_steps, architect_budget=budget))
        env.budget.scale_budget(budget)
        if env.set_layout(*lay):
            envs.append(env)
    assert envs, "no valid layout"
    k = 0
    while len(ag.rewards) < T:
        env = envs[k % len(envs)]
        k += 1
        env.reset()
        ag.reset()
        done, total = False, 0.0
        while not done and len(ag.rewards) < T:
            a = ag.select_action(env.get_state_tensor())
            _, r, done, _ = env.step(a)
            ag.store_transition(r, done)
            total += r
        ag.end_episode(total)


def make_solver_update(only=None):
    """tests/golden/solver_update_<case>.npz: the reference SolverAgent.update() on real buffers."""
    sys.path.insert(0, os.path.dirname(OUT))
    import solver_update_ref as sr
    import heist_architect.agents.solver as solver_mod
    from types import SimpleNamespace

    for name, (R, T, epochs, batch, budget, max_steps, n_lay, seed, scale) in UPDATE_CASES.items():
        if only and name not in only:
            continue
        torch.manual_seed(seed)
        ag = SolverAgent(grid_rows=R, grid_cols=R, ppo_epochs=epochs, batch_size=batch)
        sd = sr.golden_params(scale)
        ag.network.load_state_dict(sd)
        _fill_solver_buffer(ag, R, T, budget, max_steps, n_lay, seed)
        rng = np.random.default_rng(seed)
        if name == "clip20":  # stale old log-probs on a random third of the rows (as make_ppo)
            lp = np.array(ag.log_probs, np.float32)
            lp = (lp + rng.normal(0, 0.3, T) * (rng.random(T) < 1.0 / 3.0)).astype(np.float32)
            ag.log_probs = [float(v) for v in lp]
        states = np.array(ag.states, np.float32)
        actions = np.array(ag.actions, np.int64)
        logp, values = np.array(ag.log_probs, np.float32), np.array(ag.values, np.float32)
        rewards, dones = np.array(ag.rewards, np.float32), np.array(ag.dones, bool)
        assert len(states) == T and dones.sum() >= 3, (len(states), dones.sum())
        occ, lay, vis, pos = sr.encode_states(states, R, R)
        assert np.array_equal(sr.decode_states(occ, lay, vis, pos, R, R).view(np.uint32), states.view(np.uint32)), \
            "state coding does not round-trip"
        perms = np.stack([rng.permutation(T) for _ in range(epochs)]).astype(np.int32)
        n_mb = (T + batch - 1) // batch
        n_steps = epochs * n_mb
        # recorded steps: the first, the first short (tail) minibatch, the last
        rec = sorted({0, n_mb - 1, n_steps - 1}) if T % batch and n_mb > 1 else [0]

        # float64 restatement first (its ReLU signs are compared with the reference's as it runs)
        r64 = sr.run_update(sd, states, actions, logp, values, rewards, dones.astype(np.float32), perms, epochs, batch,
                            record=rec, keep_signs=True)
        assert r64["n_steps"] == n_steps

        recorded, flips, state = {}, [], {"step": 0, "perm": 0, "k": 0}
        real_clip = torch.nn.utils.clip_grad_norm_

        def clip(parameters, max_norm, *a, **kw):
            parameters = list(parameters)
            s = state["step"]
            grads = [p.grad.detach().clone() for p in parameters]
            total = real_clip(parameters, max_norm, *a, **kw)
            if s in rec:
                # the step's loss parts are locals of the reference's update(): this relies on
                # update() calling clip_grad_norm_ directly and on those three names
                loc = sys._getframe(1).f_locals
                recorded[s] = dict(grads=grads, total=float(total),
                                   parts=np.array([float(loc["policy_loss"]), float(loc["value_loss"]), float(loc["entropy"])]))
            state["step"] += 1
            state["k"] = 0
            return total

        def replay(n):
            assert n == T
            state["perm"] += 1
            return perms[state["perm"] - 1].astype(np.int64)

        def sign_hook(mod, inp, out):
            if state["k"] == 0:
                flips.append([0, 0])
            own = r64["signs"][state["step"]][state["k"]]
            flips[-1][0] += int(((out.detach() > 0) != own).sum())
            flips[-1][1] += own.numel()
            state["k"] += 1

        class _NN:  # the reference module's `nn`, with clip_grad_norm_ wrapped
            utils = SimpleNamespace(clip_grad_norm_=clip)

            def __getattr__(self, k):
                return getattr(torch.nn, k)

        hooks = [m.register_forward_hook(sign_hook) for m in (ag.network.conv1, ag.network.conv2, ag.network.conv3)]
        real_perm, real_nn = np.random.permutation, solver_mod.nn
        np.random.permutation, solver_mod.nn = replay, _NN()
        try:
            metrics = ag.update()
        finally:
            np.random.permutation, solver_mod.nn = real_perm, real_nn
            for hk in hooks:
                hk.remove()
        assert state["step"] == n_steps and state["perm"] == epochs and not ag.states
        after = dict(ag.network.named_parameters())
        assert list(after) == list(sr.PARAMS)

        adv = ag._compute_gae(torch.tensor(rewards), torch.tensor(values), torch.tensor(dones.astype(np.float32)))
        ret = (adv + torch.tensor(values)).numpy()
        adv_n = ((adv - adv.mean()) / (adv.std() + 1e-8)).numpy()

        arrs = dict(cfg=np.array([R, R, T, epochs, batch], np.int64), head_scale=np.float64(scale),
                    hyper=np.array([sr.HYPER[k] for k in ("lr", "gamma", "lam", "clip", "ecoef", "vcoef", "max_norm")]),
                    occ=occ, lay=lay, vis=vis, pos=pos, actions=actions.astype(np.int8), logp=logp, values=values,
                    rewards=rewards, dones=dones, perms=perms, adv=adv_n.astype(np.float32), ret=ret.astype(np.float32),
                    metrics=np.array([metrics["solver_policy_loss"], metrics["solver_value_loss"],
                                      metrics["solver_entropy"]], np.float64),
                    n_steps=np.int64(n_steps), rec_steps=np.array(rec, np.int64),
                    flips=np.array(flips, np.int64))

        def pack(tensors, key):  # conv tensors in full, every tensor's norm + 4 projections
            t64 = [t.detach().double().reshape(-1).numpy() for t in tensors]
            arrs[key + "conv"] = np.concatenate(t64[:sr.N_CONV]).astype(np.float32)
            arrs[key + "norm"] = np.array([np.linalg.norm(t) for t in t64])
            arrs[key + "proj"] = np.array([sr.proj_vectors(i, t.size) @ t for i, t in enumerate(t64)])

        # the reference's own fp32 noise against float64: the tests' floors
        f_max, f_l2, f_tot = [], [], []
        for s in rec:
            g32 = recorded[s]["grads"]
            g64 = [r64["steps"][s]["grads"][k] for k in sr.PARAMS]
            pack(g32, "s%d_g" % s)
            arrs["s%d_total" % s] = np.float64(recorded[s]["total"])
            arrs["s%d_parts" % s] = recorded[s]["parts"]
            f_max.append([sr.rel_max(a.double().numpy(), b.numpy()) if i != sr.HH else 0.0
                          for i, (a, b) in enumerate(zip(g32, g64))])
            f_l2.append([sr.rel_l2(a.double().numpy(), b.numpy()) if i != sr.HH else 0.0
                         for i, (a, b) in enumerate(zip(g32, g64))])
            f_tot.append(abs(recorded[s]["total"] - r64["steps"][s]["total_norm"]) / r64["steps"][s]["total_norm"])
            assert not g32[sr.HH].any() and not g64[sr.HH].any()
            assert np.abs(recorded[s]["parts"] - r64["steps"][s]["parts"]).max() <= 1e-5, s
        d32 = [after[k].detach().double() - sd[k].double() for k in sr.PARAMS]
        d64 = [r64["params"][k] - sd[k].double() for k in sr.PARAMS]
        pack(d32, "d_")
        f_d = [sr.rel_l2(a.numpy(), b.numpy()) if i != sr.HH else 0.0 for i, (a, b) in enumerate(zip(d32, d64))]
        assert not d32[sr.HH].any() and not d64[sr.HH].any()
        arrs.update(floor_grad_max=np.array(f_max), floor_grad_l2=np.array(f_l2), floor_total=np.array(f_tot),
                    floor_delta=np.array(f_d), floor_metrics=np.abs(arrs["metrics"] - r64["metrics"]))
        flip_share = max(f / n for f, n in flips)
        print("%-6s T=%d steps=%d rec=%s dones=%d layouts=%d | ref fp32 vs float64: grad/max %.2g grad/L2 %.2g "
              "total %.2g delta/L2 %.2g (scaled heads %.2g) metrics %.2g ReLU sign share %.2g (%d flips) | entropy %.4f total norm %.3g"
              % (name, T, n_steps, rec, dones.sum(), len(occ), np.max(f_max), np.max(f_l2), np.max(f_tot),
                 max(v for i, v in enumerate(f_d) if scale == 1.0 or sr.PARAMS[i] not in sr.SCALED),
                 max(f_d[sr.PARAMS.index(k)] for k in sr.SCALED),
                 arrs["floor_metrics"].max(), flip_share, sum(f for f, _ in flips), recorded[0]["parts"][2],
                 recorded[0]["total"]), flush=True)
        # a head layer scaled to |w| ~ 1e2 .. 3e3 moves by about one float32 spacing of w per Adam
        # step (lr 3e-4): its change is stored in full and held element by element to half a
        # spacing per step (round to nearest), not to 1e-4 in relative L2
        coarse = [sr.PARAMS.index(k) for k in sr.SCALED] if scale != 1.0 else []
        if coarse:
            arrs["d_heads"] = np.concatenate([d32[i].reshape(-1).numpy() for i in coarse])
            for i, (want, allowed) in sr.coarse_delta(arrs, sd, 0.5 * n_steps).items():
                assert np.array_equal(want, d32[i].reshape(-1).numpy())
                assert float((np.abs(d64[i].reshape(-1).numpy() - want) / allowed).max()) <= 1.0, (name, sr.PARAMS[i])
        fine = [v for i, v in enumerate(f_d) if i not in coarse]
        # a single Adam step is lr * g / (|g| + 1e-8): sign-like, so an element whose gradient lies
        # within fp32 noise of 0 moves by up to 2 lr either way (several steps average this out)
        assert np.max(f_max) <= 1e-4 and np.max(fine) <= (1e-4 if n_steps > 1 else 1e-3) and flip_share <= 1e-5
        assert np.abs(adv_n - r64["adv"].numpy()).max() <= 1e-5 and np.abs(ret - r64["ret"].numpy()).max() <= 1e-5
        if name == "clip20":
            ratio = r64["steps"][0]["ratio"].numpy()
            out = float(((ratio < 0.8) | (ratio > 1.2)).mean())
            print("clip20: %.0f %% of the first minibatch's ratios outside [0.8, 1.2]" % (100 * out))
            assert 0.10 <= out <= 0.60 and recorded[0]["parts"][2] < 1.55
        path = os.path.join(OUT, "solver_update_%s.npz" % name)
        np.savez_compressed(path, **arrs)
        print("   %s: %d bytes" % (os.path.basename(path), os.path.getsize(path)), flush=True)
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    which = sys.argv[1:] or ["kat", "bfs", "cones", "ppo", "nets", "env", "arch", "order", "update", "offcorner",
                             "bfs_edges"]
    makers = {"kat": make_kat, "bfs": make_bfs, "cones": make_cones, "ppo": make_ppo,
              "nets": make_nets, "env": make_env_traces, "arch": make_arch_update, "order": make_cone_order,
              "update": make_solver_update, "offcorner": make_env_traces_offcorner, "bfs_edges": make_bfs_edges}
    for w in which:
        print("==", w, flush=True)
        if w.startswith("update:"):  # update:g20,clip20 -- some cases only
            make_solver_update(w[len("update:"):].split(","))
        else:
            makers[w]()
