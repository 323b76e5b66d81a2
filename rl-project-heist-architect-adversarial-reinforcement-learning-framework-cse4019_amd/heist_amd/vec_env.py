"""HeistEnv -- N independent Heist environments stepped by one HIP launch.

This is the batched form of the reference's HeistEnvironment (environment.py:40-426):
set_layout / reset / step have the same semantics per env, the observation is the
reference's get_state_tensor() stacked as [N, 3, R, C] float32, and all state stays
in HBM.  Layout lists in the reference's dict format are packed by LayoutBatch.
"""
import ctypes
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native as nat

STATUS_NAMES = {0: "running", 1: "detected", 2: "vault_reached", 3: "timeout", 4: "already_done"}
STATUS_CODES = {v: k for k, v in STATUS_NAMES.items()}

Layout = Tuple[Sequence[Tuple[int, int]], Sequence[dict], Sequence[dict]]


@dataclass
class LayoutBatch:
    """Padded device arrays for heist_set_layout (see include/heist.h)."""
    wall_rc: torch.Tensor      # [N, max_walls, 2] int32
    n_walls: torch.Tensor      # [N] int32
    cam_params: torch.Tensor   # [N, max_cams, 6] float64
    n_cams: torch.Tensor       # [N] int32
    guard_paths: torch.Tensor  # [N, max_guards, max_path, 2] int32
    guard_meta: torch.Tensor   # [N, max_guards, 3] int32
    guard_fov: torch.Tensor    # [N, max_guards] float64
    n_guards: torch.Tensor     # [N] int32
    budget: torch.Tensor       # [N] int32

    @property
    def max_walls(self) -> int:
        return int(self.wall_rc.shape[1])

    @staticmethod
    def from_lists(layouts: Sequence[Layout], budget: Union[int, Sequence[int]], max_cams: int, max_guards: int,
                   max_path: int, device, rows: int = 64, cols: int = 64) -> "LayoutBatch":
        n = len(layouts)
        mw = max(1, max((len(w) for w, _, _ in layouts), default=0))
        W = np.zeros((n, mw, 2), np.int32)
        nw = np.zeros(n, np.int32)
        CP = np.zeros((n, max(1, max_cams), 6), np.float64)
        nc = np.zeros(n, np.int32)
        GP = np.zeros((n, max(1, max_guards), max_path, 2), np.int32)
        GM = np.zeros((n, max(1, max_guards), 3), np.int32)
        GF = np.zeros((n, max(1, max_guards)), np.float64)
        ng = np.zeros(n, np.int32)
        for e, (walls, cams, guards) in enumerate(layouts):
            if len(cams) > max_cams or len(guards) > max_guards:
                raise ValueError("env %d: %d cameras / %d guards exceed capacity %d / %d"
                                 % (e, len(cams), len(guards), max_cams, max_guards))
            nw[e] = len(walls)
            for i, (r, c) in enumerate(walls):
                W[e, i] = (r, c)
            nc[e] = len(cams)
            for i, cd in enumerate(cams):  # environment.py:127-133 defaults
                CP[e, i] = (cd["row"], cd["col"], cd.get("fov_angle", 60.0), cd.get("heading", 0.0),
                            cd.get("rotation_speed", 15.0), cd.get("vision_range", 6))
            ng[e] = len(guards)
            for i, gd in enumerate(guards):  # environment.py:141-146 defaults
                path = list(gd["patrol_path"])
                if len(path) > max_path:
                    raise ValueError("env %d guard %d: patrol path of %d points exceeds max_path %d"
                                     % (e, i, len(path), max_path))
                for k, (r, c) in enumerate(path):
                    if not (0 <= r < rows and 0 <= c < cols):
                        raise ValueError("env %d guard %d: patrol point %s outside the %dx%d grid"
                                         % (e, i, (r, c), rows, cols))
                    GP[e, i, k] = (r, c)
                GM[e, i] = (len(path), gd.get("speed", 1), gd.get("vision_range", 4))
                GF[e, i] = gd.get("fov_angle", 90.0)
        b = np.broadcast_to(np.asarray(budget, np.int32), (n,)).copy()
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
        return LayoutBatch(t(W), t(nw), t(CP), t(nc), t(GP), t(GM), t(GF), t(ng), t(b))


def _layout_to_lists(lb: "LayoutBatch"):
    W, nw, CP, nc, GP, GM, GF, ng = (t.cpu().numpy() for t in (lb.wall_rc, lb.n_walls, lb.cam_params, lb.n_cams,
                                                              lb.guard_paths, lb.guard_meta, lb.guard_fov, lb.n_guards))
    out = []
    for e in range(len(nw)):
        walls = [(int(r), int(c)) for r, c in W[e, :nw[e]]]
        cams = [{"row": int(c[0]), "col": int(c[1]), "fov_angle": float(c[2]), "rotation_speed": float(c[4]),
                 "heading": float(c[3]), "vision_range": int(c[5])} for c in CP[e, :nc[e]]]
        guards = [{"patrol_path": [(int(r), int(c)) for r, c in GP[e, i, :GM[e, i, 0]]], "speed": int(GM[e, i, 1]),
                   "vision_range": int(GM[e, i, 2]), "fov_angle": float(GF[e, i])} for i in range(ng[e])]
        out.append((walls, cams, guards))
    return out


LayoutBatch.to_lists = _layout_to_lists


@dataclass
class PlanResult:
    """HeistEnv.plan's output (heist_plan, include/heist.h), device tensors:
    ticks [N] int32 -- the fewest ticks to a clean vault arrival, -1 when there is none in reach;
    actions [H, N] int64 -- the canonical plan in rows 0 .. ticks - 1, 0 elsewhere: feed it (or
        its first rows) to step_multi / step_multi_records with auto_reset=False;
    reach [H, N, W] int32 -- row k - 1: the cells the Solver can occupy, live and unseen, after k
        ticks, in the compact record's bit order (bit i of word j is cell 32 j + i)."""
    ticks: torch.Tensor
    actions: torch.Tensor
    reach: torch.Tensor
    rows: int
    cols: int

    def reach_mask(self, k: int) -> torch.Tensor:
        """reach_k for k = 1 .. H as bool [N, R, C]."""
        if not 1 <= k <= self.reach.shape[0]:
            raise IndexError("reach_mask: k must be 1 .. %d" % self.reach.shape[0])
        w = self.reach[k - 1]
        sh = torch.arange(32, device=w.device, dtype=torch.int32)
        bits = (w.unsqueeze(-1) >> sh) & 1
        return bits.reshape(w.shape[0], -1)[:, :self.rows * self.cols].reshape(-1, self.rows, self.cols).bool()


@dataclass
class PlanField:
    """HeistEnv.plan_field's output (heist_plan_field, include/heist.h), device tensors:
    togo [N, R, C] int16 -- the fewest ticks to a clean vault arrival from every cell as the env
        stands now (what plan() gives with the Solver on that cell), -1 where there is none;
    action [N, R, C] int8 -- the lowest action that attains it, -1 where togo is -1;
    vis [H, N, W] int32 -- row k - 1: the visibility plane of the env's k-th tick from now, in the
        compact record's bit order (bit i of word j is cell 32 j + i), 0 past the env's ticks;
    togo_ticks [H, N, R, C] int16 or None -- row k: the same field k ticks from now (row 0 equals
        togo), -1 past the env's ticks; with all_ticks=True only;
    vault -- the vault's (row, col), which heist_amd.search.follow_field / expert_labels need."""
    togo: torch.Tensor
    action: torch.Tensor
    vis: torch.Tensor
    togo_ticks: Optional[torch.Tensor]
    rows: int
    cols: int
    vault: Optional[Tuple[int, int]] = None

    def vis_mask(self, k: int) -> torch.Tensor:
        """vis_k for k = 1 .. H as bool [N, R, C]."""
        if not 1 <= k <= self.vis.shape[0]:
            raise IndexError("vis_mask: k must be 1 .. %d" % self.vis.shape[0])
        w = self.vis[k - 1]
        sh = torch.arange(32, device=w.device, dtype=torch.int32)
        bits = (w.unsqueeze(-1) >> sh) & 1
        return bits.reshape(w.shape[0], -1)[:, :self.rows * self.cols].reshape(-1, self.rows, self.cols).bool()


@dataclass
class PlanValue:
    """HeistEnv.plan_value's output (heist_plan_value, include/heist.h), device tensors:
    value [N, R, C] float64 -- the largest discounted return (the env's own reward64, summed from
        the back: r_k + gamma * (...)) a Solver on that cell can still collect as the env stands
        now; 0.0 on wall cells and in an env already done;
    action [N, R, C] int8 -- the lowest action that attains it, -1 where there is none to take;
    vis [H, N, W] int32 -- PlanField.vis: row k - 1 is the visibility plane of the k-th tick from now;
    value_ticks [H, N, R, C] float64 or None -- row k: the same values k ticks from now (row 0
        equals value), 0.0 past the env's ticks; with all_ticks=True only.  8 H N R C bytes:
        2.6 GB for 4,096 envs of 20 x 20 at H = 200;
    action_ticks [H, N, R, C] int8 or None -- row k: the optimal action of step k, -1 past the
        env's ticks; with all_ticks=True only;
    vault -- the vault's (row, col); gamma -- the discount the values were computed with;
    grid [N, R, C] int8 -- the tile map (export(grid=True)), whose walls
        heist_amd.search.follow_value moves by;
    tick [N] int32 or None -- each env's tick when the tables were made, -1 where it was done
        then: HeistEnv.plan_q's tick0, which labels a rollout after the handle has been stepped."""
    value: torch.Tensor
    action: torch.Tensor
    vis: torch.Tensor
    value_ticks: Optional[torch.Tensor]
    action_ticks: Optional[torch.Tensor]
    rows: int
    cols: int
    vault: Optional[Tuple[int, int]] = None
    gamma: float = 1.0
    grid: Optional[torch.Tensor] = None
    tick: Optional[torch.Tensor] = None

    vis_mask = PlanField.vis_mask


@dataclass
class PlanMasked:
    """HeistEnv.plan_masked's output (heist_plan_masked, include/heist.h), device tensors; variant
    (e, m) is env e planned with the emitter slots of masks[e, m] alone:
    ticks [N, M] int16 -- the fewest ticks to a clean vault arrival from the Solver's cell (-1: none);
    value [N, M] float64, action [N, M] int8 -- the largest discounted return from there and the
        lowest action that starts it (PlanValue's at that cell);
    vis [H, N, M, W] int32 -- row k - 1: the variant's visibility plane of the k-th tick from now;
    togo_cells [N, M, R, C] int16, value_cells [N, M, R, C] float64 or None -- the whole tables
        (PlanField.togo / PlanValue.value of the variant); with cells=True only;
    masks [N, M] int64 -- the masks as given (bit j: slot j is live; slot 63 is the sign bit);
    tick [N] int32 -- each env's tick at the call, -1 where it was done (PlanValue.tick)."""
    ticks: torch.Tensor
    value: torch.Tensor
    action: torch.Tensor
    vis: torch.Tensor
    togo_cells: Optional[torch.Tensor]
    value_cells: Optional[torch.Tensor]
    masks: torch.Tensor
    tick: torch.Tensor
    rows: int
    cols: int
    gamma: float = 1.0

    def vis_mask(self, k: int, m: int = 0) -> torch.Tensor:
        """vis_k of variant m for k = 1 .. H as bool [N, R, C]."""
        if not 1 <= k <= self.vis.shape[0]:
            raise IndexError("vis_mask: k must be 1 .. %d" % self.vis.shape[0])
        w = self.vis[k - 1, :, m]
        sh = torch.arange(32, device=w.device, dtype=torch.int32)
        bits = (w.unsqueeze(-1) >> sh) & 1
        return bits.reshape(w.shape[0], -1)[:, :self.rows * self.cols].reshape(-1, self.rows, self.cols).bool()


@dataclass
class PlanPlace:
    """HeistEnv.plan_place's output (heist_plan_place, include/heist.h), device tensors; variant
    (e, m) is env e with the candidate camera cands[e, m] added to the base rows:
    valid [N, M] bool -- the candidate is placeable in the grid as it stands and its parameters are
        ones the raycaster takes; an invalid candidate's variant is the base rows' plan;
    ticks [N, M] int16 -- the fewest ticks to a clean vault arrival from the Solver's cell (-1: none);
    value [N, M] float64, action [N, M] int8 -- the largest discounted return from there and the
        lowest action that starts it (PlanValue's at that cell);
    vis [H, N, M, W] int32 -- row k - 1: the variant's visibility plane of the k-th tick from now,
        4 H N M W bytes;
    togo_cells [N, M, R, C] int16, value_cells [N, M, R, C] float64 or None -- the whole tables
        (PlanField.togo / PlanValue.value of the variant); with cells=True only;
    cands [N, M, 6] float64 -- the candidates as given (row, col, fov_angle, heading,
        rotation_speed, vision_range);
    tick [N] int32 -- each env's tick at the call, -1 where it was done (PlanValue.tick)."""
    valid: torch.Tensor
    ticks: torch.Tensor
    value: torch.Tensor
    action: torch.Tensor
    vis: torch.Tensor
    togo_cells: Optional[torch.Tensor]
    value_cells: Optional[torch.Tensor]
    cands: torch.Tensor
    tick: torch.Tensor
    rows: int
    cols: int
    gamma: float = 1.0

    vis_mask = PlanMasked.vis_mask


@dataclass
class PlanWalls:
    """HeistEnv.plan_walls's output (heist_plan_walls, include/heist.h), device tensors; variant
    (e, m) is env e with the tile edits edits[e, m] applied, under the emitter slots of masks[e, m]:
    valid [N, M] bool -- every edit of the variant holds in the grid as it stands (an add on an
        interior EMPTY tile that is not the Solver's cell, a remove of an interior WALL tile) and no
        two name one tile; an invalid variant is planned with no edit at all (plan_masked's variant);
    level [N, M] bool -- the variant's grid still joins the start tile to the vault over non-wall
        tiles (heist_bfs_valid's answer; set_layout would reject the level where it is False);
    ticks [N, M] int16 -- the fewest ticks to a clean vault arrival from the Solver's cell (-1: none);
    value [N, M] float64, action [N, M] int8 -- the largest discounted return from there and the
        lowest action that starts it (PlanValue's at that cell);
    vis [H, N, M, W] int32 -- row k - 1: the variant's visibility plane of the k-th tick from now,
        4 H N M W bytes;
    togo [N, M, R, C] int16, value_cells [N, M, R, C] float64 or None -- the whole tables
        (PlanField.togo / PlanValue.value of the variant; an added wall cell holds -1 / 0.0); with
        cells=True only;
    edits [N, M, E, 3] int32 -- the edits as given: (row, col, op), op 0 none, 1 add, 2 remove;
    masks [N, M] int64 or None -- the emitter masks as given (None: every slot live);
    tick [N] int32 -- each env's tick at the call, -1 where it was done (PlanValue.tick)."""
    valid: torch.Tensor
    level: torch.Tensor
    ticks: torch.Tensor
    value: torch.Tensor
    action: torch.Tensor
    vis: torch.Tensor
    togo: Optional[torch.Tensor]
    value_cells: Optional[torch.Tensor]
    edits: torch.Tensor
    masks: Optional[torch.Tensor]
    tick: torch.Tensor
    rows: int
    cols: int
    gamma: float = 1.0

    vis_mask = PlanMasked.vis_mask


@dataclass
class PlanQ:
    """HeistEnv.plan_q's output (heist_plan_q, include/heist.h; heist_amd.search.q_values gives the
    same on any device): the exact action values of visited states, [K, N] time-major, state
    (k, e) being the cell env e's Solver stands on k ticks after the tables were made.
    q [K, N, 5] float64 -- the optimal discounted return after taking action a there;
    value [K, N] float64, best [K, N] int8 -- their maximum and its first action (the tables' own
        value and action at that state);
    optimal [K, N] uint8 -- bit a is set iff q[a] equals value exactly: the set of optimal actions;
    gap [K, N] float64 or None -- value - q[taken], exactly 0.0 iff the taken action is optimal.
    A state that is not live (past the env's steps, off the grid, a wall cell) holds 0.0, best -1
    and an empty set.  An output that was not asked for is None."""
    q: Optional[torch.Tensor]
    value: Optional[torch.Tensor]
    best: Optional[torch.Tensor]
    optimal: Optional[torch.Tensor]
    gap: Optional[torch.Tensor]


@dataclass
class PlanPlay:
    """HeistEnv.plan_play's output (heist_plan_play, include/heist.h; heist_amd.search.play_table
    gives the same on CPU tensors): one episode per env played from a planner's per-tick tables.
    actions [H, N] int64 -- the actions taken, heist_step_multi's `actions` as it stands;
    expert [H, N] int8 -- the table's action in the state the step was taken from, -1 where the
        table has none (played as WAIT);
    value [H, N] float64 or None -- the value table's entry in that state;
    records [H, N, W] int32 or None -- the compact record of the observation after the step;
    reward64 [H, N] float64 or None -- the step's reward, the env's own reward64 bit for bit;
    done [H, N] bool, status [H, N] int8 -- the env's own (STATUS_NAMES);
    length [N] int32 -- the steps played, -1 for a start cell outside the grid.
    Rows after a play's end hold action 0, expert -1, value 0.0, a zero record, reward 0.0, done
    True and status already_done."""
    actions: torch.Tensor
    expert: torch.Tensor
    value: Optional[torch.Tensor]
    records: Optional[torch.Tensor]
    reward64: Optional[torch.Tensor]
    done: torch.Tensor
    status: torch.Tensor
    length: torch.Tensor


def noise_q24(noise: float) -> int:
    """A noise probability in [0, 1] as heist_plan_play's 24-bit threshold, round(noise * 2^24)."""
    q = int(round(float(noise) * (1 << 24)))
    if not 0 <= q <= 1 << 24:
        raise ValueError("noise must be in [0, 1], got %r" % (noise,))
    return q


class HeistEnv:
    """Batched HeistEnvironment on one HIP device.

    step(actions) returns (obs, reward, done, status) as device tensors: obs [N,3,R,C]
    float32 (get_state_tensor, environment.py:347-374), reward [N] float32, done [N]
    bool, status [N] int8 (STATUS_NAMES).  With auto_reset=True an env that finishes is
    reset in the same launch (headings carry over, environment.py:204-208) and its obs
    row is the next attempt's first observation.
    """

    def __init__(self, n_envs: int, config=None, max_cams: int = 8, max_guards: int = 4, max_path: int = 16,
                 device=None, auto_reset: bool = True):
        from .environment import EnvironmentConfig
        self.config = config or EnvironmentConfig()
        cfg = self.config
        self.device = nat.require_gpu(device)
        self.n_envs = int(n_envs)
        self.rows, self.cols = cfg.grid_rows, cfg.grid_cols
        self.max_cams, self.max_guards, self.max_path = max_cams, max_guards, max_path
        self.auto_reset = auto_reset
        consts = (ctypes.c_double * 3)(cfg.reward_step, cfg.reward_detection, cfg.reward_vault)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_create(cfg.grid_rows, cfg.grid_cols, cfg.max_steps, cfg.start_pos[0],
                                             cfg.start_pos[1], cfg.vault_pos[0], cfg.vault_pos[1], consts, self.n_envs,
                                             max_cams, max_guards, max_path, ctypes.byref(h)), "heist_create")
        self._h = h
        kw = dict(device=self.device)
        self.obs = torch.zeros((self.n_envs, 3, self.rows, self.cols), dtype=torch.float32, **kw)
        self.reward = torch.zeros(self.n_envs, dtype=torch.float32, **kw)
        self.reward64 = torch.zeros(self.n_envs, dtype=torch.float64, **kw)
        self.done = torch.zeros(self.n_envs, dtype=torch.uint8, **kw)
        self.status = torch.zeros(self.n_envs, dtype=torch.int8, **kw)
        self._done_bool = self.done.view(torch.bool)
        self._bufs = tuple(t.data_ptr() for t in (self.obs, self.reward, self.reward64, self.done, self.status))
        self.valid = torch.zeros(self.n_envs, dtype=torch.uint8, **kw)

    # -- lifecycle ---------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            with torch.cuda.device(self.device):
                torch.cuda.synchronize(self.device)
                nat.lib().heist_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return nat.stream(self.device)

    # -- layout ------------------------------------------------------------------
    def set_layout_batch(self, lb: LayoutBatch, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """heist_set_layout on pre-packed device arrays (only envs in mask if given);
        returns valid [N] bool."""
        n, mc, mg, mp = self.n_envs, max(1, self.max_cams), max(1, self.max_guards), self.max_path
        want = {"wall_rc": (n, lb.max_walls, 2), "n_walls": (n,), "cam_params": (n, mc, 6), "n_cams": (n,),
                "guard_paths": (n, mg, mp, 2), "guard_meta": (n, mg, 3), "guard_fov": (n, mg), "n_guards": (n,),
                "budget": (n,)}
        dtypes = {"cam_params": torch.float64, "guard_fov": torch.float64}
        for k, shp in want.items():  # the kernel indexes with this handle's capacities
            t = getattr(lb, k)
            if tuple(t.shape) != shp or t.dtype != dtypes.get(k, torch.int32) or t.device != self.device \
                    or not t.is_contiguous():
                raise ValueError("LayoutBatch.%s: expected contiguous %s %s on %s, got %s %s on %s"
                                 % (k, dtypes.get(k, torch.int32), shp, self.device, t.dtype, tuple(t.shape), t.device))
        m = None if mask is None else mask.to(device=self.device, dtype=torch.uint8).contiguous()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_set_layout(
                self._h, lb.max_walls, nat.ptr(lb.wall_rc), nat.ptr(lb.n_walls), nat.ptr(lb.cam_params),
                nat.ptr(lb.n_cams), nat.ptr(lb.guard_paths), nat.ptr(lb.guard_meta), nat.ptr(lb.guard_fov),
                nat.ptr(lb.n_guards), nat.ptr(lb.budget), nat.ptr(m), nat.ptr(self.valid), self._stream()),
                "heist_set_layout")
        return self.valid.view(torch.bool)

    def set_layouts(self, layouts: Sequence[Layout], budget: Union[int, Sequence[int]] = None,
                    env_ids: Optional[Sequence[int]] = None) -> torch.Tensor:
        """HeistEnvironment.set_layout (environment.py:102-152) for every env, or only for
        env_ids (then layouts[i] goes to env env_ids[i])."""
        if budget is None:
            budget = self.config.architect_budget
        mask = None
        if env_ids is not None:
            if len(layouts) != len(env_ids):
                raise ValueError("expected one layout per env id")
            full = [([], [], [])] * self.n_envs
            b = np.broadcast_to(np.asarray(budget, np.int32), (len(env_ids),))
            bud = np.zeros(self.n_envs, np.int32)
            for i, e in enumerate(env_ids):
                full[int(e)] = layouts[i]
                bud[int(e)] = b[i]
            m = np.zeros(self.n_envs, np.uint8)
            m[np.asarray(env_ids, np.int64)] = 1
            mask = torch.from_numpy(m).to(self.device)
            layouts, budget = full, bud
        elif len(layouts) != self.n_envs:
            raise ValueError("expected %d layouts, got %d" % (self.n_envs, len(layouts)))
        lb = LayoutBatch.from_lists(layouts, budget, self.max_cams, self.max_guards, self.max_path, self.device,
                                    self.rows, self.cols)
        return self.set_layout_batch(lb, mask)

    # -- episode -----------------------------------------------------------------
    def reset(self, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """HeistEnvironment.reset + get_state_tensor for envs with mask (None: all)."""
        m = None if mask is None else mask.to(device=self.device, dtype=torch.uint8).contiguous()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_reset(self._h, nat.ptr(m), nat.ptr(self.obs), self._stream()), "heist_reset")
        return self.obs

    def step(self, actions: torch.Tensor, auto_reset: Optional[bool] = None, obs_out: torch.Tensor = None):
        """HeistEnvironment.step + get_state_tensor for all envs (environment.py:216-299).

        The per-call host path is kept short (cached buffer addresses, no device switch
        when the handle's device is current) so that back-to-back steps stay GPU-bound."""
        a = actions
        if a.device != self.device or a.dtype != torch.int64 or not a.is_contiguous():
            a = a.to(device=self.device, dtype=torch.int64).contiguous()
        if a.numel() != self.n_envs:
            raise ValueError("step: %d actions for %d envs" % (a.numel(), self.n_envs))
        ar = self.auto_reset if auto_reset is None else auto_reset
        if obs_out is None:
            obs, optr = self.obs, self._bufs[0]
        else:
            if (obs_out.shape != self.obs.shape or obs_out.dtype != torch.float32 or obs_out.device != self.device
                    or not obs_out.is_contiguous()):
                raise ValueError("step: obs_out must be a contiguous float32 %s tensor on %s"
                                 % (tuple(self.obs.shape), self.device))
            obs, optr = obs_out, obs_out.data_ptr()
        L = nat.lib()
        if torch.cuda.current_device() == self.device.index:
            rc = L.heist_step(self._h, a.data_ptr(), optr, *self._bufs[1:], 1 if ar else 0,
                              torch.cuda.current_stream(self.device).cuda_stream)
        else:
            with torch.cuda.device(self.device):
                rc = L.heist_step(self._h, a.data_ptr(), optr, *self._bufs[1:], 1 if ar else 0,
                                  torch.cuda.current_stream(self.device).cuda_stream)
        nat.check(rc, "heist_step")
        return obs, self.reward, self._done_bool, self.status

    def step_multi(self, actions: torch.Tensor, obs_out: Optional[torch.Tensor] = None,
                   auto_reset: Optional[bool] = None, reward64: bool = False):
        """K steps in one launch (heist_step_multi) for actions [K, N] known in advance:
        tick k's observation, reward, done and status land in obs[k], reward[k], ... exactly
        as K step() calls would produce them.  Returns (obs [K,N,3,R,C], reward [K,N] f32,
        done [K,N] bool, status [K,N] int8, reward64 [K,N] f64 or None).  The per-env state
        is on chip between the ticks; env.obs is not updated (obs[K-1] is the latest)."""
        a = actions
        if a.device != self.device or a.dtype != torch.int64 or not a.is_contiguous():
            a = a.to(device=self.device, dtype=torch.int64).contiguous()
        if a.dim() != 2 or a.shape[1] != self.n_envs:
            raise ValueError("step_multi: actions must be [K, %d]" % self.n_envs)
        K = int(a.shape[0])
        kw = dict(device=self.device)
        shape = (K, self.n_envs, 3, self.rows, self.cols)
        if obs_out is None:
            obs_out = torch.empty(shape, dtype=torch.float32, **kw)
        elif (tuple(obs_out.shape) != shape or obs_out.dtype != torch.float32 or obs_out.device != self.device
              or not obs_out.is_contiguous()):
            raise ValueError("step_multi: obs_out must be a contiguous float32 %s tensor on %s" % (shape, self.device))
        rew = torch.empty((K, self.n_envs), dtype=torch.float32, **kw)
        r64 = torch.empty((K, self.n_envs), dtype=torch.float64, **kw) if reward64 else None
        done = torch.empty((K, self.n_envs), dtype=torch.uint8, **kw)
        status = torch.empty((K, self.n_envs), dtype=torch.int8, **kw)
        ar = self.auto_reset if auto_reset is None else auto_reset
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_step_multi(self._h, K, nat.ptr(a), nat.ptr(obs_out), nat.ptr(rew), nat.ptr(r64),
                                                 nat.ptr(done), nat.ptr(status), 1 if ar else 0, self._stream()),
                      "heist_step_multi")
        return obs_out, rew, done.view(torch.bool), status, r64

    @property
    def records_direct(self) -> int:
        """heist_step_records_direct: 1 when step_multi_records' launch writes the records from
        the K-tick kernel itself (no observation row is written), 0 when it steps tick by tick
        into a scratch row and packs it (no K-tick kernel for the grid, or counters, stamps or a
        probe mode armed)."""
        with torch.cuda.device(self.device):
            d = int(nat.lib().heist_step_records_direct(self._h))
        nat.check(0 if d >= 0 else d, "heist_step_records_direct")
        return d

    def step_multi_records(self, actions: torch.Tensor, records_out: Optional[torch.Tensor] = None,
                           auto_reset: Optional[bool] = None, reward64: bool = False):
        """step_multi with every tick's observation as its compact record (heist_step_multi_records):
        records[k] equals pack_obs of step_multi's obs[k], and reward, done, status, reward64 and
        the envs' state afterwards are step_multi's.  Returns (records [K,N,W] int32, reward [K,N]
        f32, done [K,N] bool, status [K,N] int8, reward64 [K,N] f64 or None); the records feed
        CompactObs.of_env(env, records).  env.obs is not updated."""
        from .obs_compact import record_words
        a = actions
        if a.device != self.device or a.dtype != torch.int64 or not a.is_contiguous():
            a = a.to(device=self.device, dtype=torch.int64).contiguous()
        if a.dim() != 2 or a.shape[1] != self.n_envs:
            raise ValueError("step_multi_records: actions must be [K, %d]" % self.n_envs)
        K = int(a.shape[0])
        kw = dict(device=self.device)
        shape = (K, self.n_envs, record_words(self.rows, self.cols))
        if records_out is None:
            records_out = torch.empty(shape, dtype=torch.int32, **kw)
        elif (tuple(records_out.shape) != shape or records_out.dtype != torch.int32 or records_out.device != self.device
              or not records_out.is_contiguous() or records_out.data_ptr() % 16):
            raise ValueError("step_multi_records: records_out must be a contiguous, 16-byte aligned int32 %s tensor on %s"
                             % (shape, self.device))
        rew = torch.empty((K, self.n_envs), dtype=torch.float32, **kw)
        r64 = torch.empty((K, self.n_envs), dtype=torch.float64, **kw) if reward64 else None
        done = torch.empty((K, self.n_envs), dtype=torch.uint8, **kw)
        status = torch.empty((K, self.n_envs), dtype=torch.int8, **kw)
        ar = self.auto_reset if auto_reset is None else auto_reset
        # the fallback's one scratch row (stream-ordered: the allocator keeps it until the work is done)
        scratch = None if self.records_direct else torch.empty_like(self.obs)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_step_multi_records(self._h, K, nat.ptr(a), nat.ptr(records_out), nat.ptr(rew),
                                                         nat.ptr(r64), nat.ptr(done), nat.ptr(status), 1 if ar else 0,
                                                         nat.ptr(scratch), self._stream()),
                      "heist_step_multi_records")
        return records_out, rew, done.view(torch.bool), status, r64

    # -- exact planner (heist_plan) ---------------------------------------------------------
    @property
    def plan_supported(self) -> int:
        """heist_plan_supported: 1 when plan() has a kernel for this handle."""
        with torch.cuda.device(self.device):
            d = int(nat.lib().heist_plan_supported(self._h))
        nat.check(0 if d >= 0 else d, "heist_plan_supported")
        return d

    def plan(self, horizon: Optional[int] = None) -> "PlanResult":
        """heist_plan: for every env as it stands, the fewest ticks in which the Solver can reach
        the vault undetected, the canonical action sequence that does it (rows of a step_multi
        `actions` tensor) and the set of cells it can occupy, live and unseen, after every tick.
        horizon: ticks to look ahead (default config.max_steps, at most 1024); an env plans
        min(horizon, max_steps - tick).  Reads the envs only."""
        from .obs_compact import record_words
        H = min(int(self.config.max_steps), 1024) if horizon is None else int(horizon)
        kw = dict(device=self.device)
        ticks = torch.empty(self.n_envs, dtype=torch.int32, **kw)
        actions = torch.empty((max(H, 0), self.n_envs), dtype=torch.int64, **kw)
        reach = torch.empty((max(H, 0), self.n_envs, record_words(self.rows, self.cols)), dtype=torch.int32, **kw)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_plan(self._h, H, nat.ptr(ticks), nat.ptr(actions), nat.ptr(reach), self._stream()),
                      "heist_plan")
        return PlanResult(ticks, actions, reach, self.rows, self.cols)

    # -- planner field (heist_plan_field) ----------------------------------------------------
    @property
    def plan_field_supported(self) -> int:
        """heist_plan_field_supported: 1 when plan_field() has a kernel for this handle."""
        with torch.cuda.device(self.device):
            d = int(nat.lib().heist_plan_field_supported(self._h))
        nat.check(0 if d >= 0 else d, "heist_plan_field_supported")
        return d

    def plan_field(self, horizon: Optional[int] = None, all_ticks: bool = False) -> "PlanField":
        """heist_plan_field: for every env as it stands and every cell, the fewest ticks in which a
        Solver on that cell can reach the vault undetected and the lowest action that starts such
        a path, plus the visibility plane of every coming tick; with all_ticks the same field for
        every later tick of the horizon (heist_amd.search.follow_field / expert_labels read it).
        horizon: ticks to look ahead (default config.max_steps, at most 1024); an env runs
        min(horizon, max_steps - tick).  Reads the envs only."""
        from .obs_compact import record_words
        H = min(int(self.config.max_steps), 1024) if horizon is None else int(horizon)
        kw = dict(device=self.device)
        n, R, C, h = self.n_envs, self.rows, self.cols, max(H, 0)
        togo = torch.empty((n, R, C), dtype=torch.int16, **kw)
        action = torch.empty((n, R, C), dtype=torch.int8, **kw)
        vis = torch.empty((h, n, record_words(R, C)), dtype=torch.int32, **kw)
        ticks = torch.empty((h, n, R, C), dtype=torch.int16, **kw) if all_ticks else None
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_plan_field(self._h, H, nat.ptr(togo), nat.ptr(action), nat.ptr(vis), nat.ptr(ticks),
                                                 self._stream()), "heist_plan_field")
        return PlanField(togo, action, vis, ticks, R, C, tuple(int(v) for v in self.config.vault_pos))

    # -- planner value (heist_plan_value) ----------------------------------------------------
    @property
    def plan_value_supported(self) -> int:
        """heist_plan_value_supported: 1 when plan_value() has a kernel for this handle (every
        grid up to 32 x 32; 0 at 64 x 64, whose value arrays do not fit a workgroup's LDS)."""
        with torch.cuda.device(self.device):
            d = int(nat.lib().heist_plan_value_supported(self._h))
        nat.check(0 if d >= 0 else d, "heist_plan_value_supported")
        return d

    def plan_value(self, horizon: Optional[int] = None, gamma: float = 1.0, all_ticks: bool = False) -> "PlanValue":
        """heist_plan_value: for every env as it stands and every cell, the largest discounted
        return (the env's own reward64) a Solver on that cell can still collect and the lowest
        action that starts such a play, plus the visibility plane of every coming tick; with
        all_ticks the same for every later tick of the horizon (heist_amd.search.follow_value /
        value_targets read them; value_ticks takes 8 H N R C bytes).  horizon: ticks to look
        ahead (default config.max_steps, at most 1024); an env runs min(horizon, max_steps - tick),
        and with fewer than max_steps - tick the return is cut at the horizon.  gamma in [0, 1].
        Reads the envs only."""
        from .obs_compact import record_words
        H = min(int(self.config.max_steps), 1024) if horizon is None else int(horizon)
        kw = dict(device=self.device)
        n, R, C, h = self.n_envs, self.rows, self.cols, max(H, 0)
        value = torch.empty((n, R, C), dtype=torch.float64, **kw)
        action = torch.empty((n, R, C), dtype=torch.int8, **kw)
        vis = torch.empty((h, n, record_words(R, C)), dtype=torch.int32, **kw)
        vticks = torch.empty((h, n, R, C), dtype=torch.float64, **kw) if all_ticks else None
        aticks = torch.empty((h, n, R, C), dtype=torch.int8, **kw) if all_ticks else None
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_plan_value(self._h, H, float(gamma), nat.ptr(value), nat.ptr(action), nat.ptr(vis),
                                                 nat.ptr(vticks), nat.ptr(aticks), self._stream()), "heist_plan_value")
        ex = self.export(grid=True)
        tick = torch.where(ex["done"] != 0, torch.full_like(ex["tick"], -1), ex["tick"])
        return PlanValue(value, action, vis, vticks, aticks, R, C, tuple(int(v) for v in self.config.vault_pos),
                         float(gamma), ex["grid"], tick)

    # -- planner what-if (heist_plan_masked) --------------------------------------------------
    @property
    def plan_masked_supported(self) -> int:
        """heist_plan_masked_supported: 1 when plan_masked() has a kernel for this handle (where
        plan_value() has one: every grid up to 32 x 32; 0 at 64 x 64)."""
        with torch.cuda.device(self.device):
            d = int(nat.lib().heist_plan_masked_supported(self._h))
        nat.check(0 if d >= 0 else d, "heist_plan_masked_supported")
        return d

    def plan_masked(self, masks, horizon: Optional[int] = None, gamma: float = 1.0, cells: bool = False) -> "PlanMasked":
        """heist_plan_masked: every env as it stands planned under M sets of its emitters in one
        launch -- the fewest ticks to the vault and the largest discounted return from the Solver's
        cell with the emitter slots of masks[e, m] alone (bit j: slot j is live; cameras are slots
        0 .. max_cams - 1, guard g is slot max_cams + g; bits of unfilled slots are ignored), plus
        every variant's visibility planes and, with cells, the whole tables.  masks: int64 [N, M],
        or [M] for the same masks on every env.  horizon and gamma as in plan_value.  vis takes
        4 H N M W bytes.  Reads the envs only."""
        from .obs_compact import record_words
        H = min(int(self.config.max_steps), 1024) if horizon is None else int(horizon)
        n, R, C, h = self.n_envs, self.rows, self.cols, max(H, 0)
        mk = torch.as_tensor(masks)
        if mk.dtype != torch.int64 or mk.dim() not in (1, 2) or (mk.dim() == 2 and mk.shape[0] != n):
            raise ValueError("plan_masked: masks must be an int64 [%d, M] or [M] tensor" % n)
        if mk.dim() == 1:
            mk = mk.reshape(1, -1).expand(n, -1)
        mk = mk.to(self.device).contiguous()
        M = int(mk.shape[1])
        kw = dict(device=self.device)
        ticks = torch.empty((n, M), dtype=torch.int16, **kw)
        value = torch.empty((n, M), dtype=torch.float64, **kw)
        action = torch.empty((n, M), dtype=torch.int8, **kw)
        vis = torch.empty((h, n, M, record_words(R, C)), dtype=torch.int32, **kw)
        tcells = torch.empty((n, M, R, C), dtype=torch.int16, **kw) if cells else None
        vcells = torch.empty((n, M, R, C), dtype=torch.float64, **kw) if cells else None
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_plan_masked(self._h, H, float(gamma), M, nat.ptr(mk) if M else None, nat.ptr(ticks),
                                                  nat.ptr(value), nat.ptr(action), nat.ptr(vis), nat.ptr(tcells),
                                                  nat.ptr(vcells), self._stream()), "heist_plan_masked")
        ex = self.export()
        tick = torch.where(ex["done"] != 0, torch.full_like(ex["tick"], -1), ex["tick"])
        return PlanMasked(ticks, value, action, vis, tcells, vcells, mk, tick, R, C, float(gamma))

    def plan_ablate(self, horizon: Optional[int] = None, gamma: float = 1.0):
        """Every env's emitters switched off one at a time: plan_masked with
        heist_amd.search.ablation_masks of the envs' own emitter counts, as a
        heist_amd.search.PlanAblation -- ticks and value of the layout as built (column 0) and
        without slot j (column 1 + j), the ticks each emitter costs, its credit in return, and
        which emitters are critical or redundant.  One launch; reads the envs only."""
        from .search import PlanAblation, ablation_masks
        ex = self.export()
        mc, mg = self.max_cams, self.max_guards
        pm = self.plan_masked(ablation_masks(ex["n_cams"], ex["n_guards"], mc, mg), horizon=horizon, gamma=gamma)
        j = torch.arange(mc + mg, device=self.device).reshape(1, -1)
        filled = torch.where(j < mc, j < ex["n_cams"].reshape(-1, 1), j - mc < ex["n_guards"].reshape(-1, 1))
        return PlanAblation.from_tables(pm.ticks, pm.value, filled)

    # -- planner walls (heist_plan_walls) ------------------------------------------------------
    @property
    def plan_walls_supported(self) -> int:
        """heist_plan_walls_supported: 1 when plan_walls() has a kernel for this handle (where
        plan_masked() has one: every grid up to 32 x 32; 0 at 64 x 64)."""
        with torch.cuda.device(self.device):
            d = int(nat.lib().heist_plan_walls_supported(self._h))
        nat.check(0 if d >= 0 else d, "heist_plan_walls_supported")
        return d

    def plan_walls(self, edits, masks=None, horizon: Optional[int] = None, gamma: float = 1.0,
                   cells: bool = False) -> "PlanWalls":
        """heist_plan_walls: every env as it stands planned with walls added or removed, M variants
        per env in one launch that casts every live emitter against the variant's own walls -- the
        fewest ticks to the vault and the largest discounted return from the Solver's cell on the
        edited grid, whether the edits hold, whether the level is still valid, plus every variant's
        visibility planes and, with cells, the whole tables.  edits: int32 [N, M, E, 3] with
        1 <= E <= 8, or [N, M, 3] for E = 1, each edit (row, col, op): op 0 none, 1 add a wall,
        2 remove one.  masks: plan_masked's int64 [N, M] or [M], or None for every slot live.
        horizon and gamma as in plan_value.  vis takes 4 H N M W bytes.  Reads the envs only."""
        from .obs_compact import record_words
        H = min(int(self.config.max_steps), 1024) if horizon is None else int(horizon)
        n, R, C, h = self.n_envs, self.rows, self.cols, max(H, 0)
        ed = torch.as_tensor(edits)
        if ed.dtype != torch.int32 or ed.dim() not in (3, 4) or ed.shape[0] != n or ed.shape[-1] != 3:
            raise ValueError("plan_walls: edits must be an int32 [%d, M, E, 3] or [%d, M, 3] tensor" % (n, n))
        if ed.dim() == 3:
            ed = ed.unsqueeze(2)
        ed = ed.to(self.device).contiguous()
        M, E = int(ed.shape[1]), int(ed.shape[2])
        mk = None
        if masks is not None:
            mk = torch.as_tensor(masks)
            if mk.dtype != torch.int64 or mk.dim() not in (1, 2) or (mk.dim() == 2 and mk.shape[0] != n):
                raise ValueError("plan_walls: masks must be an int64 [%d, M] or [M] tensor" % n)
            if mk.dim() == 1:
                mk = mk.reshape(1, -1).expand(n, -1)
            if int(mk.shape[1]) != M:
                raise ValueError("plan_walls: masks must hold one mask per variant (M = %d)" % M)
            mk = mk.to(self.device).contiguous()
        kw = dict(device=self.device)
        valid = torch.empty((n, M), dtype=torch.uint8, **kw)
        level = torch.empty((n, M), dtype=torch.uint8, **kw)
        ticks = torch.empty((n, M), dtype=torch.int16, **kw)
        value = torch.empty((n, M), dtype=torch.float64, **kw)
        action = torch.empty((n, M), dtype=torch.int8, **kw)
        vis = torch.empty((h, n, M, record_words(R, C)), dtype=torch.int32, **kw)
        tcells = torch.empty((n, M, R, C), dtype=torch.int16, **kw) if cells else None
        vcells = torch.empty((n, M, R, C), dtype=torch.float64, **kw) if cells else None
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_plan_walls(self._h, H, float(gamma), M, E, nat.ptr(ed) if M and E else None,
                                                 nat.ptr(mk), nat.ptr(valid), nat.ptr(level), nat.ptr(ticks),
                                                 nat.ptr(value), nat.ptr(action), nat.ptr(vis), nat.ptr(tcells),
                                                 nat.ptr(vcells), self._stream()), "heist_plan_walls")
        ex = self.export()
        tick = torch.where(ex["done"] != 0, torch.full_like(ex["tick"], -1), ex["tick"])
        return PlanWalls(valid.view(torch.bool), level.view(torch.bool), ticks, value, action, vis, tcells, vcells, ed,
                         mk, tick, R, C, float(gamma))

    def plan_wall_ablate(self, max_walls: Optional[int] = None, horizon: Optional[int] = None, gamma: float = 1.0):
        """Every env's interior walls removed one at a time: plan_walls with
        heist_amd.search.wall_ablation_edits of the envs' own grids, as a
        heist_amd.search.WallAblation -- ticks and value of the layout as built (column 0) and
        without wall j in row-major order (column 1 + j), each wall's signed credit, and which walls
        are critical, redundant or shielding.  max_walls: the columns (None: the largest count of
        the batch).  One launch; reads the envs only."""
        from .search import WallAblation, wall_ablation_edits
        grid = self.grid_snapshot()
        if max_walls is None:
            g = grid[:, 1:-1, 1:-1]
            max_walls = int((g == 1).reshape(g.shape[0], -1).sum(1).max().item()) if g.numel() else 0
        ed, filled = wall_ablation_edits(grid, int(max_walls))
        pw = self.plan_walls(ed, horizon=horizon, gamma=gamma)
        return WallAblation.from_tables(pw.ticks, pw.value, filled.to(self.device))

    # -- planner placement (heist_plan_place) --------------------------------------------------
    @property
    def plan_place_supported(self) -> int:
        """heist_plan_place_supported: 1 when plan_place() has a kernel for this handle (where
        plan_masked() has one: every grid up to 32 x 32; 0 at 64 x 64)."""
        with torch.cuda.device(self.device):
            d = int(nat.lib().heist_plan_place_supported(self._h))
        nat.check(0 if d >= 0 else d, "heist_plan_place_supported")
        return d

    def plan_place(self, cands, horizon: Optional[int] = None, gamma: float = 1.0, base: Optional[torch.Tensor] = None,
                   cells: bool = False) -> "PlanPlace":
        """heist_plan_place: every env as it stands planned with one more camera, M candidates per
        env in one launch that casts the candidate alone -- the fewest ticks to the vault and the
        largest discounted return from the Solver's cell over the rows of `base` ORed with the
        candidate's cone, plus every variant's visibility planes and, with cells, the whole tables.
        cands: float64 [N, M, 6], or [M, 6] for the same candidates on every env, each row a
        set_layout camera (row, col, fov_angle, heading, rotation_speed, vision_range) with the
        heading it has now.  base: the visibility rows the candidates are added to, int32
        [H, N, W] -- PlanField.vis, PlanValue.vis or PlanMasked.vis[:, :, m] of this handle as it
        stands -- or None, and then plan_field(horizon) supplies them.  horizon and gamma as in
        plan_value.  vis takes 4 H N M W bytes.  Reads the envs only."""
        from .obs_compact import record_words
        H = min(int(self.config.max_steps), 1024) if horizon is None else int(horizon)
        n, R, C, h = self.n_envs, self.rows, self.cols, max(H, 0)
        W = record_words(R, C)
        cd = torch.as_tensor(cands)
        if cd.dtype != torch.float64 or cd.dim() not in (2, 3) or cd.shape[-1] != 6 or (cd.dim() == 3 and cd.shape[0] != n):
            raise ValueError("plan_place: cands must be a float64 [%d, M, 6] or [M, 6] tensor" % n)
        if cd.dim() == 2:
            cd = cd.unsqueeze(0).expand(n, -1, -1)
        cd = cd.to(self.device).contiguous()
        M = int(cd.shape[1])
        if base is None:
            base = self.plan_field(horizon=H).vis if 1 <= H <= 1024 else None
        elif (not isinstance(base, torch.Tensor) or base.dtype != torch.int32 or tuple(base.shape) != (h, n, W)
              or base.device != self.device):
            raise ValueError("plan_place: base must be an int32 [%d, %d, %d] tensor on %s" % (h, n, W, self.device))
        else:
            base = base.contiguous()
            if base.data_ptr() % 16:  # a slice that starts off a 16-byte boundary
                base = base.clone()
        kw = dict(device=self.device)
        valid = torch.empty((n, M), dtype=torch.uint8, **kw)
        ticks = torch.empty((n, M), dtype=torch.int16, **kw)
        value = torch.empty((n, M), dtype=torch.float64, **kw)
        action = torch.empty((n, M), dtype=torch.int8, **kw)
        vis = torch.empty((h, n, M, W), dtype=torch.int32, **kw)
        tcells = torch.empty((n, M, R, C), dtype=torch.int16, **kw) if cells else None
        vcells = torch.empty((n, M, R, C), dtype=torch.float64, **kw) if cells else None
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_plan_place(self._h, H, float(gamma), M, nat.ptr(cd) if M else None, nat.ptr(base),
                                                 nat.ptr(valid), nat.ptr(ticks), nat.ptr(value), nat.ptr(action),
                                                 nat.ptr(vis), nat.ptr(tcells), nat.ptr(vcells), self._stream()),
                      "heist_plan_place")
        ex = self.export()
        tick = torch.where(ex["done"] != 0, torch.full_like(ex["tick"], -1), ex["tick"])
        return PlanPlace(valid.view(torch.bool), ticks, value, action, vis, tcells, vcells, cd, tick, R, C, float(gamma))

    # -- planner placement for guards (heist_plan_place_guard) ---------------------------------
    @property
    def plan_place_guard_supported(self) -> int:
        """heist_plan_place_guard_supported: 1 when plan_place_guard() has a kernel for this handle
        (where plan_place() has one)."""
        with torch.cuda.device(self.device):
            d = int(nat.lib().heist_plan_place_guard_supported(self._h))
        nat.check(0 if d >= 0 else d, "heist_plan_place_guard_supported")
        return d

    def _guard_candidates_arg(self, paths, meta, fov):
        """plan_place_guard's three candidate arrays, checked and broadcast to [N, M, ...] (host or
        device tensors as given; no device is touched)."""
        n = self.n_envs
        pa, me, fv = torch.as_tensor(paths), torch.as_tensor(meta), torch.as_tensor(fov)
        lead = pa.dim() - 2  # 1: [M, ...] for every env, 2: [N, M, ...]
        if (pa.dtype != torch.int32 or lead not in (1, 2) or pa.shape[-1] != 2 or not 1 <= pa.shape[-2] <= 64
                or (lead == 2 and pa.shape[0] != n)):
            raise ValueError("plan_place_guard: paths must be an int32 [%d, M, P, 2] or [M, P, 2] tensor, 1 <= P <= 64" % n)
        shape = tuple(pa.shape[:lead])
        if me.dtype != torch.int32 or tuple(me.shape) != shape + (4,):
            raise ValueError("plan_place_guard: meta must be an int32 %r tensor (len, speed, vision_range, idx)"
                             % (list(shape) + [4],))
        if fv.dtype != torch.float64 or tuple(fv.shape) != shape + (2,):
            raise ValueError("plan_place_guard: fov must be a float64 %r tensor (fov_angle, heading)"
                             % (list(shape) + [2],))
        if lead == 1:
            pa, me, fv = (x.unsqueeze(0).expand(n, *x.shape) for x in (pa, me, fv))
        return pa, me, fv

    def plan_place_guard(self, paths, meta, fov, horizon: Optional[int] = None, gamma: float = 1.0,
                         base: Optional[torch.Tensor] = None, cells: bool = False) -> "PlanPlace":
        """heist_plan_place_guard: every env as it stands planned with one more guard, M candidates
        per env in one launch that casts the candidate alone -- plan_place's answers over the rows
        of `base` ORed with the candidate's cone and its own cell.
        paths: int32 [N, M, P, 2] patrol points (row, col), 1 <= P <= 64; meta: int32 [N, M, 4] =
        (len, speed, vision_range, idx), idx the patrol index the guard stands on now; fov: float64
        [N, M, 2] = (fov_angle, heading), the heading it has now -- or [M, ...] each, the same
        candidates on every env.  base, horizon, gamma, cells as in plan_place.  Returns a PlanPlace
        whose cands is the tuple (paths, meta, fov) as launched.  Reads the envs only."""
        from .obs_compact import record_words
        H = min(int(self.config.max_steps), 1024) if horizon is None else int(horizon)
        n, R, C, h = self.n_envs, self.rows, self.cols, max(H, 0)
        W = record_words(R, C)
        pa, me, fv = (x.to(self.device).contiguous() for x in self._guard_candidates_arg(paths, meta, fov))
        M, P = int(pa.shape[1]), int(pa.shape[2])
        if base is None:
            base = self.plan_field(horizon=H).vis if 1 <= H <= 1024 else None
        elif (not isinstance(base, torch.Tensor) or base.dtype != torch.int32 or tuple(base.shape) != (h, n, W)
              or base.device != self.device):
            raise ValueError("plan_place_guard: base must be an int32 [%d, %d, %d] tensor on %s" % (h, n, W, self.device))
        else:
            base = base.contiguous()
            if base.data_ptr() % 16:  # a slice that starts off a 16-byte boundary
                base = base.clone()
        kw = dict(device=self.device)
        valid = torch.empty((n, M), dtype=torch.uint8, **kw)
        ticks = torch.empty((n, M), dtype=torch.int16, **kw)
        value = torch.empty((n, M), dtype=torch.float64, **kw)
        action = torch.empty((n, M), dtype=torch.int8, **kw)
        vis = torch.empty((h, n, M, W), dtype=torch.int32, **kw)
        tcells = torch.empty((n, M, R, C), dtype=torch.int16, **kw) if cells else None
        vcells = torch.empty((n, M, R, C), dtype=torch.float64, **kw) if cells else None
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_plan_place_guard(self._h, H, float(gamma), M, P, nat.ptr(pa) if M else None,
                                                       nat.ptr(me) if M else None, nat.ptr(fv) if M else None,
                                                       nat.ptr(base), nat.ptr(valid), nat.ptr(ticks), nat.ptr(value),
                                                       nat.ptr(action), nat.ptr(vis), nat.ptr(tcells), nat.ptr(vcells),
                                                       self._stream()),
                      "heist_plan_place_guard")
        ex = self.export()
        tick = torch.where(ex["done"] != 0, torch.full_like(ex["tick"], -1), ex["tick"])
        return PlanPlace(valid.view(torch.bool), ticks, value, action, vis, tcells, vcells, (pa, me, fv), tick, R, C,
                         float(gamma))

    # -- planner Q (heist_plan_q) --------------------------------------------------------------
    PLAN_Q_OUTPUTS = ("q", "value", "best", "optimal", "gap")

    def plan_q(self, pv, pos: torch.Tensor, taken: Optional[torch.Tensor] = None,
               tick0: Optional[torch.Tensor] = None, gamma: Optional[float] = None,
               outputs: Optional[Sequence[str]] = None) -> "PlanQ":
        """heist_plan_q: the five exact action values of every visited state in one launch that
        casts no ray and touches no env.  pv: a PlanValue made with all_ticks=True, or a
        (values [H, N, R, C] float64, vis [H, N, W] int32) pair of hand-made tables; pos [K, N, 2]
        (row, col) with K <= H, row k the Solver's cell k ticks after the tables were made
        (obs_compact.record_cells gives it from a rollout's decision records); taken [K, N] the
        action taken there, or None (then there is no gap).  tick0 [N]: each env's tick when the
        tables were made, -1 for an env done then; it defaults to pv.tick for a PlanValue, and for
        a pair to None, the handle's tick and done flag as they are now -- right only while the
        handle has not been stepped since.  gamma defaults to pv.gamma (1.0 for a pair).  outputs:
        the PlanQ fields to compute (default all; gap only with taken).  The handle's layout must
        be the one the tables were made for.  Reads the envs only."""
        from .obs_compact import record_words
        n, R, C = self.n_envs, self.rows, self.cols
        W = record_words(R, C)
        dev = self.device
        if isinstance(pv, PlanValue):
            if pv.value_ticks is None:
                raise ValueError("plan_q: the value has no per-tick rows (plan_value(all_ticks=True))")
            values, vis = pv.value_ticks, pv.vis
            gamma = pv.gamma if gamma is None else gamma
            tick0 = pv.tick if tick0 is None else tick0
        else:
            values, vis = pv
            gamma = 1.0 if gamma is None else gamma
        H = int(values.shape[0]) if values.dim() else 0

        def arg(t, dtype, shape, what, align=1):
            if tuple(t.shape) != shape or t.dtype != dtype:
                raise ValueError("plan_q: %s must be a %s %s tensor" % (what, dtype, shape))
            if t.device != dev or not t.is_contiguous() or t.data_ptr() % align:
                t = t.to(dev).contiguous()
                if t.data_ptr() % align:
                    t = t.clone()
            return t
        values = arg(values, torch.float64, (H, n, R, C), "values", 8)
        vis = arg(vis, torch.int32, (H, n, W), "vis", 16)
        pos = torch.as_tensor(pos)
        if pos.dim() != 3 or tuple(pos.shape[1:]) != (n, 2):
            raise ValueError("plan_q: pos must be [K, %d, 2]" % n)
        K = int(pos.shape[0])
        pos = pos.to(device=dev, dtype=torch.int32).contiguous()
        if taken is not None:
            taken = torch.as_tensor(taken).to(device=dev, dtype=torch.int64).reshape(K, n).contiguous()
        if tick0 is not None:
            tick0 = torch.as_tensor(tick0).to(device=dev, dtype=torch.int32).reshape(n).contiguous()
        names = self.PLAN_Q_OUTPUTS if outputs is None else tuple(outputs)
        if any(name not in self.PLAN_Q_OUTPUTS for name in names):
            raise ValueError("plan_q: outputs must be among %s" % (self.PLAN_Q_OUTPUTS,))
        if outputs is None and taken is None:
            names = tuple(name for name in names if name != "gap")
        kw = dict(device=dev)
        shapes = {"q": ((K, n, 5), torch.float64), "value": ((K, n), torch.float64), "best": ((K, n), torch.int8),
                  "optimal": ((K, n), torch.uint8), "gap": ((K, n), torch.float64)}
        out = PlanQ(*(torch.empty(shapes[f][0], dtype=shapes[f][1], **kw) if f in names else None
                      for f in self.PLAN_Q_OUTPUTS))
        P = nat.ptr
        with torch.cuda.device(dev):
            nat.check(nat.lib().heist_plan_q(self._h, H, K, float(gamma), P(values), P(vis), P(tick0), P(pos), P(taken),
                                             P(out.q), P(out.value), P(out.best), P(out.optimal), P(out.gap),
                                             self._stream()), "heist_plan_q")
        return out

    # -- planner playout (heist_plan_play) ---------------------------------------------------
    def plan_play(self, table: torch.Tensor, vis: torch.Tensor, values: Optional[torch.Tensor] = None,
                  pos: Optional[torch.Tensor] = None, noise: float = 0.0, seed: int = 0, records: bool = True,
                  rewards: bool = True) -> "PlanPlay":
        """heist_plan_play: one episode per env played from per-tick tables in one launch that
        casts no ray and touches no env.  table [H, N, R, C] int8 (plan_value(all_ticks=True)'s
        action_ticks, or any table of actions per tick and cell), vis [H, N, W] int32 (the same
        plan's vis), values [H, N, R, C] float64 or None (value_ticks), pos [N, 2] (row, col) start
        cells or None for the envs' own.  With probability noise (rounded to 24 bits) a step
        takes a uniform action instead of the table's, drawn from a hash of (seed, the env's
        tick, the env): the same seed continues the same draws mid-episode.  records / rewards:
        also return every step's compact record / float64 reward.  Reads the envs only."""
        from .obs_compact import record_words
        n, R, C = self.n_envs, self.rows, self.cols
        W = record_words(R, C)
        H = int(table.shape[0]) if table.dim() else 0
        dev = self.device

        def arg(t, dtype, shape, what, align=1):
            if tuple(t.shape) != shape or t.dtype != dtype:
                raise ValueError("plan_play: %s must be a %s %s tensor" % (what, dtype, shape))
            if t.device != dev or not t.is_contiguous() or t.data_ptr() % align:
                t = t.to(dev).contiguous()
                if t.data_ptr() % align:
                    t = t.clone()
            return t
        table = arg(table, torch.int8, (H, n, R, C), "table")
        vis = arg(vis, torch.int32, (H, n, W), "vis", 16)
        if values is not None:
            values = arg(values, torch.float64, (H, n, R, C), "values", 8)
        if pos is not None:
            pos = torch.as_tensor(pos).to(device=dev, dtype=torch.int32).reshape(n, 2).contiguous()
        kw = dict(device=dev)
        out = PlanPlay(torch.empty((H, n), dtype=torch.int64, **kw), torch.empty((H, n), dtype=torch.int8, **kw),
                       None if values is None else torch.empty((H, n), dtype=torch.float64, **kw),
                       torch.empty((H, n, W), dtype=torch.int32, **kw) if records else None,
                       torch.empty((H, n), dtype=torch.float64, **kw) if rewards else None,
                       torch.empty((H, n), dtype=torch.uint8, **kw), torch.empty((H, n), dtype=torch.int8, **kw),
                       torch.empty(n, dtype=torch.int32, **kw))
        P = nat.ptr
        with torch.cuda.device(dev):
            nat.check(nat.lib().heist_plan_play(self._h, H, P(table), P(vis), P(values), P(pos), noise_q24(noise),
                                                int(seed) & (2 ** 64 - 1), P(out.actions), P(out.expert), P(out.value),
                                                P(out.records), P(out.reward64), P(out.done), P(out.status),
                                                P(out.length), self._stream()), "heist_plan_play")
        out.done = out.done.view(torch.bool)
        return out

    def step_multi_raw(self, K: int, actions: torch.Tensor, obs_out: torch.Tensor, reward: torch.Tensor,
                       done: torch.Tensor, status: torch.Tensor, auto_reset: bool = True) -> None:
        """heist_step_multi on caller-owned buffers with no checks or allocation (the
        benchmark's timed loop; shapes as step_multi's)."""
        rc = nat.lib().heist_step_multi(self._h, K, actions.data_ptr(), obs_out.data_ptr(), reward.data_ptr(), None,
                                        done.data_ptr(), status.data_ptr(), 1 if auto_reset else 0,
                                        torch.cuda.current_stream(self.device).cuda_stream)
        nat.check(rc, "heist_step_multi")

    def step_multi_launcher(self, K: int, actions: torch.Tensor, obs_out: torch.Tensor, reward: torch.Tensor,
                            done: torch.Tensor, status: torch.Tensor, auto_reset: bool = True):
        """step_multi_raw with every argument resolved now (device pointers, the stream, the
        bound C function): returns a zero-argument callable that only issues the launch, so
        a timed region around it holds no Python argument handling.  The tensors must stay
        alive while the callable is used."""
        fn = nat.lib().heist_step_multi
        args = (self._h, K, actions.data_ptr(), obs_out.data_ptr(), reward.data_ptr(), None, done.data_ptr(),
                status.data_ptr(), 1 if auto_reset else 0, torch.cuda.current_stream(self.device).cuda_stream)

        def launch():
            rc = fn(*args)
            if rc:
                nat.check(rc, "heist_step_multi")
        return launch

    # -- introspection -------------------------------------------------------------
    def export(self, grid: bool = False) -> dict:
        """Per-env state (get_environment_state source) as device tensors."""
        kw = dict(device=self.device)
        sc = torch.empty((self.n_envs, 12), dtype=torch.int32, **kw)
        ch = torch.empty((self.n_envs, max(1, self.max_cams)), dtype=torch.float64, **kw)
        gi = torch.empty((self.n_envs, max(1, self.max_guards)), dtype=torch.int32, **kw)
        gh = torch.empty((self.n_envs, max(1, self.max_guards)), dtype=torch.float64, **kw)
        gr = torch.empty((self.n_envs, self.rows, self.cols), dtype=torch.int8, **kw) if grid else None
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_export(self._h, nat.ptr(sc), nat.ptr(gr), nat.ptr(ch), nat.ptr(gi), nat.ptr(gh),
                                             self._stream()), "heist_export")
        keys = ("pos_r", "pos_c", "tick", "done", "detected", "vault_reached", "prev_dist", "initial_dist",
                "n_cams", "n_guards", "n_walls", "spent")
        out = {k: sc[:, i] for i, k in enumerate(keys)}
        out.update(cam_heading=ch, guard_idx=gi, guard_heading=gh)
        if grid:
            out["grid"] = gr
        return out

    # -- saved states (env_state.EnvState) ------------------------------------------------
    def state_config(self) -> dict:
        """What a saved state depends on: the heist_create arguments (n_envs apart), the
        guard-cone setting, the blob format version and size."""
        from .env_state import FORMAT_VERSION
        cfg = self.config
        b = int(nat.lib().heist_state_bytes(self._h))
        nat.check(0 if b > 0 else b, "heist_state_bytes")
        return {"rows": self.rows, "cols": self.cols, "max_cams": self.max_cams, "max_guards": self.max_guards,
                "max_path": self.max_path, "guard_cones": self.kernel_config()["guard_cones"],
                "max_steps": cfg.max_steps, "start_r": cfg.start_pos[0], "start_c": cfg.start_pos[1],
                "vault_r": cfg.vault_pos[0], "vault_c": cfg.vault_pos[1], "version": FORMAT_VERSION, "bytes": b}

    def _ids(self, ids, what):
        if ids is None:
            return None
        t = torch.as_tensor(ids).reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
        if t.numel() == 0:
            raise ValueError("%s: empty index list" % what)
        return t

    def save_state(self, env_ids=None):
        """heist_state_save: the envs env_ids (None: all, in order) as an EnvState on this device.
        Reads the envs only.  The observation (env.obs) is an output, not state: keep it yourself
        if the next action is chosen from it."""
        from .env_state import EnvState
        cfg = self.state_config()
        ids = self._ids(env_ids, "save_state")
        m = self.n_envs if ids is None else int(ids.numel())
        blobs = torch.empty((m, cfg["bytes"]), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_state_save(self._h, nat.ptr(ids), m, nat.ptr(blobs), self._stream()),
                      "heist_state_save")
        return EnvState(blobs, cfg)

    def load_state(self, state, env_ids=None, index=None) -> torch.Tensor:
        """heist_state_load: env env_ids[i] (None: i) <- blob index[i] (None: i) of state; a fork
        is index naming one blob many times.  Returns status [m] bool on this device: False where
        the device rejected the item (env id out of range or named twice, blob index out of
        range, a blob whose header or records do not fit) and left the env untouched.  Raises
        HeistError, before any launch, when state was saved under another configuration."""
        state.check(self.state_config())
        ids, idx = self._ids(env_ids, "load_state"), self._ids(index, "load_state")
        if ids is not None and idx is not None and ids.numel() != idx.numel():
            raise ValueError("load_state: %d env ids for %d blob indices" % (ids.numel(), idx.numel()))
        m = int(ids.numel()) if ids is not None else (int(idx.numel()) if idx is not None else len(state))
        blobs = state.blobs
        if blobs.device != self.device:
            blobs = blobs.to(self.device)
        if blobs.data_ptr() % 16:
            blobs = blobs.clone()
        status = torch.zeros(m, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_state_load(self._h, nat.ptr(ids), m, nat.ptr(blobs), len(state), nat.ptr(idx),
                                                 nat.ptr(status), self._stream()), "heist_state_load")
        return status.view(torch.bool)

    def fork_state(self, src_ids, dst_ids) -> torch.Tensor:
        """heist_state_fork: env dst_ids[i] <- env src_ids[i] of this handle in one launch, with no
        blob and no cone rebuild; a source may be named many times.  Returns status [m] uint8 on
        this device: 0 rejected and dst untouched (an id out of range, src == dst, a dst named
        twice or also named as a source), 1 forked with the guard cones copied, 2 forked with
        the cones dst already held kept (dst had the source's layout), 3 some of each."""
        src, dst = self._ids(src_ids, "fork_state"), self._ids(dst_ids, "fork_state")
        if src is None or dst is None:
            raise ValueError("fork_state: src_ids and dst_ids are required")
        if src.numel() != dst.numel():
            raise ValueError("fork_state: %d source ids for %d destination ids" % (src.numel(), dst.numel()))
        m = int(src.numel())
        status = torch.zeros(m, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_state_fork(self._h, nat.ptr(src), nat.ptr(dst), m, nat.ptr(status),
                                                 self._stream()), "heist_state_fork")
        return status

    # -- the layouts as the handle holds them (read from the state blobs, include/heist.h) ----
    def _layout_blobs(self) -> torch.Tensor:
        """save_state()'s blobs [N, bytes] uint8, after a check that they are laid out as camera_records and
        layout_lists slice them: the header's magic and format version 1 (include/heist.h) and this handle's
        capacities."""
        blobs = self.save_state().blobs
        head = blobs[0, :28].cpu().contiguous().view(torch.int32).tolist()
        want = [0x54534548, 1, self.rows, self.cols, self.max_cams, self.max_guards, self.max_path]
        if head != want:
            raise nat.HeistError("state blob header %r is not the format version 1 layout %r that camera_records / "
                                 "layout_lists read" % (head, want))
        return blobs

    def camera_records(self) -> torch.Tensor:
        """Every camera slot as a heist_set_layout cam_params row, float64 [N, max_cams, 6] = (row,
        col, fov_angle, heading, rotation_speed, vision_range) with the heading the camera has now:
        the 32-byte camera records of the state blobs (save_state).  Slots from n_cams[e] up hold
        whatever the handle last kept there.  Reads the envs only."""
        mc = self.max_cams
        blobs = self._layout_blobs()
        rec = blobs[:, 112:112 + 32 * mc].reshape(self.n_envs, mc, 32)
        f = rec[:, :, :24].contiguous().view(torch.float64)              # fov, heading, speed
        i = rec[:, :, 24:].contiguous().view(torch.int16).double()       # row, col, range, rays
        return torch.stack([i[..., 0], i[..., 1], f[..., 0], f[..., 1], f[..., 2], i[..., 2]], -1)

    def layout_lists(self):
        """The envs' layouts as the handle holds them now, in the reference's set_layout format, and
        what each spent: (layouts, spent) with layouts[e] = (walls, cameras, guards) -- the interior
        wall tiles of the grid in row-major order, the filled camera slots with their current
        headings, the filled guard slots with their patrol paths -- read from the state blobs
        (save_state).  set_layouts(layouts, budget=spent) rebuilds the same grids and records; a
        wall that a guard's start tile replaced is not listed, so a rebuild can spend less.  Host
        lists; reads the envs only."""
        mc, mg, mp = self.max_cams, self.max_guards, self.max_path
        n, R, C = self.n_envs, self.rows, self.cols
        blobs = self._layout_blobs().cpu()
        sc = blobs[:, 64:112].contiguous().view(torch.int32).numpy()   # heist_export's 12 scalars
        cams = self.camera_records().cpu().numpy()
        g0 = 112 + 32 * mc
        grec = blobs[:, g0:g0 + 32 * mg].reshape(n, mg, 32)
        gf = grec[:, :, :16].contiguous().view(torch.float64).numpy()  # fov, heading
        gi = grec[:, :, 16:26].contiguous().view(torch.int16).numpy()  # patrol index, step, length, range, rays
        p0 = g0 + 32 * mg
        paths = blobs[:, p0:p0 + 2 * mg * mp].contiguous().view(torch.int16).numpy().reshape(n, mg, mp)
        q0 = p0 + ((2 * mg * mp + 15) & ~15)
        grid = blobs[:, q0:q0 + R * C].numpy().reshape(n, R, C)
        layouts, spent = [], []
        for e in range(n):
            walls = [(int(r), int(c)) for r, c in zip(*np.nonzero(grid[e, 1:R - 1, 1:C - 1] == 1))]
            walls = [(r + 1, c + 1) for r, c in walls]
            cl = [{"row": int(v[0]), "col": int(v[1]), "fov_angle": float(v[2]), "heading": float(v[3]),
                   "rotation_speed": float(v[4]), "vision_range": int(v[5])} for v in cams[e, :sc[e, 8]]]
            gl = []
            for g in range(int(sc[e, 9])):
                ln = int(gi[e, g, 2])
                pts = [(int(v) & 0xff, (int(v) >> 8) & 0xff) for v in paths[e, g, :ln]]
                gl.append({"patrol_path": pts, "speed": int(gi[e, g, 1]), "vision_range": int(gi[e, g, 3]),
                           "fov_angle": float(gf[e, g, 0])})
            layouts.append((walls, cl, gl))
            spent.append(int(sc[e, 11]))
        return layouts, spent

    # -- compact observation records (obs_compact.CompactObs) ---------------------------
    def grid_snapshot(self) -> torch.Tensor:
        """The envs' grids [N, R, C] int8 as they stand now (heist_export's grid alone): what
        heist_obs_expand reads channel 0 from, valid for records packed until the next
        set_layout."""
        gr = torch.empty((self.n_envs, self.rows, self.cols), dtype=torch.int8, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_export(self._h, None, nat.ptr(gr), None, None, None, self._stream()),
                      "heist_export")
        return gr

    def pack_obs(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """heist_obs_pack: observation rows [..., 3, R, C] float32 of this env (one tick's
        [N, 3, R, C], or a step_multi launch's [K, N, 3, R, C]) -> records [..., W] int32, W =
        heist_obs_record_bytes / 4.  out: a contiguous int32 tensor of that shape to write into."""
        from .obs_compact import record_words
        tail = (3, self.rows, self.cols)
        if (tuple(obs.shape[-3:]) != tail or obs.dtype != torch.float32 or obs.device != self.device
                or not obs.is_contiguous()):
            raise ValueError("pack_obs: obs must be a contiguous float32 [..., %d, %d, %d] tensor on %s"
                             % (tail + (self.device,)))
        shape = tuple(obs.shape[:-3]) + (record_words(self.rows, self.cols),)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=self.device)
        elif (tuple(out.shape) != shape or out.dtype != torch.int32 or out.device != self.device
              or not out.is_contiguous()):
            raise ValueError("pack_obs: out must be a contiguous int32 %s tensor on %s" % (shape, self.device))
        n = obs.numel() // (3 * self.rows * self.cols)
        vr, vc = self.config.vault_pos
        with torch.cuda.device(self.device):
            nat.check(nat.lib().heist_obs_pack(nat.ptr(obs), n, self.rows, self.cols, vr, vc, nat.ptr(out),
                                               self._stream()), "heist_obs_pack")
        return out

    def count_samples(self, counter: Optional[torch.Tensor]) -> None:
        """Instrumentation (no reference counterpart): later step/reset calls add the number of
        ray samples env e evaluates to ``counter[e]`` (int64 [n_envs] on this device, zeroed by
        the caller) -- the ALU work figure of SURVEY 8(d).  ``None`` switches counting off."""
        if counter is not None and (counter.dtype != torch.int64 or counter.numel() != self.n_envs
                                    or counter.device != self.device or not counter.is_contiguous()):
            raise ValueError("count_samples: need a contiguous int64 [%d] tensor on %s" % (self.n_envs, self.device))
        nat.check(nat.lib().heist_count_samples(self._h, nat.ptr(counter)), "heist_count_samples")
        self._counter = counter  # keep the buffer alive while the library holds its pointer

    def count_exact_rays(self, counter: Optional[torch.Tensor]) -> None:
        """Instrumentation: later step/reset calls add to ``counter[e]`` the number of env e's
        rays cast on the exact fp64 path (near-tie re-casts of the fp32 fast path, or every
        ray with ``set_ray_mode(1)``).  ``None`` switches counting off."""
        if counter is not None and (counter.dtype != torch.int64 or counter.numel() != self.n_envs
                                    or counter.device != self.device or not counter.is_contiguous()):
            raise ValueError("count_exact_rays: need a contiguous int64 [%d] tensor on %s" % (self.n_envs, self.device))
        nat.check(nat.lib().heist_count_redo(self._h, nat.ptr(counter)), "heist_count_redo")
        self._redo_counter = counter

    def set_ray_mode(self, mode: int) -> None:
        """0 (default): fp32 fast raycast with exact fp64 re-cast of near-tie rays; 1: exact
        fp64 raycast for every ray.  Results are bit-identical; 1 is for parity tests and A/B
        timing."""
        nat.check(nat.lib().heist_set_ray_mode(self._h, int(mode)), "heist_set_ray_mode")

    def set_guard_cones(self, on: bool) -> None:
        """True (default): the next set_layout precomputes every guard's vision cone per
        (patrol point, heading) on the exact path and step/reset OR the cached cone instead
        of raycasting the guard; False: every guard is raycast every tick.  Results are
        bit-identical; takes effect at the next set_layout."""
        nat.check(nat.lib().heist_set_guard_cones(self._h, 1 if on else 0), "heist_set_guard_cones")

    CONFIG_KEYS = ("step_waves", "ray_chunk", "step_occ", "vis_gap", "obs_store", "ray_mode", "probe_mode",
                   "dispatch_order", "split_obs", "guard_cones", "multi_waves", "fan_on", "lean", "interval_fans",
                   "step_lean", "lean_waves")

    def kernel_config(self) -> dict:
        """The handle's effective kernel configuration (heist_get_config): the HEIST_* knobs as
        heist_create resolved them plus later set_* calls.  probe_mode != 0 means the
        profiling step kernel, whose results are wrong by design."""
        out = (ctypes.c_int32 * len(self.CONFIG_KEYS))()
        nat.check(nat.lib().heist_get_config(self._h, ctypes.cast(out, ctypes.c_void_p), len(self.CONFIG_KEYS)),
                  "heist_get_config")
        return dict(zip(self.CONFIG_KEYS, (int(v) for v in out)))

    @property
    def visibility(self) -> torch.Tensor:
        """Current visibility plane [N, R, C] (obs channel 1)."""
        return self.obs[:, 1]
