"""heist_amd -- MI355X-native hot path of the Heist Architect adversarial RL game.

Batched environment step/reset, layout BFS, GAE and the clipped-PPO loss run as
hand-written HIP kernels for gfx950 behind the C ABI in include/heist.h
(libheist_hip.so); this package mirrors the reference's Python API on top.
"""
__version__ = "0.1.0"

from .environment import EnvironmentConfig, HeistEnvironment  # noqa: F401
from .vec_env import (HeistEnv, LayoutBatch, PlanField, PlanMasked, PlanPlace, PlanPlay, PlanQ, PlanResult,  # noqa: F401
                      PlanValue, PlanWalls, STATUS_NAMES)
from .obs_compact import CompactObs, record_cells  # noqa: F401
from .env_state import EnvState  # noqa: F401
from .search import (ExpertData, GreedyAdversary, LookaheadResult, PlacementScan, PlanAblation, RelocationScan,  # noqa: F401
                     ablation_masks, architect_patrol, camera_candidates, exhaustive_lookahead, expert_data,
                     expert_labels, expert_rollout, follow_field, greedy_adversary, greedy_cameras, greedy_pick,
                     guard_candidates, guard_placement_scan, placement_scan, play_table, q_values, relocation_scan)
from .search import (GreedyWalls, WallAblation, WallScan, greedy_walls, wall_ablation_edits,  # noqa: F401
                     wall_candidates, wall_placement_scan)
