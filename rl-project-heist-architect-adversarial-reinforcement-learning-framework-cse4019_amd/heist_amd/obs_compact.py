"""CompactObs -- observations kept as records (include/heist.h, heist_obs_pack / heist_obs_expand).

An observation [3, R, C] float32 is the layout's grid / 5, one visibility bit per cell and the
solver's cell, so a buffer of M observations is M records of 64 B (20 x 20; 144 B at 32 x 32)
plus one int8 grid per env, 75-85x less than the float32 tensors.  Selecting samples gathers
records; expand() rebuilds the selected observations bit for bit in one launch.  The grid
snapshot belongs to the layouts the records were packed under: take it (HeistEnv.grid_snapshot)
before the env's layouts change, after which the records stay valid without the env.
"""
from typing import Optional, Tuple

import torch

from . import _native as nat


def record_words(rows: int, cols: int) -> int:
    """uint32 words of one record (heist_obs_record_bytes / 4)."""
    b = nat.lib().heist_obs_record_bytes(int(rows), int(cols))
    nat.check(0 if b > 0 else b, "heist_obs_record_bytes")
    return b // 4


def record_cells(records: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    """The Solver's cell of each record, [..., 2] int32 (row, col), from the records' position word
    (word ceil(rows * cols / 32): row | col << 8): the decision records of a rollout give
    HeistEnv.plan_q's pos directly.  rows and cols are needed because the padded record width does
    not determine the position word's index.  Pure torch, any device."""
    word = records[..., (int(rows) * int(cols) + 31) // 32]
    return torch.stack([word & 0xFF, (word >> 8) & 0xFF], -1).to(torch.int32)


class CompactObs:
    """M observation records: records [M, W] int32, rec_env [M] int32 (each record's env), the
    grid snapshot [n_envs, R, C] int8 they were packed under, (rows, cols, vault) and an optional
    leading shape (T, N) with T * N == M (a time-major rollout buffer)."""

    def __init__(self, records: torch.Tensor, rec_env: torch.Tensor, grid: torch.Tensor, rows: int, cols: int,
                 vault: Tuple[int, int], lead: Optional[Tuple[int, int]] = None):
        W = record_words(rows, cols)
        records = records.reshape(-1, W)
        if records.dtype != torch.int32 or rec_env.dtype != torch.int32 or grid.dtype != torch.int8:
            raise ValueError("CompactObs: records / rec_env must be int32 and grid int8")
        if rec_env.numel() != records.shape[0] or tuple(grid.shape[1:]) != (rows, cols):
            raise ValueError("CompactObs: %d records need %d envs entries and a [n_envs, %d, %d] grid"
                             % (records.shape[0], records.shape[0], rows, cols))
        if lead is not None and int(lead[0]) * int(lead[1]) != records.shape[0]:
            raise ValueError("CompactObs: leading shape %s does not hold %d records" % (tuple(lead), records.shape[0]))
        self.records = records.contiguous()
        self.rec_env = rec_env.reshape(-1).contiguous()
        self.grid = grid.contiguous()
        self.rows, self.cols, self.vault = int(rows), int(cols), (int(vault[0]), int(vault[1]))
        self.lead = None if lead is None else (int(lead[0]), int(lead[1]))

    @classmethod
    def of_env(cls, env, records: torch.Tensor, grid: Optional[torch.Tensor] = None) -> "CompactObs":
        """Records packed from env's own observations: [N, W] (one tick) or [T, N, W] (tick-major,
        e.g. a step_multi launch's rows); grid defaults to env.grid_snapshot() now."""
        W = record_words(env.rows, env.cols)
        if records.shape[-1] != W or records.numel() % (env.n_envs * W):
            raise ValueError("CompactObs.of_env: expected [..., %d, %d] records" % (env.n_envs, W))
        T = records.numel() // (env.n_envs * W)
        rec_env = torch.arange(env.n_envs, dtype=torch.int32, device=records.device).repeat(T)
        return cls(records, rec_env, env.grid_snapshot() if grid is None else grid, env.rows, env.cols,
                   env.config.vault_pos, lead=(T, env.n_envs) if records.dim() == 3 else None)

    def __len__(self) -> int:
        return int(self.records.shape[0])

    def nbytes(self) -> int:
        """Device bytes held: records, rec_env and the grid snapshot."""
        return sum(int(t.numel()) * t.element_size() for t in (self.records, self.rec_env, self.grid))

    def flat(self) -> "CompactObs":
        """The same records without the leading shape (record t * N + e is [t, e])."""
        return CompactObs(self.records, self.rec_env, self.grid, self.rows, self.cols, self.vault)

    def __getitem__(self, key) -> "CompactObs":
        """Select records by an index tensor (int64, or a bool mask) over the flat records, or by a
        (t_i, e_i) pair of index tensors over the leading shape: gathers records, never
        observations."""
        if isinstance(key, tuple):
            if len(key) != 2 or self.lead is None:
                raise IndexError("CompactObs: a (t_i, e_i) pair needs a [T, N] leading shape")
            key = key[0].to(torch.int64) * self.lead[1] + key[1].to(torch.int64)
        return CompactObs(self.records[key], self.rec_env[key], self.grid, self.rows, self.cols, self.vault)

    def expand(self, index: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Observations [m, 3, R, C] float32 of the records index selects (int64 into the flat
        records; None: all of them, in order): one heist_obs_expand launch on the current
        stream."""
        dev = self.records.device
        if index is not None:
            index = index.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        m = len(self) if index is None else int(index.numel())
        out = torch.empty((m, 3, self.rows, self.cols), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            nat.check(nat.lib().heist_obs_expand(
                nat.ptr(self.records), len(self), nat.ptr(self.rec_env), nat.ptr(index), m, nat.ptr(self.grid),
                int(self.grid.shape[0]), self.rows, self.cols, self.vault[0], self.vault[1], nat.ptr(out),
                nat.stream(dev)), "heist_obs_expand")
        return out
