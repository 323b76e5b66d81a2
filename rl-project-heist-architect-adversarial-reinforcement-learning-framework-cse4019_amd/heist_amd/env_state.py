"""EnvState -- saved env states (include/heist.h, heist_state_save / heist_state_load).

One blob restates one env: its layout and everything reset / step read and write, about 1 KB at
20 x 20.  An EnvState is m blobs as a [m, bytes] uint8 tensor plus the configuration they were
saved under (the heist_create arguments and the guard-cone setting a handle must share to load
them; HeistEnv.state_config).  It is plain data: it moves between devices, slices, and goes
through torch.save as a state_dict.  The device checks each blob's own header again at load.
"""
import os
from typing import Dict, Optional

import torch

from ._native import HeistError

FORMAT_VERSION = 1
# the handle properties a blob depends on (the blob header's words, in order, after magic and version)
CONFIG_KEYS = ("rows", "cols", "max_cams", "max_guards", "max_path", "guard_cones", "max_steps", "start_r", "start_c",
               "vault_r", "vault_c")


class EnvState:
    """m saved envs: blobs [m, bytes] uint8 (any device), config (CONFIG_KEYS -> int, plus
    "version" and "bytes"), and extra: a dict of caller data kept alongside (tensors follow .to)."""

    def __init__(self, blobs: torch.Tensor, config: Dict[str, int], extra: Optional[dict] = None):
        config = {k: int(v) for k, v in dict(config).items()}
        missing = [k for k in CONFIG_KEYS + ("version", "bytes") if k not in config]
        if missing:
            raise HeistError("EnvState: configuration lacks %s" % ", ".join(missing))
        if blobs.dtype != torch.uint8 or blobs.dim() != 2 or int(blobs.shape[1]) != config["bytes"]:
            raise HeistError("EnvState: blobs must be a [m, %d] uint8 tensor, got %s %s"
                             % (config["bytes"], blobs.dtype, tuple(blobs.shape)))
        if config["bytes"] % 16:
            raise HeistError("EnvState: blob size %d is not a multiple of 16" % config["bytes"])
        self.blobs = blobs.contiguous()
        self.config = config
        self.extra = dict(extra or {})

    def __len__(self) -> int:
        return int(self.blobs.shape[0])

    @property
    def device(self) -> torch.device:
        return self.blobs.device

    def nbytes(self) -> int:
        return int(self.blobs.numel())

    def to(self, device) -> "EnvState":
        extra = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in self.extra.items()}
        return EnvState(self.blobs.to(device), self.config, extra)

    def cpu(self) -> "EnvState":
        return self.to("cpu")

    def __getitem__(self, key) -> "EnvState":
        """Blobs by an int, a slice, a list or an index / bool tensor (extra is not carried: it
        describes the whole batch)."""
        if isinstance(key, int):
            key = slice(key, key + 1) if key != -1 else slice(-1, None)
        elif isinstance(key, (list, tuple)):
            key = torch.as_tensor(key, dtype=torch.int64, device=self.blobs.device)
        return EnvState(self.blobs[key], self.config)

    def check(self, config: Dict[str, int], what: str = "load_state") -> None:
        """Raise HeistError unless these blobs were saved under `config` (a handle's state_config)."""
        bad = [k for k in CONFIG_KEYS + ("version", "bytes") if int(config.get(k, -1)) != self.config[k]]
        if bad:
            raise HeistError("%s: the saved states do not fit this env: %s" % (what, ", ".join(
                "%s saved %d, here %s" % (k, self.config[k], config.get(k)) for k in bad)))

    def state_dict(self) -> dict:
        return {"format": "heist_env_state", "blobs": self.blobs, "config": dict(self.config), "extra": dict(self.extra)}

    @classmethod
    def from_state_dict(cls, sd: dict) -> "EnvState":
        if not isinstance(sd, dict) or sd.get("format") != "heist_env_state":
            raise HeistError("EnvState.from_state_dict: not an EnvState state_dict")
        return cls(sd["blobs"], sd["config"], sd.get("extra"))

    def save(self, path: str) -> None:
        torch.save(self.cpu().state_dict(), path)

    @classmethod
    def load(cls, path: str, map_location="cpu") -> "EnvState":
        return cls.from_state_dict(torch.load(path, map_location=map_location, weights_only=False))

    def __repr__(self):
        c = self.config
        return "EnvState(%d envs x %d B, %dx%d, cams<=%d guards<=%d path<=%d, %s)" % (
            len(self), c["bytes"], c["rows"], c["cols"], c["max_cams"], c["max_guards"], c["max_path"], self.device)


def env_checkpoint_name(episode: int, rank: int = 0, world_size: int = 1) -> str:
    """File name of the trainer's env checkpoint of `episode` (AdversarialTrainer(checkpoint_env=
    True)): env_ep{N}.pt, and one shard per rank, env_ep{N}_rank{r}.pt, in a multi-rank run."""
    if world_size > 1:
        return "env_ep%d_rank%d.pt" % (int(episode), int(rank))
    return "env_ep%d.pt" % int(episode)


def env_checkpoint_path(save_dir: str, episode: int, rank: int = 0, world_size: int = 1) -> str:
    return os.path.join(save_dir, env_checkpoint_name(episode, rank, world_size))
