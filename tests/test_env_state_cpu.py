"""CPU-side checks of the saved-state container (heist_amd.env_state.EnvState) and of the
trainer's env checkpoint names: no device work -- the blobs are opaque bytes here."""
import inspect

import pytest
import torch

from heist_amd import EnvState
from heist_amd._native import HeistError
from heist_amd.env_state import CONFIG_KEYS, FORMAT_VERSION, env_checkpoint_name, env_checkpoint_path


def _config(**over):
    cfg = {"rows": 20, "cols": 20, "max_cams": 5, "max_guards": 3, "max_path": 8, "guard_cones": 1, "max_steps": 200,
           "start_r": 1, "start_c": 1, "vault_r": 18, "vault_c": 18, "version": FORMAT_VERSION, "bytes": 944}
    cfg.update(over)
    return cfg


def _state(m=6, **over):
    cfg = _config(**over)
    g = torch.Generator().manual_seed(m)
    return EnvState(torch.randint(0, 256, (m, cfg["bytes"]), dtype=torch.uint8, generator=g), cfg)


def test_round_trip_state_dict_and_torch_save(tmp_path):
    st = _state()
    st.extra = {"obs": torch.arange(6.0), "note": "kept"}
    sd = st.state_dict()
    assert sd["format"] == "heist_env_state" and set(CONFIG_KEYS) <= set(sd["config"])
    back = EnvState.from_state_dict(sd)
    assert torch.equal(back.blobs, st.blobs) and back.config == st.config and back.extra["note"] == "kept"
    path = str(tmp_path / "s.pt")
    torch.save(sd, path)
    back = EnvState.from_state_dict(torch.load(path, weights_only=False))
    assert torch.equal(back.blobs, st.blobs) and back.config == st.config
    assert torch.equal(back.extra["obs"], st.extra["obs"])
    st.save(path)
    back = EnvState.load(path)
    assert len(back) == 6 and back.nbytes() == 6 * 944 and back.device.type == "cpu"
    assert torch.equal(back.cpu().blobs, st.blobs) and torch.equal(back.to("cpu").blobs, st.blobs)
    with pytest.raises(HeistError):
        EnvState.from_state_dict({"blobs": st.blobs, "config": st.config})


def test_slicing():
    st = _state(7)
    assert len(st[2]) == 1 and torch.equal(st[2].blobs[0], st.blobs[2])
    assert torch.equal(st[-1].blobs[0], st.blobs[6])
    assert torch.equal(st[1:4].blobs, st.blobs[1:4]) and st[1:4].config == st.config
    assert torch.equal(st[[5, 0, 0]].blobs, st.blobs[[5, 0, 0]])
    mask = torch.tensor([True, False] * 3 + [True])
    assert torch.equal(st[mask].blobs, st.blobs[mask])
    assert torch.equal(st[torch.tensor([3, 1])].blobs, st.blobs[[3, 1]])
    assert st[1:4].blobs.is_contiguous()


def test_malformed_containers_raise():
    cfg = _config()
    with pytest.raises(HeistError):
        EnvState(torch.zeros((2, 960), dtype=torch.uint8), cfg)  # not the configuration's blob size
    with pytest.raises(HeistError):
        EnvState(torch.zeros((2, 944), dtype=torch.int8), cfg)
    with pytest.raises(HeistError):
        EnvState(torch.zeros(944, dtype=torch.uint8), cfg)
    with pytest.raises(HeistError):
        EnvState(torch.zeros((2, 944), dtype=torch.uint8), {k: v for k, v in cfg.items() if k != "max_path"})
    with pytest.raises(HeistError):
        EnvState(torch.zeros((2, 970), dtype=torch.uint8), _config(bytes=970))


@pytest.mark.parametrize("key,value", [("rows", 12), ("cols", 17), ("max_cams", 4), ("max_guards", 2), ("max_path", 16),
                                       ("guard_cones", 0), ("max_steps", 100), ("vault_r", 10), ("version", 2),
                                       ("bytes", 992)])
def test_configuration_mismatch_raises(key, value):
    st = _state()
    st.check(_config())  # the matching handle passes
    with pytest.raises(HeistError) as ei:
        st.check(_config(**{key: value}))
    assert key in str(ei.value)


def test_env_checkpoint_names():
    assert env_checkpoint_name(150) == "env_ep150.pt"
    assert env_checkpoint_name(150, rank=0, world_size=1) == "env_ep150.pt"
    assert [env_checkpoint_name(150, r, 4) for r in range(4)] == ["env_ep150_rank%d.pt" % r for r in range(4)]
    assert env_checkpoint_path("ck", 7, 1, 2).replace("\\", "/") == "ck/env_ep7_rank1.pt"


def test_trainer_option_defaults_off():
    from heist_amd.training import AdversarialTrainer
    p = inspect.signature(AdversarialTrainer.__init__).parameters["checkpoint_env"]
    assert p.default is False
