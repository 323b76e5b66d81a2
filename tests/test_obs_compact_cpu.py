"""CPU-side checks of the compact observation record ABI (include/heist.h): record sizes,
argument validation and exported symbols -- no device work."""
import ctypes

import pytest

from heist_amd import _build, _native


@pytest.mark.parametrize("rows,cols,nbytes", [(20, 20, 64), (32, 32, 144), (13, 17, 32), (10, 10, 32), (64, 64, 528)])
def test_record_bytes(rows, cols, nbytes):
    assert _native.lib().heist_obs_record_bytes(rows, cols) == nbytes


@pytest.mark.parametrize("rows,cols", [(0, 20), (20, 0), (65, 20), (20, 65)])
def test_record_bytes_rejects_bad_sizes(rows, cols):
    lib = _native.lib()
    assert lib.heist_obs_record_bytes(rows, cols) < 0
    assert b"rows" in lib.heist_last_error()
    from heist_amd.obs_compact import record_words
    with pytest.raises(_native.HeistError):
        record_words(rows, cols)


def test_symbols_exported_and_bound():
    lib = ctypes.CDLL(_build.LIB_PATH)
    for name in ("heist_obs_record_bytes", "heist_obs_pack", "heist_obs_expand"):
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES and name in _native.header_functions()


def test_pack_expand_validate_arguments_without_device():
    """Bad sizes fail with HEIST_EINVAL before any device work; n = 0 and m = 0 are no-ops."""
    lib = _native.lib()
    assert lib.heist_obs_pack(None, 4, 0, 20, 0, 0, None, None) == 100000
    assert lib.heist_obs_pack(None, 4, 20, 65, 0, 0, None, None) == 100000
    assert lib.heist_obs_pack(None, 4, 20, 20, 20, 0, None, None) == 100000  # vault outside the grid
    assert lib.heist_obs_pack(None, -1, 20, 20, 18, 18, None, None) == 100000
    assert lib.heist_obs_pack(None, 4, 20, 20, 18, 18, None, None) == 100000  # null pointers
    assert lib.heist_obs_pack(None, 0, 20, 20, 18, 18, None, None) == 0
    assert lib.heist_obs_expand(None, 0, None, None, 4, None, 1, 65, 20, 0, 0, None, None) == 100000
    assert lib.heist_obs_expand(None, 0, None, None, 4, None, 1, 20, 20, 0, 20, None, None) == 100000
    assert lib.heist_obs_expand(None, 0, None, None, -1, None, 1, 20, 20, 18, 18, None, None) == 100000
    assert lib.heist_obs_expand(None, 0, None, None, 4, None, 1, 20, 20, 18, 18, None, None) == 100000
    assert lib.heist_obs_expand(None, 0, None, None, 0, None, 1, 20, 20, 18, 18, None, None) == 0


def test_obs_storage_defaults_to_full():
    """The trainer option exists and leaves the default storage as it was."""
    import inspect
    from heist_amd.training import AdversarialTrainer
    sig = inspect.signature(AdversarialTrainer.__init__)
    assert sig.parameters["obs_storage"].default == "full"
