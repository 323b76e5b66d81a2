"""CPU-side checks of the record-emitting K-tick launch's ABI (include/heist.h:
heist_step_records_direct, heist_step_multi_records): exported symbols, bindings and the handle
check -- no device work."""
import ctypes
import inspect

from heist_amd import _build, _native

NAMES = ("heist_step_records_direct", "heist_step_multi_records")


def test_symbols_exported_and_bound():
    lib = ctypes.CDLL(_build.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES and name in _native.header_functions()
    # heist_step_multi's arguments with obs_scratch before the stream
    multi, rec = _native.SIGNATURES["heist_step_multi"], _native.SIGNATURES["heist_step_multi_records"]
    assert rec[0] is multi[0] and rec[1] == multi[1][:-1] + [ctypes.c_void_p] + multi[1][-1:]


def test_null_handle():
    lib = _native.lib()
    assert lib.heist_step_multi_records(None, 1, None, None, None, None, None, None, 1, None, None) == 100000  # HEIST_EINVAL
    assert b"handle" in lib.heist_last_error()
    assert lib.heist_step_records_direct(None) == -1


def test_abi_version_unchanged():
    assert _native.lib().heist_abi_version() == 5


def test_python_surface():
    from heist_amd import HeistEnv
    assert isinstance(inspect.getattr_static(HeistEnv, "records_direct"), property)
    sig = inspect.signature(HeistEnv.step_multi_records)
    assert list(sig.parameters)[1:] == ["actions", "records_out", "auto_reset", "reward64"]
    assert sig.parameters["records_out"].default is None and sig.parameters["reward64"].default is False
