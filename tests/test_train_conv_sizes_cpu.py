"""The fp32-MFMA training convolutions' size dispatch through the C ABI (host code only, no GPU):
which grids heist_train_conv_supported accepts, and that heist_train_conv_partial_floats is
the number of weight-gradient chunks the kernels count (40 bands of 4 rows at 20 x 20, 48
bands of 2 rows at 32 x 32) times the layer's partial size."""
import pytest

from heist_amd import _build, _native

# partial floats per chunk: row tiles x column tiles x 256 + the bias (csrc/heist_train_conv.hip)
WSZ = {1: 2 * 2 * 256 + 32, 2: 4 * 18 * 256 + 64, 3: 4 * 36 * 256 + 64}


@pytest.fixture(scope="module")
def lib():
    if _build.needs_build():
        _build.build()
    return _native.lib()


def test_supported_sizes(lib):
    assert lib.heist_train_conv_supported(20, 20) == 1
    assert lib.heist_train_conv_supported(32, 32) == 1
    for r, c in ((10, 10), (16, 16), (32, 20), (20, 32), (64, 64), (0, 0)):
        assert lib.heist_train_conv_supported(r, c) == 0, (r, c)
        assert lib.heist_train_conv_partial_floats(3, 8, r, c) < 0, (r, c)


@pytest.mark.parametrize("R,bands,chunk", [(20, 5, 40), (32, 16, 48)])
def test_partial_floats_follow_the_chunk(lib, R, bands, chunk):
    for n in (0, 1, 3, 8, 37, 130, 6400, 16384):
        nchunks = (n * bands + chunk - 1) // chunk
        for layer in (1, 2, 3):
            assert lib.heist_train_conv_partial_floats(layer, n, R, R) == nchunks * WSZ[layer], (layer, n)
    assert lib.heist_train_conv_partial_floats(4, 8, R, R) < 0
    assert lib.heist_train_conv_partial_floats(1, -1, R, R) < 0
