"""The streaming convolution's crossfade weights (arx_stream_fade_weights, host only): the table a
stream with a crossfade uploads for its transition blocks."""
import ctypes as C

import numpy as np
import pytest

from audiorenderingv2_amd import _lib
from audiorenderingv2_amd.renderer import fade_weights

LINEAR, HANN = 0, 1


@pytest.mark.parametrize("shape", ["linear", "hann"])
@pytest.mark.parametrize("F", [1, 2, 7, 4096])
def test_weights_match_the_formulas(shape, F):
    w = fade_weights(shape, F)
    assert w.shape == (F,) and w.dtype == np.float64
    t = (np.arange(F) + 0.5) / F
    want = t if shape == "linear" else 0.5 - 0.5 * np.cos(np.pi * t)
    assert np.abs(w - want).max() <= 1e-15
    assert np.all(w > 0.0) and np.all(w < 1.0)
    assert np.all(np.diff(w) > 0.0)
    assert np.abs(w + w[::-1] - 1.0).max() <= 1e-15
    # the shape's number names the same table
    assert np.array_equal(fade_weights({"linear": LINEAR, "hann": HANN}[shape], F), w)


def test_weights_reject_bad_arguments():
    L = _lib.lib()
    w = np.full(4, -1.0)
    p = w.ctypes.data_as(C.POINTER(C.c_double))
    for shape, F, buf in [(HANN, 0, p), (LINEAR, -3, p), (2, 4, p), (-1, 4, p), (HANN, 4, None)]:
        assert L.arx_stream_fade_weights(shape, F, buf) == 1, (shape, F)  # ARX_ERR_INVALID_ARGUMENT
    assert np.all(w == -1.0)  # nothing written
    with pytest.raises(_lib.ArxError):
        fade_weights("hann", 0)
    with pytest.raises(_lib.ArxError):
        fade_weights("cosine", 4)
