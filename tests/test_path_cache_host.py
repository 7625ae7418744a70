"""Host side of the path cache (no GPU needed): the size of its records and the argument checks of its
two renderer calls (arx_debug_set_path_cache, arx_debug_path_cache_state; include/arx.h)."""
import ctypes as C

import pytest

from audiorenderingv2_amd import _lib

RECORD_BYTES = 24  # t, id, unit, v, w, det


@pytest.mark.parametrize("n,bounces", [(0, 8), (1, 1), (36_000, 8), (600_000, 8), (10**6, 16), (2 * 10**7, 16)])
def test_cache_bytes(n, bounces):
    got = _lib.lib().arx_debug_path_cache_bytes(n, bounces)
    assert got == n * bounces * RECORD_BYTES
    if (n, bounces) == (10**6, 16):
        assert got == 384_000_000       # C3: under the default cap of 1 GiB
    if (n, bounces) == (2 * 10**7, 16):
        assert got > 1 << 30            # C4: over it


def test_null_renderer_is_rejected():
    st, nb, nq = C.c_int32(), C.c_uint64(), C.c_uint64()
    assert _lib.lib().arx_debug_set_path_cache(None, 1, 1 << 30) == 1  # ARX_ERR_INVALID_ARGUMENT
    assert _lib.lib().arx_debug_path_cache_state(None, C.byref(st), C.byref(nb), C.byref(nq)) == 1
    with pytest.raises(_lib.ArxError):
        _lib.check(_lib.lib().arx_debug_set_path_cache(None, 0, 0))
