"""Host side of the path filter (no GPU needed): the size of its planes and lists, the argument checks of
its two renderer calls (arx_debug_set_path_filter, arx_debug_path_filter_state; include/arx.h), and the
path cache's own byte figure, which the filter leaves alone."""
import ctypes as C

import pytest

from audiorenderingv2_amd import _lib

SEGMENT = 16  # pos.x, pos.y, pos.z, dist: one row per query and one more per ray
STATE = 16    # dir.x, dir.y, dir.z, e
PER_RAY = 2   # queries run and flags
CAND = 16     # a candidate list's entry (mask, slot)
HEAD = 16     # behind the list, one head per 1024 slots (a block of the filter kernel)


def want(n, bounces, lists):
    return n * ((bounces + 1) * SEGMENT + bounces * STATE + PER_RAY) + lists * (n * CAND + HEAD * ((n + 1023) // 1024))


@pytest.mark.parametrize("lists", [0, 1, 2])
@pytest.mark.parametrize("n,bounces", [(0, 8), (1, 1), (36_000, 8), (600_000, 8), (10**6, 16), (2 * 10**7, 64)])
def test_filter_bytes(n, bounces, lists):
    got = _lib.lib().arx_debug_path_filter_bytes(n, bounces, lists)
    assert got == want(n, bounces, lists)
    assert got == n * (32 * bounces + 18) + lists * (16 * n + 16 * -(-n // 1024))
    if (n, bounces, lists) == (10**6, 16, 2):
        assert got == 562_031_264  # C3 with two frames in flight: 32 B per query, 18 B per ray, two lists


@pytest.mark.parametrize("n,bounces", [(0, 8), (36_000, 8), (10**6, 16)])
def test_cache_bytes_are_the_records_alone(n, bounces):
    assert _lib.lib().arx_debug_path_cache_bytes(n, bounces) == n * bounces * 24


def test_null_renderer_is_rejected():
    fl, nb, cr, cq = C.c_int32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert _lib.lib().arx_debug_set_path_filter(None, 1) == 1  # ARX_ERR_INVALID_ARGUMENT
    assert _lib.lib().arx_debug_path_filter_state(None, C.byref(fl), C.byref(nb), C.byref(cr), C.byref(cq)) == 1
    with pytest.raises(_lib.ArxError):
        _lib.check(_lib.lib().arx_debug_set_path_filter(None, 0))
