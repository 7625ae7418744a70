"""Host side of the longest-first ray pool (no GPU needed): the helpers the trace kernel and the pool's
sort share (arx_layout.hpp pool_static_rays, ray_cost16), reached through arx_debug_ray_order_host."""
import ctypes as C

import pytest

from audiorenderingv2_amd import _lib


def host(n=0, dyn_share=0, steps=0):
    n_static, cost16, share = C.c_uint64(), C.c_uint32(), C.c_uint32()
    _lib.check(_lib.lib().arx_debug_ray_order_host(n, dyn_share, steps, C.byref(n_static), C.byref(cost16), C.byref(share)))
    return int(n_static.value), int(cost16.value), int(share.value)


@pytest.mark.parametrize("n", [1, 255, 256, 491_520, 10**7])
def test_static_rays_helper_is_the_kernels_expression(n):
    """trace_kernel deals rays [0, n - ((n * dyn_share) >> 8)) out statically; the sort starts at the
    same slot.  The build's own share, the experiment shares of the A/B, none and all."""
    build_share = host()[2]
    assert 0 < build_share <= 256
    for share in {build_share, 0, 128, 160, 192, 256}:
        got = host(n=n, dyn_share=share)[0]
        assert got == n - ((n * share) >> 8), (n, share)
        assert 0 <= got <= n


def test_ray_cost_saturates_at_16_bits():
    for steps, want in [(0, 0), (1, 1), (566, 566), (65534, 65534), (65535, 65535), (65536, 65535), (65537, 65535),
                        (131071, 65535), (1 << 20, 65535), (0xFFFFFFFF, 65535)]:
        assert host(steps=steps)[1] == want, steps
