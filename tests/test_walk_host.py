"""CPU: the host side of the walk-through convolution (arx_convolute_walk, include/arx.h) -- how many
blocks a walk has, the even schedule, the documented scratch formula, and the NULL-renderer check."""
import ctypes as C

import numpy as np
import pytest

from audiorenderingv2_amd import walk_blocks, walk_schedule
from audiorenderingv2_amd._lib import lib

INVALID = 1  # ARX_ERR_INVALID_ARGUMENT


def ceil_div(a, b):
    return -(-a // b)


@pytest.mark.parametrize("n_frames,block,ir_len", [(0, 256, 16000),           # no input: only the tail
                                                   (8192, 4096, 16000),       # n_frames a multiple of B
                                                   (1000, 16, 16 * 7 + 1),    # ir_len - 1 a multiple of B
                                                   (2880000, 4096, 96000),    # the measured shape: 704 + 24
                                                   (12345, 1000, 44100), (5, 1, 1), (1, 4096, 4096)])
def test_walk_blocks_is_the_formula(n_frames, block, ir_len):
    want = ceil_div(n_frames, block) + ceil_div(ir_len - 1, block)
    assert walk_blocks(n_frames, block, ir_len) == want
    if (n_frames, block, ir_len) == (2880000, 4096, 96000):
        assert want == 704 + 24


def test_walk_blocks_rejects_bad_sizes():
    assert walk_blocks(100, 0, 16000) == 0
    assert walk_blocks(100, -4, 16000) == 0
    assert walk_blocks(100, 16, 0) == 0


def even(n_in, n_blocks, n_irs):
    out = np.full(n_blocks, -7, np.int32)
    assert lib().arx_walk_even_schedule(n_in, n_blocks, n_irs, out.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    return out


@pytest.mark.parametrize("shape,want", [((10, 13, 3), [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2]),
                                        ((4, 4, 7), [0, 1, 3, 5]),
                                        ((1, 5, 2), [0, 0, 0, 0, 0])])
def test_even_schedule_exact(shape, want):
    assert even(*shape).tolist() == want


@pytest.mark.parametrize("n_in,n_blocks,n_irs", [(10, 13, 3), (4, 4, 7), (1, 5, 2), (704, 728, 64), (64, 70, 64), (7, 7, 1),
                                                 (50, 61, 9)])
def test_even_schedule_properties(n_in, n_blocks, n_irs):
    s = even(n_in, n_blocks, n_irs)
    assert np.all(np.diff(s) >= 0)
    assert s.min() >= 0 and s.max() < n_irs
    assert np.all(s[n_in:] == s[n_in - 1])
    assert s.tolist()[:n_in] == [min(n_irs - 1, b * n_irs // n_in) for b in range(n_in)]
    if n_in >= n_irs:  # every IR is heard
        assert sorted(set(s.tolist())) == list(range(n_irs))


def test_even_schedule_rejects_bad_arguments():
    out = np.zeros(4, np.int32)
    assert lib().arx_walk_even_schedule(4, 4, 0, out.ctypes.data_as(C.POINTER(C.c_int32))) == INVALID
    assert lib().arx_walk_even_schedule(4, 4, 2, None) == INVALID
    assert lib().arx_walk_even_schedule(0, 0, 2, None) == 0


def test_walk_schedule_is_the_even_schedule_over_walk_blocks():
    s = walk_schedule(10 * 16, 16, 3 * 16 + 1, 3)
    assert s.dtype == np.int32 and s.tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2]


def up256(v):
    return (v + 255) // 256 * 256


def documented_bytes(ir_len, B, U, n_blocks, T, F):
    """include/arx.h's formula under arx_convolute_walk."""
    N = 16
    while N < 2 * B:
        N *= 2
    P = ceil_div(ir_len, B)
    terms = [16 * N, 8 * F, 16 * N * P * U, 16 * N * n_blocks, 16 * N * (n_blocks + T), 16 * F * T, 8 * ir_len * U,
             8 * B * n_blocks, 16 * B * n_blocks, 16 * (n_blocks + T)]
    return sum(up256(t) for t in terms)


@pytest.mark.parametrize("args", [(96000, 4096, 64, 728, 63, 4096),   # the measured shape: N = 8192, P = 24
                                  (16000, 1, 2, 14, 1, 1),            # N = 16, the smallest plan; terms below 256 B
                                  (44100, 1000, 4, 14, 4, 600)])      # N - B != B, P = 45
def test_walk_bytes_is_the_documented_formula(args):
    got = int(lib().arx_debug_walk_bytes(*args))
    assert got == documented_bytes(*args)
    assert got % 256 == 0


def test_walk_bytes_rejects_what_the_call_rejects():
    assert lib().arx_debug_walk_bytes(16000, 0, 1, 1, 0, 0) == 0
    assert lib().arx_debug_walk_bytes(16000, 4097, 1, 1, 0, 0) == 0
    assert lib().arx_debug_walk_bytes(100, 256, 1, 1, 0, 0) == 0   # block above ir_len
    assert lib().arx_debug_walk_bytes(16000, 256, 1, 1, 0, 257) == 0


def test_null_renderer_is_an_invalid_argument():
    ir = np.zeros(16, np.float32)
    sched = np.zeros(1, np.int32)
    x = np.zeros(4, np.float64)
    out = np.zeros(8, np.float64)
    st = lib().arx_convolute_walk(None, ir.ctypes.data, ir.ctypes.data, 1, sched.ctypes.data_as(C.POINTER(C.c_int32)), 1,
                                  x.ctypes.data, 4, 4, 0, 1, out.ctypes.data, None)
    assert st == INVALID
    assert b"NULL" in lib().arx_last_error()
    assert lib().arx_debug_set_walk_tile(None, 0) == INVALID
    assert lib().arx_debug_walk_state(None, (C.c_uint64 * 5)()) == INVALID
