"""GPU: band synthesis (arx_combine_bands, include/arx.h) -- the band IRs filtered and summed into one IR pair,
bit for bit the documented f64 arithmetic; and the chain render_bands -> combine_bands on the device
(render_broadband).

The bit tests use filters rounded to f32 and widened to f64: the product of two 24-bit significands is exact
in f64, so fma(g, x, acc) is numpy's acc + g * x on bits and the reference needs no fma.  The reference loops
bands and taps in the documented order on vectors over n; it is computed once per shape and shared.  Inputs
are PCG64(11)'s uniform(0, 1) times a 10 % mask as f32, a different draw per ear.  The chain tests use the
12-triangle box and the settings of tests/test_gpu_bands.py.
"""

import numpy as np
import pytest

from audiorenderingv2_amd import ArxError, AudioRenderer, DeviceBuffer, RenderSettings, band_filters, receiver_local
from audiorenderingv2_amd._lib import lib
from audiorenderingv2_amd.scene import Scene, _box_tris

pytestmark = pytest.mark.gpu

INVALID = 1
SHAPES = [(1, 1, 1), (1, 1, 1000), (3, 3, 63), (4, 255, 1000), (5, 1023, 4099), (8, 2047, 1000), (8, 511, 16001),
          (8, 8191, 300)]
GUARD = 256


def f64_sum(ir, g):
    """sum_b sum_k g_b[k] * ir_b[n + c - k] in f64: bands and taps in the documented order, multiply then
    add, on vectors over n.  Samples outside [0, ir_len) are zeros, which leave an accumulator's bits alone."""
    n_bands, n = ir.shape
    taps = g.shape[1]
    c = (taps - 1) // 2
    s = None
    for b in range(n_bands):
        x = np.zeros(n + 2 * taps)
        x[taps:taps + n] = ir[b]
        acc = np.zeros(n)
        for k in range(taps):
            acc = acc + g[b, k] * x[taps + c - k:taps + c - k + n]
        s = acc if b == 0 else s + acc
    return s


def draw_irs(rng, n_bands, n):
    """uniform(0, 1) times a 10 % mask as f32, a draw per ear."""
    return tuple((rng.uniform(0.0, 1.0, (n_bands, n)) * (rng.uniform(0.0, 1.0, (n_bands, n)) < 0.1)).astype(np.float32)
                 for _ in range(2))


class Cases:
    """Inputs, f32-valued filters and reference bits by shape, made once."""

    def __init__(self):
        self.made = {}

    def get(self, shape):
        if shape not in self.made:
            n_bands, taps, n = shape
            rng = np.random.Generator(np.random.PCG64(11))
            irs = draw_irs(rng, n_bands, n)
            g = rng.uniform(-1.0, 1.0, (n_bands, taps)).astype(np.float32).astype(np.float64)
            if shape == (1, 1, 1000):
                g[:] = 1.0
            want = tuple(f64_sum(ir, g).astype(np.float32).view(np.uint32) for ir in irs)
            self.made[shape] = (irs, g, want)
        return self.made[shape]


@pytest.fixture(scope="module")
def cases():
    return Cases()


@pytest.fixture(scope="module")
def bare():
    """A renderer without a scene: the call needs none."""
    r = AudioRenderer(RenderSettings(rays=(4, 4, 1), sample_rate=16000, ir_length_in_seconds=1))
    yield r
    r.close()


def bits(pair):
    return tuple(np.asarray(a).view(np.uint32) for a in pair)


def same_bits(got, want):
    return all(np.array_equal(a, b) for a, b in zip(bits(got), want))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bits(bare, cases, shape):
    irs, g, want = cases.get(shape)
    out = bare.combine_bands(irs, g)
    assert out["ms"] > 0.0 and out["ir"][0].shape == (shape[2],)
    for ear in range(2):
        assert np.array_equal(out["ir"][ear].view(np.uint32), want[ear]), (shape, ear)
    if shape == (1, 1, 1000):  # g = [1.0]: the output is the input
        assert same_bits(out["ir"], bits((irs[0][0], irs[1][0])))
        assert irs[0].any()


def test_host_and_device_pointers_give_the_same_bits(bare, cases):
    shape = (5, 1023, 4099)
    irs, g, want = cases.get(shape)
    bufs = [DeviceBuffer.from_numpy(0, a) for a in (*irs, g)] + [DeviceBuffer(0, shape[2] * 4) for _ in range(2)]
    try:
        out = bare.combine_bands(tuple(bufs[:2]), bufs[2], n_bands=shape[0], ir_len=shape[2], out=tuple(bufs[3:]), taps=shape[1])
        assert out["ir"] == tuple(bufs[3:])
        dev = tuple(b.to_numpy(np.float32, shape[2]) for b in bufs[3:])
        host = bare.combine_bands(irs, g)["ir"]
        assert same_bits(dev, want) and same_bits(host, want)
        # mixed: device IRs, host filters, host outputs
        mixed = bare.combine_bands(tuple(bufs[:2]), g, n_bands=shape[0], ir_len=shape[2])["ir"]
        assert same_bits(mixed, want)
    finally:
        for b in bufs:
            b.close()


@pytest.mark.parametrize("shape", [(3, 3, 63), (4, 255, 1000)], ids=lambda s: "x".join(map(str, s)))
def test_guards_stay_and_inputs_are_unchanged(bare, cases, shape):
    irs, g, want = cases.get(shape)
    n = shape[2]
    ff = np.full(n + 2 * GUARD, 0xFFFFFFFF, np.uint32)
    ins = [DeviceBuffer.from_numpy(0, a) for a in (*irs, g)]
    outs = [DeviceBuffer.from_numpy(0, ff) for _ in range(2)]
    try:
        bare.combine_bands(tuple(ins[:2]), ins[2], n_bands=shape[0], ir_len=n, taps=shape[1],
                           out=tuple(b.ptr + 4 * GUARD for b in outs))
        for ear in range(2):
            got = outs[ear].to_numpy(np.uint32)
            assert np.all(got[:GUARD] == 0xFFFFFFFF) and np.all(got[GUARD + n:] == 0xFFFFFFFF)
            assert np.array_equal(got[GUARD:GUARD + n], want[ear])
            assert np.array_equal(ins[ear].to_numpy(np.float32).view(np.uint32), irs[ear].reshape(-1).view(np.uint32))
        assert np.array_equal(ins[2].to_numpy(np.float64).view(np.uint64), g.reshape(-1).view(np.uint64))
        # host outputs between guards
        host = [ff.copy() for _ in range(2)]
        keep = [a.copy() for a in irs]
        st = lib().arx_combine_bands(bare.handle, irs[0].ctypes.data, irs[1].ctypes.data, shape[0], n, g.ctypes.data, shape[1],
                                     host[0].ctypes.data + 4 * GUARD, host[1].ctypes.data + 4 * GUARD, None)
        assert st == 0
        for ear in range(2):
            assert np.all(host[ear][:GUARD] == 0xFFFFFFFF) and np.all(host[ear][GUARD + n:] == 0xFFFFFFFF)
            assert np.array_equal(host[ear][GUARD:GUARD + n], want[ear])
            assert np.array_equal(keep[ear].view(np.uint32), irs[ear].view(np.uint32))
    finally:
        for b in ins + outs:
            b.close()


def test_scratch_regrows_and_keeps_its_results(cases):
    small, large = (4, 255, 1000), (8, 511, 16001)
    assert lib().arx_debug_combine_bytes(large[2], large[0], large[1]) > lib().arx_debug_combine_bytes(small[2], small[0], small[1])
    r = AudioRenderer(RenderSettings(rays=(4, 4, 1), sample_rate=16000, ir_length_in_seconds=1))
    try:
        first = r.combine_bands(*cases.get(small)[:2])["ir"]
        middle = r.combine_bands(*cases.get(large)[:2])["ir"]
        third = r.combine_bands(*cases.get(small)[:2])["ir"]
        assert same_bits(first, cases.get(small)[2]) and same_bits(middle, cases.get(large)[2])
        assert same_bits(third, bits(first))
    finally:
        r.close()


def test_full_precision_filters(bare):
    """arx_band_filters' own coefficients (products no longer exact): per sample |out - ref| <= 2^-24 |ref| +
    taps * 2^-52 * sum_b sum_k |g_b[k] x_b[m]| -- the f32 rounding, and the worst case of an fma chain
    against a multiply-add chain."""
    taps, n = 1023, 4099
    g = band_filters(16000, [125, 250, 500, 1000, 2000, 3000, 4000], taps)
    irs = draw_irs(np.random.Generator(np.random.PCG64(11)), 8, n)
    out = bare.combine_bands(irs, g)["ir"]
    for ear in range(2):
        ref = f64_sum(irs[ear], g)
        mass = f64_sum(np.abs(irs[ear]), np.abs(g))
        err = np.abs(out[ear].astype(np.float64) - ref)
        bound = 2.0 ** -24 * np.abs(ref) + taps * 2.0 ** -52 * mass
        print(f"ear {ear}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g}, max |ref| = {np.abs(ref).max():.3g}")
        assert np.abs(ref).max() > 0.0
        assert np.all(err <= bound)


# ---- the chain: render_bands -> combine_bands on the device ----

BOX_RAYS = (64, 64, 1)
BOX_EMITTER = (-1.5, 1.2, 0.0)
BOX_LISTENER = ((1.5, 1.2, 0.3), 0.0)
S = dict(sample_rate=16000, base_power=3.62, max_bounces=8, hrtf_absorption_rate=0.5)
CHAIN_CROSSOVERS = [250, 1000, 2500]


def box(table_of):
    """The 12-triangle box of tests/test_gpu_bands.py with PCG64(7)'s table; its scene carries the column
    minimum.  table_of(scene absorption, table) picks the band table to install."""
    walls = _box_tris(np.array([[-3.0, 0.0, -2.0]], np.float32), np.array([[3.0, 3.0, 2.0]], np.float32))
    table = np.random.Generator(np.random.PCG64(7)).uniform(0.05, 0.9, (4, 12)).astype(np.float32)
    scene = Scene(walls, table.min(axis=0), ["wall"] * 12)
    n = BOX_RAYS[0] * BOX_RAYS[1] * BOX_RAYS[2]
    e0 = np.float32(3.62 / (n * 4.18879020478))
    r = AudioRenderer(RenderSettings(**S, rays=BOX_RAYS, energy_thres=float(np.float32(e0 * np.float32(0.02)))), scene=scene,
                      receiver=receiver_local())
    r.set_path_cache(1)
    r.setEmitterPosInOptix(BOX_EMITTER)
    r.setSphereCenterInOptix(*BOX_LISTENER)
    r.set_band_absorption(table_of(scene.tri_abs, table))
    return r


def test_chain_with_equal_bands_is_the_plain_render():
    """Four bands equal to the scene and a bank that sums to a unit impulse: the broadband IR o is the plain
    IR x again, |o - x| <= 2^-23 |x| + 1e-10 max|x| on every sample of both ears."""
    r = box(lambda scene_abs, table: np.tile(scene_abs, (4, 1)))
    try:
        r.render()
        x = r.get_ir()
        o = r.render_broadband(band_filters(16000, CHAIN_CROSSOVERS, 1023))["ir"]
        for ear in range(2):
            assert np.count_nonzero(x[ear]) > 0
            xe, oe = x[ear].astype(np.float64), o[ear].astype(np.float64)
            err = np.abs(oe - xe)
            bound = 2.0 ** -23 * np.abs(xe) + 1e-10 * np.abs(xe).max()
            print(f"ear {ear}: {np.count_nonzero(x[ear])} non-zero bins, max err / bound = {np.max(err / bound):.3g}")
            assert np.all(err <= bound)
    finally:
        r.close()


def test_chain_on_the_device_is_the_chain_through_the_host():
    r = box(lambda scene_abs, table: table)
    try:
        g = band_filters(16000, CHAIN_CROSSOVERS, 1023)
        dev = r.render_broadband(g)
        assert dev["ms"] > 0.0 and dev["render_ms"] > 0.0 and len(dev["acoustics"]) == 4 and len(dev["stats"]) == 4
        band_irs = r.render_bands(irs=True, acoustics=False)["ir"]
        assert all(band_irs[0][b].any() for b in range(4))
        before = (bits(r.get_ir()), r.path_cache_state(queries=True))
        host = r.combine_bands(band_irs, g)["ir"]
        after = (bits(r.get_ir()), r.path_cache_state(queries=True))
        assert same_bits(dev["ir"], bits(host)) and host[0].any()
        assert same_bits(before[0], after[0]) and before[1] == after[1]
        assert not same_bits(host, before[0])  # the broadband IR is not the renderer's own
        # set_ir: the renderer's IR becomes the broadband one
        kept = r.render_broadband(g, set_ir=True)
        assert same_bits(kept["ir"], bits(host))
        assert same_bits(r.get_ir(), bits(kept["ir"]))
    finally:
        r.close()


def test_errors(bare, cases):
    shape = (3, 3, 63)
    irs, g, want = cases.get(shape)
    out = [np.zeros(shape[2], np.float32) for _ in range(2)]
    good = dict(l=irs[0].ctypes.data, r=irs[1].ctypes.data, b=3, n=63, g=g.ctypes.data, t=3, ol=out[0].ctypes.data,
                or_=out[1].ctypes.data)

    def call(handle=None, **over):
        a = {**good, **over}
        st = lib().arx_combine_bands(handle or bare.handle, a["l"], a["r"], a["b"], a["n"], a["g"], a["t"], a["ol"], a["or_"], None)
        return st, lib().arx_last_error()

    assert call()[0] == 0
    bad = [dict(l=None), dict(r=None), dict(g=None), dict(ol=None), dict(or_=None), dict(ol=None, or_=None),
           dict(b=0), dict(b=9), dict(b=-1), dict(t=0), dict(t=2), dict(t=-1), dict(t=8193), dict(t=8192),
           dict(n=0), dict(n=2 ** 31)]
    for over in bad:
        st, msg = call(**over)
        assert st == INVALID and len(msg) > 0, over
    # a caller's own stream, as in arx_render_bands
    other = AudioRenderer(RenderSettings(rays=(4, 4, 1), sample_rate=16000, ir_length_in_seconds=1))
    try:
        own = bare.get_stream()
        bare.set_stream(other.get_stream())
        st, msg = call()
        assert st == INVALID and b"stream" in msg
        bare.set_stream(own)
    finally:
        other.close()
    with pytest.raises(ValueError):
        bare.combine_bands(irs, g[:2])  # the wrapper wants a filter row per band
    with pytest.raises(ArxError):
        bare.combine_bands(irs, np.ones((3, 4)))  # an even number of taps
    # the renderer stays usable
    for o in out:
        o[:] = 0.0
    assert call()[0] == 0 and same_bits(out, want)
