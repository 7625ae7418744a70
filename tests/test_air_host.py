"""Host: air absorption's definitions (include/arx.h "Air absorption") -- ISO 9613-1's pure-tone formula
(arx_air_absorption_iso9613), the attenuation table (arx_air_attenuation_host) and the table's size
(arx_debug_air_bytes).  Plain C++, no device.

Tolerances, each from the number formats and not from the code under test:
  * the five check values of include/arx.h's formula are printed to 4 decimals of dB/km: 2e-4 relative;
  * the numpy restatement runs the same f64 operations in the same order, and pow / exp may differ in their
    last bits between two libms: 1e-12 relative;
  * the table is (float)exp(x) of one f64 expression; libm's exp is not correctly rounded, so two libms can
    round to neighbouring floats: 1 f32 ulp.  Everything else about the table is exact.
"""
import ctypes as C

import numpy as np
import pytest

from audiorenderingv2_amd import ArxError, air_absorption_iso9613, air_attenuation
from audiorenderingv2_amd._lib import lib

INVALID = 1
OCTAVES = [63.0, 125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0]


# ---------------------------------------------------------------- ISO 9613-1 ---
def iso_numpy(f, t_c, rh, p_kpa):
    """The formula of include/arx.h in numpy f64, operation for operation."""
    f = np.asarray(f, np.float64)
    T, T0, T01, pr = np.float64(t_c) + 273.15, 293.15, 273.16, 101.325
    p = np.float64(p_kpa) / pr
    c = -6.8346 * np.power(T01 / T, 1.261) + 4.6151
    h = np.float64(rh) * np.power(10.0, c) / p
    tr = T / T0
    fro = p * (24.0 + 4.04e4 * h * (0.02 + h) / (0.391 + h))
    frn = p * np.power(tr, -0.5) * (9.0 + 280.0 * h * np.exp(-4.170 * (np.power(tr, -1.0 / 3.0) - 1.0)))
    f2 = f * f
    return 8.686 * f2 * (1.84e-11 / p * np.power(tr, 0.5) +
                         np.power(tr, -2.5) * (0.01275 * np.exp(-2239.1 / T) / (fro + f2 / fro) +
                                               0.1068 * np.exp(-3352.0 / T) / (frn + f2 / frn)))


CHECK_VALUES = [(20.0, 70.0, 1000.0, 4.9778), (20.0, 70.0, 8000.0, 77.6332), (20.0, 50.0, 1000.0, 4.6647),
                (20.0, 50.0, 4000.0, 29.6655), (15.0, 20.0, 2000.0, 28.3103)]


@pytest.mark.parametrize("t_c,rh,f,db_per_km", CHECK_VALUES)
def test_iso9613_check_values(t_c, rh, f, db_per_km):
    got = air_absorption_iso9613([f], t_c, rh)[0] * 1000.0
    print(f"{t_c} C {rh} % {f} Hz: {got:.6f} dB/km, expected {db_per_km}")
    assert abs(got - db_per_km) <= 2e-4 * db_per_km


@pytest.mark.parametrize("t_c,rh,p_kpa", [(20.0, 50.0, 101.325), (20.0, 70.0, 101.325), (15.0, 20.0, 101.325),
                                          (-20.0, 0.0, 60.0), (50.0, 100.0, 200.0), (0.0, 35.5, 85.0)])
def test_iso9613_equals_the_numpy_restatement(t_c, rh, p_kpa):
    f = np.array(OCTAVES + [20.0, 31.5, 16000.0, 123.456], np.float64)
    got = air_absorption_iso9613(f, t_c, rh, p_kpa)
    want = iso_numpy(f, t_c, rh, p_kpa)
    err = np.abs(got - want) / want
    print(f"{t_c} C {rh} % {p_kpa} kPa: largest relative difference {err.max():.3e}")
    assert got.shape == f.shape and np.all(np.isfinite(got)) and np.all(got > 0)
    assert err.max() <= 1e-12


def test_iso9613_grows_with_frequency():
    a = air_absorption_iso9613(OCTAVES, 20.0, 50.0)
    assert np.all(np.diff(a) > 0), a


def test_iso9613_defaults_and_empty():
    assert np.array_equal(air_absorption_iso9613([1000.0]), air_absorption_iso9613([1000.0], 20.0, 50.0, 101.325))
    assert air_absorption_iso9613(np.zeros(0)).shape == (0,)


BAD_ISO = [dict(temperature_c=-20.001), dict(temperature_c=50.001), dict(temperature_c=np.nan), dict(temperature_c=np.inf),
           dict(relative_humidity=-0.001), dict(relative_humidity=100.001), dict(relative_humidity=np.nan),
           dict(pressure_kpa=0.0), dict(pressure_kpa=-1.0), dict(pressure_kpa=200.001), dict(pressure_kpa=np.nan),
           dict(pressure_kpa=np.inf), dict(freqs_hz=[1000.0, 0.0]), dict(freqs_hz=[-5.0]), dict(freqs_hz=[np.nan]),
           dict(freqs_hz=[1000.0, np.inf])]


@pytest.mark.parametrize("bad", BAD_ISO, ids=[f"{k}={v}" for d in BAD_ISO for k, v in d.items()])
def test_iso9613_rejects(bad):
    kw = dict(freqs_hz=[1000.0], temperature_c=20.0, relative_humidity=50.0, pressure_kpa=101.325)
    kw.update(bad)
    with pytest.raises(ArxError) as e:
        air_absorption_iso9613(**kw)
    assert e.value.status == INVALID


def test_iso9613_null_pointers():
    dp = C.POINTER(C.c_double)
    f = np.array([1000.0])
    out = np.zeros(1)
    fn = lib().arx_air_absorption_iso9613
    assert fn(20.0, 50.0, 101.325, None, 1, out.ctypes.data_as(dp)) == INVALID
    assert fn(20.0, 50.0, 101.325, f.ctypes.data_as(dp), 1, None) == INVALID
    assert fn(20.0, 50.0, 101.325, f.ctypes.data_as(dp), -1, out.ctypes.data_as(dp)) == INVALID
    assert fn(20.0, 50.0, 101.325, None, 0, None) == 0  # nothing asked for


# ---------------------------------------------------------- the attenuation table ---
def table_numpy(alpha, sample_rate, ir_len):
    """(ir_len, n) f32: the definition's expression in numpy f64, operation for operation."""
    k = np.arange(ir_len, dtype=np.float64)
    d = (k * 343.0) / np.float64(sample_rate)
    a = np.asarray(alpha, np.float64)
    return np.exp(-((a[None, :] * 0.23025850929940458) * d[:, None])).astype(np.float32)


def ulps(a, b):
    """The distance of two arrays of non-negative finite f32 in units in the last place."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


TABLE_CASES = [((0.0, 0.05, 0.3), 16000, 4001, 4), ((0.0, 0.05, 0.3), 16000, 1000, 8),
               (tuple(0.04 * b for b in range(8)), 16000, 3000, 8), ((0.02,), 2500, 2500, 4),
               ((0.0046647, 0.0296655, 0.105, 2.5), 44100, 5000, 4), ((1e-300, 700.0), 48000, 600, 4)]


@pytest.mark.parametrize("alpha,sample_rate,ir_len,width", TABLE_CASES)
def test_table_against_numpy(alpha, sample_rate, ir_len, width):
    n = len(alpha)
    t = air_attenuation(alpha, sample_rate, ir_len, width)
    assert t.shape == (ir_len, width) and t.dtype == np.float32
    filled = width if n == 1 else n
    want = table_numpy(alpha if n > 1 else alpha * width, sample_rate, ir_len)
    d = ulps(t[:, :filled], want[:, :filled])
    print(f"alpha {alpha} at {sample_rate} Hz, {ir_len} bins: largest distance {int(d.max())} ulp")
    assert d.max() <= 1
    assert np.all(t[0, :filled].view(np.uint32) == np.float32(1.0).view(np.uint32))  # row 0 is exactly 1
    for b in range(filled):
        a = alpha[0] if n == 1 else alpha[b]
        if a == 0.0:
            assert np.all(t[:, b].view(np.uint32) == np.float32(1.0).view(np.uint32)), b
        assert np.all(np.diff(t[:, b]) <= 0), b  # never grows with the bin
        assert np.all(t[:, b] <= 1.0) and np.all(t[:, b] >= 0.0)
    if n == 1:
        assert all(np.array_equal(t[:, b].view(np.uint32), t[:, 0].view(np.uint32)) for b in range(width))
    else:
        assert not t[:, n:].view(np.uint32).any()  # the padding is +0


def test_table_default_width():
    assert air_attenuation([0.1], 16000, 10).shape == (10, 4)
    assert air_attenuation([0.1] * 4, 16000, 10).shape == (10, 4)
    assert air_attenuation([0.1] * 5, 16000, 10).shape == (10, 8)


def test_table_decays_by_its_coefficient():
    """Plain sanity: 0.1 dB/m over 343 m (one second of path) is 34.3 dB."""
    t = air_attenuation([0.1], 1000, 1001)
    assert abs(-10.0 * np.log10(np.float64(t[1000, 0])) - 34.3) < 1e-4


BAD_TABLE = [((0.1, 0.2, 0.3, 0.4, 0.5), 16000, 10, 4, "fit"), ((0.1,), 16000, 10, 5, "width"), ((0.1,), 16000, 10, 0, "width"),
             ((0.1,), 16000, 10, 16, "width"), ((0.1, np.nan), 16000, 10, 4, "band 1"), ((-0.1, 0.2), 16000, 10, 4, "band 0"),
             ((0.1, 0.2, np.inf), 16000, 10, 4, "band 2"), ((0.1,), 0, 10, 4, "sample rate"), ((0.1,), -16000, 10, 4, "sample rate"),
             ((0.1,), 16000, 0, 4, "ir_len"), ((0.1,), 16000, -3, 4, "ir_len"), ((0.1,) * 9, 16000, 10, 8, "1..8")]


@pytest.mark.parametrize("alpha,sample_rate,ir_len,width,word", BAD_TABLE)
def test_table_rejects(alpha, sample_rate, ir_len, width, word):
    with pytest.raises(ArxError) as e:
        air_attenuation(alpha, sample_rate, ir_len, width)
    assert e.value.status == INVALID and word in str(e.value), str(e.value)


def test_table_null_pointers():
    dp = C.POINTER(C.c_double)
    a = np.array([0.1])
    out = np.zeros((4, 4), np.float32)
    fn = lib().arx_air_attenuation_host
    assert fn(None, 1, 16000, 4, 4, out.ctypes.data_as(C.POINTER(C.c_float))) == INVALID
    assert fn(a.ctypes.data_as(dp), 1, 16000, 4, 4, None) == INVALID
    assert fn(a.ctypes.data_as(dp), 0, 16000, 4, 4, out.ctypes.data_as(C.POINTER(C.c_float))) == INVALID


# ------------------------------------------------------------------ the size ---
def test_air_bytes():
    f = lib().arx_debug_air_bytes
    for ir_len in (0, 1, 2500, 32000, 96000):
        for n in range(1, 9):
            assert f(ir_len, n) == ir_len * (4 if n <= 4 else 8) * 4, (ir_len, n)
    assert f(96000, 8) == 3072000
    for n in (0, -1, 9, 100):
        assert f(32000, n) == 0
    assert f(-1, 3) == 0


def test_no_renderer_means_no_coefficients():
    assert lib().arx_air_absorption_bands(None) == 0
    assert lib().arx_debug_air_tables_made(None) == 0
    a = np.array([0.1])
    assert lib().arx_set_air_absorption(None, a.ctypes.data_as(C.POINTER(C.c_double)), 1) == INVALID
