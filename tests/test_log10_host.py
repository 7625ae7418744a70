"""Host: the log10 the room-acoustic analysis takes for its levels on the device and on the host alike
(arx_acoustics.hip's log10_shared, through arx_debug_log10_shared; plain C++, no device).

The bound is worked out from the formats, not from the function: the logarithm's form (f - f^2/2 + s (f^2/2 + R))
is within 1 ulp, the product by the rounded 1 / ln(10) adds its own half ulp and half an ulp for the constant,
so the function is within 2 ulp of log10; numpy's log10 is within 1 ulp; two such values differ by at most 3 ulp.
The arguments are what the analysis forms: ratios of two positive int64, so from 2^-63 to 2^63.
"""
import ctypes as C

import numpy as np

from audiorenderingv2_amd._lib import lib

ULP = 2.0 ** -52
DP = C.POINTER(C.c_double)


def log10_shared(x):
    x = np.ascontiguousarray(x, np.float64)
    out = np.zeros_like(x)
    assert lib().arx_debug_log10_shared(x.ctypes.data_as(DP), x.size, out.ctypes.data_as(DP)) == 0
    return out


def test_against_numpy_over_the_argument_range():
    rng = np.random.Generator(np.random.PCG64(3))
    num = rng.integers(1, 2 ** 62, 100000).astype(np.float64)
    den = rng.integers(1, 2 ** 62, 100000).astype(np.float64)
    x = np.concatenate([rng.uniform(0.0, 1.0, 200000) + 2.0 ** -63,  # E / total, the fits' arguments
                        2.0 ** rng.uniform(-63.0, 63.0, 200000),        # every binade of the range
                        num / den, np.nextafter(1.0, 0.0) ** np.arange(1, 2001),  # just below 1, where the result is small
                        [2.0 ** -63, 2.0 ** 63, 0.5, 2.0, 10.0, 0.1, 1e-3, np.sqrt(0.5), np.sqrt(2.0), 1.4142135623730951]])
    got, want = log10_shared(x), np.log10(x)
    err = np.abs(got - want) / np.abs(want)
    print(f"{x.size} arguments: largest distance from numpy's log10 {np.nanmax(err) / ULP:.2f} ulp")
    assert np.all(np.isfinite(got)) and np.nanmax(err) <= 3 * ULP


def test_exact_values_and_the_library_route():
    assert log10_shared([1.0])[0] == 0.0
    got = log10_shared([0.0, -1.0, np.inf, np.nan, 5e-324])
    assert got[0] == -np.inf and np.isnan(got[1]) and got[2] == np.inf and np.isnan(got[3])
    assert abs(got[4] - np.log10(5e-324)) <= 3 * ULP * abs(np.log10(5e-324))
    assert np.all(np.diff(log10_shared(np.linspace(0.01, 1.0, 5001))) > 0)  # rises over the fits' range, 2e-4 apart
    assert lib().arx_debug_log10_shared(None, 1, None) == 1 and lib().arx_debug_log10_shared(None, 0, None) == 0
