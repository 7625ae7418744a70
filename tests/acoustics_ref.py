"""Reference for the room-acoustic parameters (include/arx.h, arx_acoustics), shared by
test_acoustics_host.py and test_gpu_acoustics.py: the definitions restated in Python.

Python ints give the decay curve E, the bins, the windows and Ts's numerator -- exact at any size --
and numpy f64 does the three fits with the same centred formula.  The level tests use the same four
decimal literals as the header.  Inputs and references are made once per process and never changed.
"""
import functools
import math

import numpy as np

C5, C10, C25, C35 = 3.1622776601683794e-01, 1.0000000000000001e-01, 3.1622776601683794e-03, 3.1622776601683794e-04
VALID = ("edt", "t20", "t30", "c50", "c80", "d50", "ts")
FLOATS = ("edt_s", "t20_s", "t30_s", "c50_db", "c80_db", "d50", "ts_s")
INTS = ("total", "onset_bin", "last_bin", "edt_bins", "t20_bins", "t30_bins", "valid_mask")
# Every float within 1e-9 relative: the centred f64 fit differs from a long-double fit by at most
# 3e-16 on the decaying inputs below, and a worst-case summation bound over 5e4 terms is about 5e-12,
# so 1e-9 keeps two orders of margin and still catches an uncentred or f32 formulation.
RTOL = 1e-9

# (sample rate, seconds, RT of the left ear): a prime length below one workgroup's span of bins, a
# length no power of two divides, and 48 kHz x 2 s
SHAPES = [(1000, 1, 0.3), (1021, 2, 0.8), (48000, 2, 0.9)]


def edc_ints(h):
    """E[0..n] as Python ints, E[n] = 0."""
    e = [0] * (len(h) + 1)
    for k in range(len(h) - 1, -1, -1):
        e[k] = e[k + 1] + int(h[k])
    return e


def channel_reference(h, sr):
    """One channel's parameters (the dict of AudioRenderer.acoustics) and its E[0..n)."""
    h = [int(v) for v in h]
    n = len(h)
    E = edc_ints(h)
    nan = float("nan")
    out = {"total": E[0], "edt_s": nan, "t20_s": nan, "t30_s": nan, "c50_db": nan, "c80_db": nan, "d50": nan, "ts_s": nan,
           "onset_bin": -1, "last_bin": -1, "edt_bins": (-1, -1), "t20_bins": (-1, -1), "t30_bins": (-1, -1)}
    valid = set()
    total = E[0]
    if total > 0:
        nz = [k for k in range(n) if h[k] > 0]
        onset, last = nz[0], nz[-1]
        out["onset_bin"], out["last_bin"] = onset, last
        Ef = np.array([float(v) for v in E[:n]], np.float64)  # (double)E[k], correctly rounded
        pos = np.array([v > 0 for v in E[:n]])
        k_all = np.arange(n)

        def first_below(c):
            ks = k_all[(Ef <= Ef[0] * c) & (k_all >= onset)]
            return int(ks[0]) if ks.size else None

        def last_above(c):
            ks = k_all[(Ef >= Ef[0] * c) & pos]
            return int(ks[-1]) if ks.size else None

        a5 = first_below(C5)
        ranges = {"edt": (onset, last_above(C10)), "t20": (a5, last_above(C25)), "t30": (a5, last_above(C35))}
        for name, (a, b) in ranges.items():
            if a is None or b is None:
                continue
            out[name + "_bins"] = (a, b)
            if b - a < 1:
                continue
            x = np.arange(a, b + 1, dtype=np.float64) - (a + b) / 2
            y = 10.0 * np.log10(Ef[a:b + 1] / Ef[0])
            slope = float((x * y).sum() / (x * x).sum())
            if slope < 0:
                out[name + "_s"] = -60.0 / (slope * sr)
                valid.add(name)
        for ms, cname in ((50, "c50"), (80, "c80")):
            nw = (ms * sr + 500) // 1000
            if nw <= 0:
                continue
            late = E[min(onset + nw, n)]
            early = E[onset] - late
            if cname == "c50":
                out["d50"] = early / total
                valid.add("d50")
            if early > 0:
                out[cname + "_db"] = math.inf if late == 0 else 10.0 * math.log10(early / late)
                valid.add(cname)
        num = sum((k - onset) * h[k] for k in range(onset + 1, n))  # passes 64 bits: a Python int
        out["ts_s"] = num / (total * sr)
        valid.add("ts")
    out["valid"] = valid
    out["valid_mask"] = sum(1 << VALID.index(v) for v in valid)
    return out, np.array(E[:n], np.int64)


def reference(left, right, sr):
    """{"left" | "right" | "sum": (parameters, E)}."""
    L = [int(v) for v in left]
    R = [int(v) for v in right]
    return {"left": channel_reference(L, sr), "right": channel_reference(R, sr),
            "sum": channel_reference([a + b for a, b in zip(L, R)], sr)}


def decaying(sr, seconds, rt, seed):
    """Seeded Poisson draws of A exp(-13.8155 k / (RT sr)) behind 2 % leading zero bins, the right
    ear with another RT."""
    n = sr * seconds
    lead = n // 50
    rng = np.random.default_rng(seed)
    k = np.arange(n - lead, dtype=np.float64)
    ears = []
    for ear_rt, amp in ((rt, 1.0e6), (1.25 * rt, 0.7e6)):
        h = np.zeros(n, np.int64)
        h[lead:] = rng.poisson(amp * np.exp(-13.8155 * k / (ear_rt * sr)))
        ears.append(h)
    return ears[0], ears[1]


def edge_inputs():
    """name -> (left, right, sample rate)."""
    z = lambda n: np.zeros(n, np.int64)  # noqa: E731
    out = {}
    out["all_zero"] = (z(1000), z(1000), 1000)
    a, b = z(1000), z(1000)
    a[0], b[0] = 12345, 7
    out["first_bin_only"] = (a, b, 1000)  # C50 = +inf, no time valid
    a, b = z(1000), z(1000)
    a[-1], b[-1] = 5, 9
    out["last_bin_only"] = (a, b, 1000)
    a, b = z(8), z(8)
    a[:] = [0, 900, 300, 100, 30, 10, 3, 1]
    b[:] = [0, 0, 500, 200, 50, 20, 5, 2]
    out["sr8"] = (a, b, 8)  # n50 = 0: the 50 ms window is empty
    # two equal bins of the decay curve behind the onset: E = 4v, v, v, 0, ...; T20's and T30's range is
    # [1, 2], flat, so the slope is exactly zero (x = -1/2, +1/2) -- not below zero, the time invalid
    a, b = z(1000), z(1000)
    a[0], a[2] = 3 << 20, 1 << 20
    b[0], b[2] = 3 << 10, 1 << 10
    out["flat_pair"] = (a, b, 1000)
    # sum(L + R) = 2^62 over the last quarter of the bins: Ts's numerator needs more than 64 bits
    a, b = z(4096), z(4096)
    a[3072:] = 1 << 51
    b[3072:] = 1 << 51
    out["two_to_62"] = (a, b, 1024)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(left, right, sample rate, reference) of a named input: "decay<i>" for SHAPES[i], "decay_44k"
    (44.1 kHz x 3 s), or an edge input's name.  Made once; do not modify."""
    if name.startswith("decay"):
        sr, sec, rt = (44100, 3, 1.1) if name == "decay_44k" else SHAPES[int(name[5:])]
        L, R = decaying(sr, sec, rt, seed=20240 + sr)
    else:
        L, R, sr = edge_inputs()[name]
    for arr in (L, R):
        arr.setflags(write=False)
    return L, R, sr, reference(L, R, sr)


EDGE_NAMES = ("all_zero", "first_bin_only", "last_bin_only", "sr8", "flat_pair", "two_to_62")


def assert_matches(got, want, what=""):
    """got: a dict of AudioRenderer.acoustics / acoustics_from_histogram; want: channel_reference's.
    Integers and the valid mask exactly, floats within RTOL with the same NaN / inf pattern."""
    for k in INTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert got["valid"] == want["valid"], (what, got["valid"], want["valid"])
    for k in FLOATS:
        g, w = got[k], want[k]
        print(f"{what} {k}: got {g!r} reference {w!r}")
        if math.isnan(w) or math.isinf(w):
            assert (math.isnan(g) and math.isnan(w)) or g == w, (what, k, g, w)
        else:
            assert math.isfinite(g) and abs(g - w) <= RTOL * abs(w), (what, k, g, w)
