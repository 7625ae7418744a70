"""GPU: the power-of-two "linear + fold" convolution in every kernel family it has, file and live.

conv_plan_create takes the direct mixed-radix path when ir_len = N1 x N2 with both factors 7-smooth
and <= 512, and the power-of-two path for everything else: any ir_len with a prime factor above 7,
and every ir_len above 2^18 (48 kHz x 6 s, 96 kHz x 3 s: ordinary long-reverb settings).  The usual
rates at 1-2 s are all direct plans, so the suite's other convolution tests reach the power-of-two
path at one shape only (sr = 1100: M = 4096 = 64 x 64).  The cases here pick one (sr, secs) per
kernel family that launch_pass_b / pass_a / pass_c choose between:

  lg(M)  N1 x N2      tc  kernels
  15     128 x 256    16  generic lds_fft with a radix-2 stage; pass_bw<., 256> (fft256_wave)
  16     256 x 256    16  columns_wave<256>; pass_bw<., 256>
  17     256 x 512    16  columns_wave<256>; pass_bw<., 512> (fft512_wave, dft8, mul_w8, mul_w83)
  18     512 x 512     8  columns_wave<512>; pass_bw<., 512>
  19     512 x 1024    8  columns_wave<512>; generic pass_b, 4 rows per thread
  20     1024 x 1024   4  generic columns, 64 threads per column
  23     2048 x 4096   2  pass_b at its kMaxPer = 16 limit; 96 KB / 128 KB of dynamic LDS

Every case first pins its plan (conv_plan), so a later change to direct_split cannot silently move
it onto the other path.  The bars are the project's own: 1 ULP of the output's maximum against the
f64 oracle for a file (test_gpu_parity.py), 1e-12 of the maximum for a live block (test_gpu_live.py)
-- and, for a single-tap IR on both paths, a per-sample bound that an error of a few of a quiet
sample's own ULPs, or a sample misplaced at a block seam, cannot pass.
"""
import numpy as np
import pytest

import pyoracle as po
from audiorenderingv2_amd import AudioRenderer, RenderSettings

pytestmark = pytest.mark.gpu


def ulp_of_max(y):
    return np.spacing(np.float32(np.abs(y).max()))


def conv_renderer(sr, secs=2):
    return AudioRenderer(RenderSettings(rays=(1, 1, 1), sample_rate=sr, ir_length_in_seconds=secs))


def sparse_ir(n, rng, k=300, scale=1e-4):
    ir = np.zeros(n, np.float32)
    ir[rng.integers(0, n, k)] = rng.exponential(scale, k).astype(np.float32)
    return ir


def rel_err(got, ref):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)


def pow2_plan(n, sr, lg, n1, n2):
    return f"pow2 linear+fold: n={n} sr={sr} M={1 << lg} ({n1}x{n2})"


def convolute_audio_np(x, sr, ir):
    """orc_convolute_audio (oracle/arx_oracle.c) restated with numpy.fft in f64: one-second blocks
    zero padded to n = ir.size, circularly convolved with the IR (unnormalised inverse: n x the
    convolution), overlap-added at hops of sr and clipped to len(x), divided by n // 2, rounded once
    to f32.  The tail len(x) mod sr is never read."""
    n, length = ir.size, x.size
    H = np.fft.fft(ir.astype(np.float64))
    acc = np.zeros(length)
    for s in range(length // sr):
        blk = np.zeros(n)
        m = min(sr, n)
        blk[:m] = x[s * sr:s * sr + m]
        y = np.fft.ifft(np.fft.fft(blk) * H).real * n
        copy = n if s * sr + n < length else length - s * sr
        acc[s * sr:s * sr + copy] += y[:copy]
    return (acc / (n // 2)).astype(np.float32)


def file_case(sr, secs, length):
    """Inputs of test_gpu_parity.test_convolution_matches_oracle."""
    rng = np.random.default_rng(sr + length)
    n = sr * secs
    irl, irr = sparse_ir(n, rng), sparse_ir(n, rng)
    x = (0.3 * rng.standard_normal(length)).astype(np.float32)
    return irl, irr, x


# ---- 1. file convolution against the f64 oracle, one case per kernel family ----------------------
# (sr, secs, length) -> lg(M), N1, N2.  Three blocks (an odd count: the last pair has no second
# block) and a ragged tail the reference drops; (6500, 2, 30000) is four blocks, so lg 15 also runs
# at 20000 frames for its lone last block.
FILE_CASES = [
    (6500, 2, 30000, 15, 128, 256),
    (6500, 2, 20000, 15, 128, 256),
    (17000, 2, 60000, 16, 256, 256),
    (34000, 2, 110000, 17, 256, 512),
    (44000, 2, 140000, 18, 512, 512),
    (48000, 6, 150000, 19, 512, 1024),
    (48000, 10, 150000, 20, 1024, 1024),
]


@pytest.mark.parametrize("sr,secs,length,lg,n1,n2", FILE_CASES)
def test_file_convolution_matches_oracle(sr, secs, length, lg, n1, n2):
    irl, irr, x = file_case(sr, secs, length)
    r = conv_renderer(sr, secs)
    try:
        assert r.conv_plan(live=False).startswith(pow2_plan(sr * secs, sr, lg, n1, n2))
        r.set_ir(irl, irr)
        L, R, _, _ = r.convoluteAudioFile(x)
    finally:
        r.close()
    for ear, got, ir in (("L", L, irl), ("R", R, irr)):
        ref = po.convolute_audio(x, sr, ir)
        assert ref.any()
        err, tol = np.abs(got - ref).max(), ulp_of_max(ref)
        print(f"lg {lg} {ear}: max err {err:.3e}, 1 ulp of max {tol:.3e}")
        assert err <= tol


# ---- 2. the largest rows ----------------------------------------------------------------------
def test_numpy_restatement_equals_oracle():
    """convolute_audio_np against po.convolute_audio at small shapes (one per path of the plan
    choice; the reference itself has one path).  Both are f64 computations good to ~1e-15 of the
    output's maximum, rounded once to f32: they can differ by the f64 error, plus one spacing of a
    sample whose rounding that error flips."""
    for sr, secs, length in ((1100, 2, 6000), (1125, 2, 4000), (1000, 1, 3300)):
        irl, _, x = file_case(sr, secs, length)
        a, b = convolute_audio_np(x, sr, irl), po.convolute_audio(x, sr, irl)
        assert b.any()
        tol = np.spacing(np.abs(b)).astype(np.float64) + 1e-14 * np.abs(b).max()
        assert np.all(np.abs(a.astype(np.float64) - b) <= tol), (sr, secs, length)


def test_file_convolution_largest_rows():
    """M = 2^23 = 2048 x 4096, tc = 2, one block: pass_b keeps kMaxPer = 16 spectrum values per
    thread and asks for 128 KB of dynamic LDS, passes A / C for 96 KB; about 1 GB of device memory.
    The reference is the numpy restatement above (the recursive oracle needs seconds per transform
    at this length)."""
    sr, secs = 2_100_000, 1
    length = sr + 1000
    irl, irr, x = file_case(sr, secs, length)
    r = conv_renderer(sr, secs)
    try:
        assert r.conv_plan(live=False).startswith(pow2_plan(sr, sr, 23, 2048, 4096))
        r.set_ir(irl, irr)
        L, R, _, _ = r.convoluteAudioFile(x)
    finally:
        r.close()
    for ear, got, ir in (("L", L, irl), ("R", R, irr)):
        ref = convolute_audio_np(x, sr, ir)
        assert ref.any()
        err, tol = np.abs(got - ref).max(), ulp_of_max(ref)
        print(f"lg 23 {ear}: max err {err:.3e}, 1 ulp of max {tol:.3e}")
        assert err <= tol


# ---- 3. live block, power-of-two plans --------------------------------------------------------
# pass_a<2>, pass B, pass_c into Y, pass_d_live with its i + n < ylen fold.  (sr, secs) -> lg, N1, N2
# of the live plan (hop 4096).
LIVE_CASES = [(17000, 2, 16, 256, 256), (34000, 2, 17, 256, 512), (48000, 6, 19, 512, 1024)]


def live_ir(n, rng):
    """The IR of test_gpu_live.live_renderer, plus one tap in each ear's last two samples: whatever
    the block length, part of the block's linear convolution then lies past n and comes back
    through pass_d_live's fold term."""
    irs = []
    for ch in range(2):
        ir = np.zeros(n, np.float32)
        ir[rng.integers(0, n, 500)] = rng.exponential(1e-3, 500).astype(np.float32)
        ir[n - 1 - ch] = np.float32(1e-3)
        irs.append(ir)
    return irs


def live_renderer(sr, secs, lg, n1, n2):
    n = sr * secs
    r = conv_renderer(sr, secs)
    irl, irr = live_ir(n, np.random.default_rng(sr))
    r.set_ir(irl, irr)
    assert r.conv_plan(live=True).startswith(pow2_plan(n, 4096, lg, n1, n2))
    return r, irl, irr


@pytest.mark.parametrize("n_in", [4096, 1000, 0])
@pytest.mark.parametrize("sr,secs,lg,n1,n2", LIVE_CASES)
def test_live_block_matches_oracle(sr, secs, lg, n1, n2, n_in):
    r, irl, irr = live_renderer(sr, secs, lg, n1, n2)
    try:
        x = np.random.default_rng(sr + n_in).uniform(-1, 1, n_in)
        got = r.convoluteLiveInput(x)
    finally:
        r.close()
    if n_in == 0:
        assert not got.any()
        return
    err = rel_err(got, po.convolute_live_block(x, irl, irr))
    print(f"live lg {lg} n_in {n_in}: rel err {err:.3e}")
    assert err < 1e-12


@pytest.mark.parametrize("sr,secs,lg,n1,n2", LIVE_CASES)
def test_live_block_larger_hop_and_new_ir(sr, secs, lg, n1, n2):
    """A block longer than the plan's hop re-makes the plan with that hop; after set_ir the next
    block follows the new IR."""
    n = sr * secs
    r, irl, irr = live_renderer(sr, secs, lg, n1, n2)
    try:
        rng = np.random.default_rng(sr + 5000)
        x = rng.uniform(-1, 1, 5000)
        got = r.convoluteLiveInput(x)
        assert r.conv_plan(live=True).startswith(pow2_plan(n, 5000, lg, n1, n2))
        irl2, irr2 = irr * np.float32(0.5), irl * np.float32(2.0)
        r.set_ir(irl2, irr2)
        x2 = rng.uniform(-1, 1, 4096)
        got2 = r.convoluteLiveInput(x2)
    finally:
        r.close()
    err = rel_err(got, po.convolute_live_block(x, irl, irr))
    err2 = rel_err(got2, po.convolute_live_block(x2, irl2, irr2))
    print(f"live lg {lg}: block of 5000 rel err {err:.3e}, new IR rel err {err2:.3e}")
    assert err < 1e-12
    assert err2 < 1e-12


# ---- 4. delay identity, per-sample tolerance, both paths ---------------------------------------
# One tap g at delay k <= n - sr (the last delay without circular wrap) per ear.  The reference's
# scale n / (n / 2) is exactly 2 for even n and 2 g a power of two, so the expected output is exact:
# out[j] = 2 g x[j - k] for 0 <= j - k < (length // sr) sr, and 0 everywhere else -- no oracle needed.
# Per sample: |got - expected| <= half a spacing of the expected f32 value (the final rounding) +
# 1e-12 max|x| (the project's bound for the f64 convolution, test_gpu_live.py).
DELAY_CASES = [
    # power-of-two plans
    (1100, 2, 6000, "pow2 linear+fold: n=2200 sr=1100 M=4096 (64x64)"),
    (17000, 2, 60000, pow2_plan(34000, 17000, 16, 256, 256)),
    (44000, 2, 140000, pow2_plan(88000, 44000, 18, 512, 512)),
    (48000, 6, 300000, pow2_plan(288000, 48000, 19, 512, 1024)),
    # direct plans
    (16000, 2, 5 * 16000 + 777, "mixed-radix direct circular: n=32000 sr=16000 (160x200)"),  # compile-time, chained C
    (441, 2, 5000, "mixed-radix direct circular: n=882 sr=441 "),                           # odd N1: pass_c_mr + pass_d
    (48000, 1, 100000, "mixed-radix direct circular: n=48000 sr=48000 "),                    # n = sr
    (77175, 2, 200000, "mixed-radix direct circular: n=154350 sr=77175 "),                   # radix 7, 512-wide kernels
]


def delayed(x, k, gain, sr):
    out = np.zeros(x.size, np.float32)
    m = min((x.size // sr) * sr, x.size - k)  # j - k < S sr and j < len
    out[k:k + m] = np.float32(2.0 * gain) * x[:m]
    return out


@pytest.mark.parametrize("sr,secs,length,plan", DELAY_CASES)
def test_single_tap_is_an_exact_delay(sr, secs, length, plan):
    n = sr * secs
    assert n % 2 == 0
    rng = np.random.default_rng(sr + length)
    x = (0.3 * rng.standard_normal(length)).astype(np.float32)
    last = n - sr
    if last >= 2:
        mid = int(rng.integers(1, last))  # strictly between 0 and n - sr
        ears = [((0, 0.5), (last, 0.5)), ((mid, 0.5), (0, 0.5)), ((last, 0.5), (mid, 0.5))]
    else:  # n = sr: delay 0 alone is free of wrap; the ears differ in gain, so that a swap still shows
        ears = [((0, 0.5), (0, 0.25)), ((0, 0.25), (0, 0.5))]
    slack = 1e-12 * float(np.abs(x).max())
    r = conv_renderer(sr, secs)
    try:
        assert r.conv_plan(live=False).startswith(plan)
        for (kl, gl), (kr, gr) in ears:
            irl, irr = np.zeros(n, np.float32), np.zeros(n, np.float32)
            irl[kl], irr[kr] = gl, gr
            r.set_ir(irl, irr)
            L, R, _, _ = r.convoluteAudioFile(x)
            for ear, got, k, g in (("L", L, kl, gl), ("R", R, kr, gr)):
                want = delayed(x, k, g, sr)
                err = np.abs(got.astype(np.float64) - want)
                tol = 0.5 * np.spacing(np.abs(want)).astype(np.float64) + slack
                bad = np.flatnonzero(err > tol)
                print(f"{ear} k={k} gain={g}: worst err {err.max():.3e} = {err.max() / np.abs(x).max():.3e} max|x|, "
                      f"{bad.size} samples over the bound")
                assert bad.size == 0, (ear, k, g, bad[:8], got[bad[:8]], want[bad[:8]])
    finally:
        r.close()
