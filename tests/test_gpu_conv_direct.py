"""GPU: the mixed-radix direct convolution in every kernel family mr_dispatch has and on every call
route, file and live.

conv_plan_create takes the direct path whenever ir_len = N1 x N2 with 7-smooth factors <= 512 --
every usual rate at 1-3 s.  mr_dispatch (arx_conv.hip) then picks the kernels' template arguments:
a compile-time plan (300 x 320, 160 x 200, 315 x 280, 250 x 256) or a run-time plan Mr<R7, LM, 0, 0>,
R7 in {false, true} x LM in {320, 512}; chain_plan picks pass_c_chain / pass_c_chain3 (n = 2 sr, N1
even) or pass_c_mr + pass_d; and the call route picks pass B:

  route                                      kernels
  1  a new IR and a file in one call          pass_a_mr<0> (pairs + the IR batch), pass_b_pair
  2  the same IR again                        pass_a_mr<0>, pass_b_mr<0> (four rows per workgroup)
  3  the IR spectra made alone first          pass_a_mr<0> (IR batch alone), pass_b_pair<HONLY>; then 2
  4  a prepared input                         pass_b_mr<3>; pass_b_pair<XS> (new IR), pass_b_mr<4> (same IR)
  5  a time-block shard                       pass_c_chain with emit_from = 1 and / or tail = 0
  6  the live block                           pass_a_mr<2>, pass_b_mr<0> (one row), pass_c_mr (two columns)
  7  a single tap, per-sample bound           route 1's kernels

The rest of the suite runs these routes on the compile-time plans of 48 / 16 / 44.1 kHz; the cases
here (CASES, tests/test_conv_direct_host.py, which checks on the CPU that each takes the plan named
there) put every run-time family, chained and windowed, and 250 x 256 through them, at the shape
edges the template code branches on: single-stage sub-FFTs, N1 = 2, odd N1, sub-length 512, ragged
last tiles with xcd_tile's remapped numbering, all four odd radices together (22.05 kHz x 2 s).

Bars, all the project's own: 1 ULP of the output's maximum against the f64 oracle (route 1, as
test_gpu_parity.py); bit-identity with route 1 (routes 2, 3, 5: DESIGN.md §6.5 "One route for the
IR spectra", §8e's shards) and with convolute_device (route 4); 1e-12 of the maximum against the
oracle for a live block (test_gpu_live.py); half a spacing of the exact f32 + 1e-12 max|x| per
sample for a single tap (test_gpu_conv_pow2.py).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pyoracle as po
from audiorenderingv2_amd import AudioRenderer, DeviceBuffer, RenderGroup, RenderSettings
from audiorenderingv2_amd._lib import check, lib
from test_conv_direct_host import CASES, case_id

pytestmark = pytest.mark.gpu

BY_SR = {c.sr: c for c in CASES}
CHAINED = [c for c in CASES if c.chained]
LARGEST = 131072  # 512 x 512: three blocks, once


def settings(c):
    return RenderSettings(rays=(1, 1, 1), sample_rate=c.sr, ir_length_in_seconds=c.secs)


def plan_prefix(c, hop=None):
    return f"mixed-radix direct circular: n={c.sr * c.secs} sr={hop or c.sr} ({c.n1}x{c.n2})"


def pinned_renderer(c):
    """A renderer whose file plan is the table's.  (conv_plan makes the spectra of the IR set so far,
    so it is asked before set_ir: the next convolution still meets a new IR.)"""
    r = AudioRenderer(settings(c))
    plan = r.conv_plan(live=False)
    assert plan.startswith(plan_prefix(c)), plan
    return r


def sparse_ir(n, rng, k=300, scale=1e-4):
    ir = np.zeros(n, np.float32)
    ir[rng.integers(0, n, k)] = rng.exponential(scale, k).astype(np.float32)
    return ir


def ragged(c):
    return max(1, c.sr // 3)  # a tail shorter than a block, which the reference never reads


def run_lengths(c):
    """Five blocks and a ragged tail (the last pair a lone block: `odd` false, and the segment after
    the last pair) and four blocks (every pair whole)."""
    if c.sr == LARGEST:
        return [3 * c.sr + 777]
    return [5 * c.sr + ragged(c), 4 * c.sr]


def shard_lengths(c):
    """Four pairs, the last a lone block, and a tail; three whole pairs."""
    return [7 * c.sr + ragged(c), 6 * c.sr]


def inputs(c, length):
    rng = np.random.default_rng([c.sr, c.secs, length])
    n = c.sr * c.secs
    irl, irr = sparse_ir(n, rng), sparse_ir(n, rng)
    x = (0.3 * rng.standard_normal(length)).astype(np.float32)
    return irl, irr, x


def bits(a):
    return np.asarray(a).view(np.uint32)


def assert_same_bits(got, want, what):
    for ear, g, w in zip("LR", got, want):
        diff = np.flatnonzero(bits(g) != bits(w))
        assert diff.size == 0, (f"{what}, {ear}: {diff.size} of {g.size} samples differ, first at {diff[:4]}: "
                                f"{g[diff[:4]]} != {w[diff[:4]]}")


def frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def route1(sr, length):
    """The case's file convolved twice on one renderer: with the IR new (route 1) and again (route
    2).  Computed once per (case, length); every bit-identity bar of this file refers to `first`."""
    c = BY_SR[sr]
    irl, irr, x = inputs(c, length)
    r = pinned_renderer(c)
    try:
        r.set_ir(irl, irr)
        L1, R1, _, _ = r.convoluteAudioFile(x)
        L2, R2, _, _ = r.convoluteAudioFile(x)
    finally:
        r.close()
    frozen(irl, irr, x, L1, R1, L2, R2)
    return {"ir": (irl, irr), "x": x, "first": (L1, R1), "again": (L2, R2)}


# ---- 1. a new IR and the file in one call, against the f64 oracle --------------------------------
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_new_ir_and_file_match_oracle(c):
    for length in run_lengths(c):
        run = route1(c.sr, length)
        for ear, got, ir in zip("LR", run["first"], run["ir"]):
            ref = po.convolute_audio(run["x"], c.sr, ir)
            assert ref.any()
            err, tol = np.abs(got - ref).max(), np.spacing(np.float32(np.abs(ref).max()))
            print(f"{c.n1}x{c.n2} {c.family} len {length} {ear}: max err {err:.3e}, 1 ulp of max {tol:.3e}")
            assert err <= tol, (length, ear)


# ---- 2. the same IR again: the stored spectra, pass_b_mr<0> ---------------------------------------
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_same_ir_again_is_bit_identical(c):
    for length in run_lengths(c):
        run = route1(c.sr, length)
        assert_same_bits(run["again"], run["first"], f"len {length}, stored spectra")


# ---- 3. the spectra made alone first --------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_spectra_made_alone_give_the_same_bits(c):
    """DESIGN.md §6.5, "One route for the IR spectra": whether arx_prepare_ir_spectra or a file
    shorter than one block made them (pass_b_pair<HONLY>) or the convolution's own first pass did
    (route 1), the output is the same bits."""
    length = run_lengths(c)[0]
    run = route1(c.sr, length)
    short = np.random.default_rng(c.sr).standard_normal(max(1, c.sr // 3)).astype(np.float32)
    for how in ("prepare_ir_spectra", "short_file_first"):
        r = pinned_renderer(c)
        try:
            r.set_ir(*run["ir"])
            if how == "prepare_ir_spectra":
                r.prepare_ir_spectra(file=True, live=False)
            else:
                Ls, Rs, _, _ = r.convoluteAudioFile(short)  # no whole block: zero output, spectra made alone
                assert not Ls.any() and not Rs.any()
            L, R, _, _ = r.convoluteAudioFile(run["x"])
        finally:
            r.close()
        assert_same_bits((L, R), run["first"], how)


# ---- 4. a prepared input --------------------------------------------------------------------------
def fetch(r, a, b, n):
    r.stats()  # synchronises the renderer's stream (the device buffers are read on the null stream)
    return a.to_numpy(np.float32, n), b.to_numpy(np.float32, n)


WINDOWED_PREPARED = BY_SR[9604]  # no chained pass C: the kept copy of the input


@pytest.mark.parametrize("c", CHAINED + [WINDOWED_PREPARED], ids=case_id)
def test_prepared_input_equals_device_convolution(c):
    """test_gpu_conv_reuse.py's sequence: three IRs; convolute_device per IR is the reference; the
    input prepared once and then overwritten by the caller; each IR used twice, new (pass_b_pair<XS>)
    and unchanged (pass_b_mr<4>)."""
    n = c.sr * c.secs
    for length in run_lengths(c):
        rng = np.random.default_rng([c.sr, c.secs, length, 4])
        x = (0.3 * rng.standard_normal(length)).astype(np.float32)
        irs = [(sparse_ir(n, rng), sparse_ir(n, rng)) for _ in range(3)]
        r = pinned_renderer(c)
        dx = DeviceBuffer.from_numpy(0, x)
        bufs = [DeviceBuffer(0, x.nbytes) for _ in range(4)]
        try:
            want = []
            for irl, irr in irs:
                r.set_ir(irl, irr)
                r.convolute_device(dx.ptr, x.size, bufs[0].ptr, bufs[1].ptr)
                want.append(fetch(r, bufs[0], bufs[1], x.size))
            assert want[0][0].any() and not np.array_equal(want[0][0], want[1][0])
            r.convolute_prepare_input(dx.ptr, x.size)
            r.stats()
            z = np.zeros(x.size, np.float32)  # the caller may overwrite its input once it is prepared
            check(lib().arx_memcpy(0, C.c_void_p(dx.ptr), z.ctypes.data_as(C.c_void_p), z.nbytes))
            for k, (irl, irr) in enumerate(irs):
                r.set_ir(irl, irr)
                assert r.convolute_prepared(bufs[2].ptr, bufs[3].ptr) == x.size
                assert_same_bits(fetch(r, bufs[2], bufs[3], x.size), want[k], f"len {length}, IR {k} new")
                assert r.convolute_prepared(bufs[2].ptr, bufs[3].ptr) == x.size
                assert_same_bits(fetch(r, bufs[2], bufs[3], x.size), want[k], f"len {length}, IR {k} unchanged")
        finally:
            for b in [dx, *bufs]:
                b.close()
            r.close()


# ---- 5. time-block shards -------------------------------------------------------------------------
def sharded(g, x):
    """Run the group's sharded convolution into NaN-filled outputs; per rank: (begin, end, L, R) of
    its full-length outputs (as test_gpu_group_conv.sharded)."""
    bufs = []
    for m in g.members:
        d = m.settings.device
        out_l, out_r = DeviceBuffer(d, 4 * x.size), DeviceBuffer(d, 4 * x.size)
        nan = np.full(x.size, np.nan, np.float32)
        for b in (out_l, out_r):  # frames a rank does not own must stay untouched
            check(lib().arx_memcpy(d, C.c_void_p(b.ptr), nan.ctypes.data_as(C.c_void_p), nan.nbytes))
        bufs.append((DeviceBuffer.from_numpy(d, x), out_l, out_r))
    try:
        g.convolute_device([b[0].ptr for b in bufs], x.size, [b[1].ptr for b in bufs], [b[2].ptr for b in bufs])
        g.synchronize()
        res = []
        for i, (_, ol, orr) in enumerate(bufs):
            b, e = g.conv_shard(x.size, i)
            res.append((b, e, ol.to_numpy(np.float32, x.size), orr.to_numpy(np.float32, x.size)))
    finally:
        for trio in bufs:
            for buf in trio:
                buf.close()
    return res


def assemble_and_check(res, ref, x_size, whole_file):
    """test_gpu_group_conv.assemble_and_check: the ranks' ranges tile [0, len) in rank order, a rank
    writes exactly its frames (or, on a plan that does not shard, the whole file), and the union is
    the one-renderer convolution bit for bit."""
    L, R = np.full(x_size, np.nan, np.float32), np.full(x_size, np.nan, np.float32)
    cursor = 0
    for b, e, ol, orr in res:
        assert b == cursor or (b == e), (b, e, cursor)
        cursor = max(cursor, e)
        L[b:e], R[b:e] = ol[b:e], orr[b:e]
        if whole_file:
            assert np.array_equal(bits(ol), bits(ref[0])) and np.array_equal(bits(orr), bits(ref[1]))
        else:
            outside = np.ones(x_size, bool)
            outside[b:e] = False
            assert np.isnan(ol[outside]).all() and np.isnan(orr[outside]).all(), (b, e)
    assert cursor == x_size
    assert_same_bits((L, R), ref, "union of the shards")


def pinned_group(c, k):
    g = RenderGroup(settings(c), devices=[0] * k)
    for m in g.members:
        plan = m.conv_plan(live=False)
        assert plan.startswith(plan_prefix(c)), plan
    return g


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("c", [c for c in CHAINED if c.sr != LARGEST], ids=case_id)
def test_shards_tile_the_file_bit_identically(c, k):
    """k ranks on one device: shards of two pairs and of one behind a seam pair (emit_from = 1), with
    and without the file's last segment (tail), and ranks that own no pair (k = 5).  Each file runs
    with the IR new on every member (the seam pair's pass_b_pair stores H) and again with the stored
    spectra."""
    g = pinned_group(c, k)
    try:
        assert g.conv_sharded
        for length in shard_lengths(c):
            run = route1(c.sr, length)
            x = run["x"]
            owned = [g.conv_shard(x.size, i) for i in range(k)]
            assert sum(e - b for b, e in owned) == x.size
            assert (k == 5) == any(b == e for b, e in owned)
            for i in range(k):
                g.member(i).set_ir(*run["ir"])
            assemble_and_check(sharded(g, x), run["first"], x.size, whole_file=False)
            assemble_and_check(sharded(g, x), run["first"], x.size, whole_file=False)
    finally:
        g.close()


def test_windowed_plan_convolves_the_whole_file_on_every_rank():
    c = BY_SR[441]  # 21 x 42: N1 odd, no chained pass C
    g = pinned_group(c, 3)
    try:
        assert not g.conv_sharded
        for length in shard_lengths(c):
            run = route1(c.sr, length)
            for i in range(3):
                g.member(i).set_ir(*run["ir"])
            assemble_and_check(sharded(g, run["x"]), run["first"], run["x"].size, whole_file=True)
    finally:
        g.close()


# ---- 6. the live block ----------------------------------------------------------------------------
def rel_err(got, ref):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)


def live_ir(n, rng):
    """The IR of test_gpu_conv_pow2.live_ir: 500 taps and one in each ear's last two samples, so
    that part of the block's convolution wraps round the circular length."""
    irs = []
    for ch in range(2):
        ir = np.zeros(n, np.float32)
        ir[rng.integers(0, n, 500)] = rng.exponential(1e-3, 500).astype(np.float32)
        ir[n - 1 - ch] = np.float32(1e-3)
        irs.append(ir)
    return irs


@pytest.mark.parametrize("c", [c for c in CASES if c.live], ids=case_id)
def test_live_block_matches_oracle(c):
    """convoluteLiveInput with a full hop, a partial block and no input; after set_ir the next block
    follows the new IR."""
    n = c.sr * c.secs
    hop = min(n, 4096)
    rng = np.random.default_rng([c.sr, c.secs, 6])
    irl, irr = live_ir(n, rng)
    r = AudioRenderer(settings(c))
    try:
        r.set_ir(irl, irr)
        plan = r.conv_plan(live=True)
        assert plan.startswith(plan_prefix(c, hop)), plan
        for n_in in (hop, hop // 3 + 1, 0):
            x = rng.uniform(-1, 1, n_in)
            got = r.convoluteLiveInput(x)
            if n_in == 0:
                assert not got.any()
                continue
            err = rel_err(got, po.convolute_live_block(x, irl, irr))
            print(f"live {c.n1}x{c.n2} {c.family} n_in {n_in}: rel err {err:.3e}")
            assert err < 1e-12, n_in
        irl2, irr2 = irr * np.float32(0.5), irl * np.float32(2.0)
        r.set_ir(irl2, irr2)
        x = rng.uniform(-1, 1, hop)
        err = rel_err(r.convoluteLiveInput(x), po.convolute_live_block(x, irl2, irr2))
        print(f"live {c.n1}x{c.n2} {c.family} new IR: rel err {err:.3e}")
        assert err < 1e-12
        assert r.conv_plan(live=True).startswith(plan_prefix(c, hop))
    finally:
        r.close()


# ---- 7. a single tap: an exact delay, per-sample bound --------------------------------------------
# As test_gpu_conv_pow2.test_single_tap_is_an_exact_delay: one tap g = 0.5 at delay k <= n - sr per
# ear.  The reference's scale n / (n / 2) is exactly 2, so out[j] = 2 g x[j - k] for
# 0 <= j - k < (length // sr) sr and 0 elsewhere, exactly.  Per sample: |got - expected| <= half a
# spacing of the expected f32 (the final rounding) + 1e-12 max|x|.  The 1-ULP-of-max bar of route 1
# cannot see a quiet sample a few of its own ULPs off, nor one sample misplaced at a seam; this can.
def delayed(x, k, gain, sr):
    out = np.zeros(x.size, np.float32)
    m = min((x.size // sr) * sr, x.size - k)  # j - k < S sr and j < len
    out[k:k + m] = np.float32(2.0 * gain) * x[:m]
    return out


@pytest.mark.parametrize("c", [c for c in CASES if c.tap], ids=case_id)
def test_single_tap_is_an_exact_delay(c):
    n, sr = c.sr * c.secs, c.sr
    assert n % 2 == 0
    length = 5 * sr + ragged(c)
    rng = np.random.default_rng([c.sr, c.secs, 7])
    x = (0.3 * rng.standard_normal(length)).astype(np.float32)
    last = n - sr
    mid = int(rng.integers(1, last))  # strictly between 0 and n - sr
    ears = [((0, 0.5), (last, 0.5)), ((mid, 0.5), (0, 0.5)), ((last, 0.5), (mid, 0.5))]
    slack = 1e-12 * float(np.abs(x).max())
    r = pinned_renderer(c)
    try:
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
                print(f"{c.n1}x{c.n2} {ear} k={k}: worst err {err.max():.3e} = {err.max() / np.abs(x).max():.3e} "
                      f"max|x|, {bad.size} samples over the bound")
                assert bad.size == 0, (ear, k, g, bad[:8], got[bad[:8]], want[bad[:8]])
    finally:
        r.close()
