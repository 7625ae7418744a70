"""CPU: the plan choice of the mixed-radix direct convolution (arx_conv.hip), restated, against the
case table that tests/test_gpu_conv_direct.py runs on the GPU.

conv_plan_create takes the direct path when ir_len = N1 x N2 with both factors 7-smooth and <= 512
(direct_split); mr_dispatch then picks one of ten sets of kernel template arguments -- four
compile-time plans (300 x 320, 160 x 200, 315 x 280, 250 x 256) and the run-time plans
Mr<R7, LM, 0, 0>, R7 in {false, true} x LM in {320, 512} -- and chain_plan picks the chained pass C
(pass_c_chain / pass_c_chain3: n = 2 sr and N1 even) or pass_c_mr + pass_d ("windowed").  The GPU
file has one case per cell of that matrix and per shape edge the template code branches on; this
file restates factor7, direct_split, mr_dispatch's choice and chain_plan in Python and asserts, for
every row of the table, its split, radices, family and pass C, that the table covers every cell, and
that every edge is held by a row.  A later change to direct_split that moves a row fails here with
the row named; on the GPU it would otherwise silently test another kernel.
"""
from collections import namedtuple

import pytest

K_MAX_SUB_LEN = 512  # kMaxSubLen
K_MAX_RADICES = 12   # kMaxRadices
CT_PLANS = ((300, 320), (160, 200), (315, 280), (250, 256))  # mr_dispatch's compile-time plans
TC_A, TC_C, TC_LIVE = 8, 4, 2  # columns per workgroup: ARX_CONV_TCA, ARX_CONV_TCC, the live block


def factor7(L):
    """factor7: L = 8^a 4^b 2^c 3^d 5^e 7^f in stage order, or None."""
    v, twos, r = L, 0, []
    while v % 2 == 0:
        v //= 2
        twos += 1
    while twos >= 3:
        r.append(8)
        twos -= 3
    if twos == 2:
        r.append(4)
    if twos == 1:
        r.append(2)
    for q in (3, 5, 7):
        while v % q == 0:
            v //= q
            r.append(q)
    return r if v == 1 and len(r) <= K_MAX_RADICES else None


def direct_split(n):
    """direct_split: (N1, N2) or None; N2 % 8 == 0 preferred, then the most balanced, the first
    such d winning a tie."""
    best, split = -1, None
    for d in range(2, K_MAX_SUB_LEN + 1):
        if n % d:
            continue
        e = n // d
        if e < 2 or e > K_MAX_SUB_LEN or factor7(d) is None or factor7(e) is None:
            continue
        score = (1000000 if e % 8 else 0) + abs(d - e)
        if best < 0 or score < best:
            best, split = score, (d, e)
    return split


Plan = namedtuple("Plan", "n1 n2 f1 f2 family chained")


def plan_of(ir_len, sr):
    """conv_plan_create + mr_dispatch + chain_plan for a direct plan, or None (power-of-two path).
    family: "ct" for a compile-time plan, else "F/320", "T/320", "F/512", "T/512" (R7 / LM)."""
    split = direct_split(ir_len) if ir_len >= sr else None
    if split is None:
        return None
    n1, n2 = split
    f1, f2 = factor7(n1), factor7(n2)
    if split in CT_PLANS:
        family = "ct"
    else:
        family = ("T" if 7 in f1 + f2 else "F") + ("/320" if max(n1, n2) <= 320 else "/512")
    return Plan(n1, n2, f1, f2, family, ir_len == 2 * sr and n1 % 2 == 0)


def tiles(n2, tc):
    return -(-n2 // tc)


def remapped_and_ragged(n2, tc):
    """xcd_tile's remapped branch (a tile count that is a multiple of 8) with a ragged last tile."""
    return tiles(n2, tc) % 8 == 0 and n2 % tc != 0


# (sr, secs) -> N1, N2, radices of N1 and of N2, family, chained pass C; `live`: also a live-block
# case, `tap`: also a single-tap case of the GPU file
Case = namedtuple("Case", "sr secs n1 n2 f1 f2 family chained live tap")
CASES = [
    Case(5, 2, 2, 5, [2], [5], "F/320", True, False, False),
    Case(8, 2, 2, 8, [2], [8], "F/320", True, False, False),
    Case(9, 2, 3, 6, [3], [2, 3], "F/320", False, False, False),
    Case(10, 2, 4, 5, [4], [5], "F/320", True, False, False),
    Case(18, 2, 6, 6, [2, 3], [2, 3], "F/320", True, True, True),
    Case(3125, 2, 50, 125, [2, 5, 5], [5, 5, 5], "F/320", True, True, True),
    Case(7, 2, 2, 7, [2], [7], "T/320", True, False, False),
    Case(21, 2, 6, 7, [2, 3], [7], "T/320", True, False, False),
    Case(1575, 2, 50, 63, [2, 5, 5], [3, 3, 7], "T/320", True, False, True),
    Case(22050, 2, 210, 210, [2, 3, 5, 7], [2, 3, 5, 7], "T/320", True, True, True),
    Case(441, 2, 21, 42, [3, 7], [2, 3, 7], "T/320", False, False, False),
    Case(46875, 2, 250, 375, [2, 5, 5, 5], [3, 5, 5, 5], "F/512", True, True, False),
    Case(131072, 2, 512, 512, [8, 8, 8], [8, 8, 8], "F/512", True, True, False),
    Case(37500, 2, 375, 200, [3, 5, 5, 5], [8, 5, 5], "F/512", False, False, False),
    Case(16807, 2, 98, 343, [2, 7, 7], [7, 7, 7], "T/512", True, True, True),
    Case(9604, 2, 343, 56, [7, 7, 7], [8, 7], "T/512", False, True, False),
    Case(32000, 2, 250, 256, [2, 5, 5, 5], [8, 8, 4], "ct", True, False, False),
]
RUN_TIME_FAMILIES = ("F/320", "T/320", "F/512", "T/512")


def case_id(c):
    return f"{c.sr}x{c.secs}"


def check_case(c):
    """The row against the restated plan choice; the message names the row and what moved."""
    p = plan_of(c.sr * c.secs, c.sr)
    where = f"case sr={c.sr} secs={c.secs}"
    assert p is not None, f"{where}: no direct plan (power-of-two path)"
    assert (p.n1, p.n2) == (c.n1, c.n2), f"{where}: split {p.n1}x{p.n2}, table says {c.n1}x{c.n2}"
    assert (p.f1, p.f2) == (c.f1, c.f2), f"{where}: radices {p.f1} / {p.f2}, table says {c.f1} / {c.f2}"
    assert p.family == c.family, f"{where}: kernel family {p.family}, table says {c.family}"
    assert p.chained == c.chained, f"{where}: chained pass C {p.chained}, table says {c.chained}"


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_case_takes_the_plan_the_table_says(c):
    check_case(c)
    # the live plan (hop min(ir_len, 4096)) splits the same ir_len: the same kernel family
    n = c.sr * c.secs
    live = plan_of(n, min(n, 4096))
    assert (live.n1, live.n2, live.family) == (c.n1, c.n2, c.family)


def test_restatement_on_the_usual_rates():
    """The splits DESIGN.md and arx_conv.hip name, and two lengths that are not direct plans."""
    for sr, secs, want in ((48000, 2, (300, 320)), (16000, 2, (160, 200)), (44100, 2, (315, 280)),
                           (32000, 2, (250, 256)), (22050, 1, (147, 150)), (96000, 2, (400, 480))):
        assert direct_split(sr * secs) == want, (sr, secs)
    assert plan_of(2200, 1100) is None       # 11 is no radix
    assert plan_of(288000, 48000) is None    # above 2^18
    assert factor7(320) == [8, 8, 5] and factor7(280) == [8, 5, 7] and factor7(11) is None


def test_table_covers_every_cell():
    """Four run-time families x {chained, windowed}, plus the compile-time 250 x 256."""
    cells = {(c.family, c.chained) for c in CASES}
    for fam in RUN_TIME_FAMILIES:
        for chained in (True, False):
            assert (fam, chained) in cells, f"no case for family {fam}, chained={chained}"
    assert ("ct", True) in cells and any((c.n1, c.n2) == (250, 256) for c in CASES)
    assert len({(c.sr, c.secs) for c in CASES}) == len(CASES)


def test_edges_are_each_held_by_a_case():
    subs = [n for c in CASES for n in (c.n1, c.n2)]
    # single-stage sub-FFTs: fft_mr_wave's swizzled first stage with no second stage (2, 4, 8) and
    # the odd primes alone
    for n in (2, 3, 4, 5, 7, 8):
        assert n in subs and len(factor7(n)) == 1, n
    # N1 = 2: rows 0 and N1 / 2 are all of pass_b_pair; half = 1 in the chained pass C
    assert any(c.n1 == 2 and c.chained for c in CASES)
    # odd N1: row 0 without a partner row in pass_b_pair
    assert any(c.n1 % 2 == 1 for c in CASES) and any(c.n1 == 3 for c in CASES)
    # sub-length kMaxSubLen: every per-lane slot, the largest LDS
    assert any(c.n1 == K_MAX_SUB_LEN and c.n2 == K_MAX_SUB_LEN for c in CASES)
    # a ragged last column tile with a tile count that is a multiple of 8, in passes A and C, on both
    # 320 families
    for fam in ("F/320", "T/320"):
        assert any(c.family == fam and remapped_and_ragged(c.n2, TC_A) and remapped_and_ragged(c.n2, TC_C)
                   for c in CASES), fam
    assert (tiles(125, TC_A), tiles(125, TC_C)) == (16, 32) and (tiles(63, TC_A), tiles(63, TC_C)) == (8, 16)
    # a single ragged tile (fewer columns than one workgroup holds)
    assert any(c.n2 < TC_C for c in CASES) or any(c.n2 < TC_A and c.n2 % TC_C for c in CASES)
    # N1 % 4 == 2: the last row group of pass_b_mr (four rows per workgroup) is half empty
    assert any(c.n1 % 4 == 2 and c.n1 > 2 for c in CASES)
    # every radix together, chained, run-time, at a usual rate
    c = next(c for c in CASES if c.sr == 22050)
    assert (c.n1, c.n2, c.family, c.chained) == (210, 210, "T/320", True) and set(c.f1) == {2, 3, 5, 7}
    # sub-lengths above 320 that are odd, as rows and as columns
    assert any(c.n2 > 320 and c.n2 % 2 for c in CASES) and any(c.n1 > 320 and c.n1 % 2 for c in CASES)
    # the live block: every run-time family, odd N2 (the ragged last tile at two columns per
    # workgroup) on both LM, and the smallest plan
    live = [c for c in CASES if c.live]
    assert {c.family for c in live} == set(RUN_TIME_FAMILIES)
    for lm in ("/320", "/512"):
        assert any(c.family.endswith(lm) and c.n2 % TC_LIVE == 1 for c in live), lm
    assert any(c.n1 * c.n2 < 4096 for c in live)  # the live hop is ir_len itself
    # the single-tap cases: one per run-time family that has a chained plan, and the tiny one
    assert {c.family for c in CASES if c.tap} >= {"F/320", "T/320", "T/512"}


def test_a_moved_row_is_noticed():
    """check_case fails, naming the row, when a row's split or family is not the plan's."""
    c = CASES[5]
    with pytest.raises(AssertionError, match="case sr=3125 secs=2: split 50x125"):
        check_case(c._replace(n1=125, n2=50))
    with pytest.raises(AssertionError, match="kernel family F/320"):
        check_case(c._replace(family="T/320"))
    with pytest.raises(AssertionError, match="chained pass C"):
        check_case(CASES[2]._replace(chained=True))
