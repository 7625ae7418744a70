"""CPU: the plan both listener batches run on (csrc/arx_batch_plan.hpp) -- the chunk scratch's and the pinned
block's layout, the byte terms of arx_debug_listener_bytes / arx_debug_listener_band_bytes and the chunk
choice -- walked by tests/cpp/batch_plan.cpp over bands x chunk x rays x ir_len and checked here against
the closed forms include/arx.h documents."""
import math
import os
import shutil
import subprocess

import pytest

from conftest import REPO

BANDS, CHUNKS, RAYS, LENS = (0, 1, 4, 5, 8), (1, 2, 64), (1, 1024, 1025), (1, 16000)
ACOU = 4100                          # the driver's analysis scratch: no multiple of 16
RECV_NODES, RECV_TRIS = 1019, 1020   # the 1 020-triangle head
ENTRY, RESULTS, BLOCK = 112, 336, 64  # a table entry, three arx_acoustics, a counter block


def up16(v):
    return (v + 15) // 16 * 16


def parse(line):
    """A driver row: its leading numbers, and its name:offset:size regions."""
    words = line.split()
    nums = [w for w in words[1:] if ":" not in w]
    regs = {w.split(":")[0]: tuple(int(v) for v in w.split(":")[1:]) for w in words[1:] if ":" in w}
    return [int(v) for v in nums], regs


def check_regions(regs, total, aligned_sum):
    """Every offset 16-B aligned, the regions disjoint and inside `total`; with aligned_sum, `total` the sum
    of the sizes rounded up to 16."""
    spans = sorted((at, at + size) for at, size in regs.values() if size > 0)
    for at, _ in regs.values():
        assert at % 16 == 0
    for (a0, a1), (b0, _) in zip(spans, spans[1:]):
        assert a1 <= b0, (spans,)
    assert spans[0][0] >= 0 and spans[-1][1] <= total
    if aligned_sum:
        assert total == sum(up16(size) for _, size in regs.values())


def documented_each(rays, ir_len, bands):
    heads = math.ceil(rays / 1024)
    shared = 96 * RECV_NODES + 48 * RECV_TRIS + 96 + ENTRY + 16 * rays + 16 * heads + 16 + 64 * heads
    if bands == 0:  # tests/test_listeners_host.py's closed form
        return shared + 16 * ir_len + 128 + RESULTS + 8 * ir_len
    return shared + bands * (16 * ir_len + BLOCK + RESULTS + 8 * ir_len) + BLOCK + 8 * ir_len  # test_listener_bands_host.py's


def run_driver(tmp_path, flags=()):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "batch_plan")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(REPO, "audiorenderingv2_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "batch_plan.cpp"), "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    return run_driver(tmp_path_factory.mktemp("batch_plan"))


def test_the_scratch_layout(rows):
    seen = set()
    for line in (ln for ln in rows if ln.startswith("scratch ")):
        (bands, chunk, rays, ir_len, total), regs = parse(line)
        list_stride, work_stride = regs.pop("strides")
        heads = math.ceil(rays / 1024)
        cells = max(bands, 1)
        assert list_stride == 16 * rays + 16 * heads and work_stride == 16 + 64 * heads
        want = {"counts": 8 * rays if bands else 0, "base": 8 * BLOCK if bands else 0, "edc": 24 * ir_len, "acou": ACOU,
                "lists": chunk * list_stride, "work": chunk * work_stride, "table": chunk * ENTRY,
                "hist": chunk * cells * 16 * ir_len, "counters": chunk * (cells + 1) * BLOCK, "res": chunk * cells * RESULTS,
                "ir": chunk * cells * 8 * ir_len, "bb": chunk * 8 * ir_len if bands else 0}
        assert {k: size for k, (_, size) in regs.items()} == want, line
        check_regions(regs, total, aligned_sum=True)
        # the per-call regions come first
        assert regs["counts"][0] == 0 and regs["base"][0] <= regs["edc"][0] <= regs["acou"][0] < regs["lists"][0]
        seen.add((bands, chunk, rays, ir_len))
    assert seen == {(b, j, n, ln) for b in BANDS for j in CHUNKS for n in RAYS for ln in LENS}


def test_the_pinned_layout(rows):
    seen = set()
    for line in (ln for ln in rows if ln.startswith("pinned ")):
        (bands, n, total), regs = parse(line)
        cells, halves = max(bands, 1), 1 if bands else 2  # the plain call's [n, 2n) half for the one-listener route
        want = {"entries": n * ENTRY, "counters": halves * n * (cells + 1) * BLOCK, "res": halves * n * cells * RESULTS, "flag": 16}
        assert {k: size for k, (_, size) in regs.items()} == want, line
        check_regions(regs, total, aligned_sum=True)
        seen.add((bands, n))
    assert seen == {(b, j) for b in BANDS for j in CHUNKS}


def test_the_byte_terms_are_the_documented_formulas(rows):
    seen = set()
    for line in (ln for ln in rows if ln.startswith("bytes ")):
        (bands, rays, ir_len, each, fixed), _ = parse(line)
        assert each == documented_each(rays, ir_len, bands), line
        assert fixed == (8 * rays + 512 if bands else 0), line
        seen.add((bands, rays, ir_len))
    assert seen == {(b, n, ln) for b in BANDS for n in RAYS for ln in LENS}


def test_the_chunk_choice(rows):
    got = {ln.split()[1]: int(ln.split()[2]) for ln in rows if ln.startswith("chunk ")}
    assert got == {"forced_5_left_3": 3, "forced_5_left_9": 5,
                   "header_8_bands": 14, "header_4_bands": 20, "header_8_bands_left_9": 9,  # include/arx.h's figures
                   "budget_below_fixed": 0, "budget_at_fixed": 0,
                   "cap": 64, "cap_small_listeners": 64}


def test_the_driver_is_clean_under_the_sanitizers(tmp_path, rows):
    """The same program once more with -fsanitize=address,undefined, stand-alone: the same output, no report."""
    assert run_driver(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")) == rows
