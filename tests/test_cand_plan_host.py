"""CPU: how replay_cand_kernel's blocks find their parts of a candidate list from the heads
(csrc/arx_cand_plan.hpp).  tests/cpp/cand_plan.cpp walks the header's functions as the kernel does -- tiles of
256 heads, four a lane, a scan, the owner lane's cand_lane_item -- over the lists written here; the
expectation is the plain double loop over stretches and their parts, dealt to the blocks in turn."""
import os
import random
import shutil
import subprocess

import pytest

from conftest import REPO


def lists():
    rng = random.Random(19)
    crowded = [1024] * 27 + [rng.randrange(0, 200) for _ in range(40)] + [0] * 910  # 977 stretches: 1 M rays
    out = {"crowded": (2048, crowded), "crowded_few_blocks": (7, crowded),
           "empty": (16, [0] * 300), "one_stretch": (16, [65]), "one_candidate_last": (4, [0] * 256 + [1]),
           "full": (64, [1024] * 257), "edges": (5, [0, 1, 63, 64, 65, 1023, 1024, 0, 0, 128] * 30),
           "tile_boundary": (3, [0] * 255 + [1024, 1024] + [0] * 254 + [64, 1]),
           "random": (33, [rng.choice([0, 0, 0, rng.randrange(1025)]) for _ in range(1500)]),
           "more_blocks_than_parts": (2048, [3, 0, 70])}
    return out


def double_loop(heads):
    return [(fb, part, n) for fb, n in enumerate(heads) for part in range((n + 63) // 64)]


def run_driver(tmp_path, flags=()):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe, cases = str(tmp_path / "cand_plan"), str(tmp_path / "cases.txt")
    with open(cases, "w") as fh:
        for name, (blocks, heads) in lists().items():
            fh.write(f"{name} {blocks} {len(heads)} " + " ".join(str(h) for h in heads) + "\n")
    subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(REPO, "audiorenderingv2_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "cand_plan.cpp"), "-o", exe], check=True)
    return subprocess.run([exe, cases], capture_output=True, text=True, check=True).stdout.splitlines()


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    return run_driver(tmp_path_factory.mktemp("cand_plan"))


def test_every_part_goes_to_one_block_in_stretch_order(rows):
    got, name = {}, None
    for ln in rows:
        w = ln.split()
        if w[0] == "case":
            name = w[1]
            got[name] = {"items": int(w[4]), "blocks": {}}
        else:
            got[name]["blocks"][int(w[1])] = [tuple(int(v) for v in p.split(":")) for p in w[2:]]
    assert set(got) == set(lists())
    for name, (blocks, heads) in lists().items():
        want = double_loop(heads)
        assert got[name]["items"] == len(want), name
        assert sorted(got[name]["blocks"]) == list(range(blocks)), name
        for j in range(blocks):  # block j: parts j, j + blocks, ...
            assert got[name]["blocks"][j] == want[j::blocks], (name, j)
    assert got["empty"]["items"] == 0 and got["full"]["items"] == 257 * 16 and got["one_stretch"]["items"] == 2


def test_the_driver_is_clean_under_the_sanitizers(tmp_path, rows):
    """The same program once more with -fsanitize=address,undefined, stand-alone: the same output, no report."""
    assert run_driver(tmp_path, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")) == rows
