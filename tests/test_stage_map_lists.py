"""The stage map's lists (t41_sdr_amd/csrc/rx_stagemap.hpp): build_stage_lists() turns the masks of t41rx_set_stage_map into
the ascending channel list of each stage and the blanker's complement, and refuses what the setter refuses.
tests/stage_map_check.cpp walks it -- every accepted mask over a few channels, the empty list, all channels, lists of 1 / 16 /
17 / 64 / 65, the complement, every refusal; this test builds it with the host compiler and the address /
undefined-behaviour sanitizers and runs it.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_lists_hold_for_every_map(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the stage map check is a plain C++17 program")
    exe = str(tmp_path / "stage_map_check")
    # (the sanitizers' runtimes linked into the program: it runs as it is, whatever the environment loads next to it)
    build = subprocess.run(
        [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan",
         "-I", os.path.join(ROOT, "t41_sdr_amd", "csrc"), os.path.join(ROOT, "tests", "stage_map_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    # 24 + 24^2 + 24^3 small maps, 10 sizes x (2 + 24), 5 stages x 5 lengths, one random map, 6 + 15 + 24 + 1 refusals
    walked = 24 + 24 ** 2 + 24 ** 3 + 10 * 26 + 25 + 1 + 6 + 15 + 24 + 1
    assert "stage map lists: %d maps walked, no violation" % walked in run.stdout
