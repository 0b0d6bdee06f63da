"""The FT8 map's list (t41_sdr_amd/csrc/rx_ft8map.hpp): build_ft8_list() checks the rows of t41rx_set_ft8_map and turns them
into the ascending list of {channel, row} pairs the list forms of the FT8 kernels run on, and refuses what the setter
refuses.  tests/ft8_map_check.cpp walks it -- every map of 1 .. 4 channels, lists of 0 / 1 / all, a permutation, every
refusal; this test builds it with the host compiler and the address / undefined-behaviour sanitizers and runs it.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ft8_list_holds_for_every_map(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the FT8 map check is a plain C++17 program")
    exe = str(tmp_path / "ft8_map_check")
    # (the sanitizers' runtimes linked into the program: it runs as it is, whatever the environment loads next to it)
    build = subprocess.run(
        [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan",
         "-I", os.path.join(ROOT, "t41_sdr_amd", "csrc"), os.path.join(ROOT, "tests", "ft8_map_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    # every map of n = 1 .. 4 channels over n_rows = 1 .. n rows, (n_rows + 1)^n each; 4 sizes x (nobody, one on row 0, one on
    # the last row, all); one permutation; the map the refusals start from; 5 + 1 + 5 + 15 + 3 + 2 refusals; 1 accepted and
    # 4 refused with FT8 receive on
    small = sum((r + 1) ** n for n in range(1, 5) for r in range(1, n + 1))
    assert small == 1092
    walked = small + 4 * 4 + 1 + 1 + (5 + 1 + 5 + 15 + 3 + 2) + (1 + 4)
    assert "FT8 map lists: %d maps walked, no violation" % walked in run.stdout
