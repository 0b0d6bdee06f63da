"""The panadapter map's list (t41_sdr_amd/csrc/rx_panmap.hpp): check_pan_map() checks the rows of t41rx_set_panadapter_map and
refuses what the setter refuses, pan_list_of() turns them and the parameter sets' gains into the ascending list of {channel,
row, RFgain, rfGainAllBands} entries the list forms of the panadapter and beacon kernels run on.  tests/pan_map_check.cpp
walks them -- the three maps of test_panadapter_map.py, 4096 channels with 2 listed, lists of 0 / 1 / all, the gains taken
from the channel's own set and a rebuild after a set change, every refusal with its entry named; this test builds it with
the host compiler and the address / undefined-behaviour sanitizers and runs it.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_panadapter_list_holds_for_every_map(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the panadapter map check is a plain C++17 program")
    exe = str(tmp_path / "pan_map_check")
    # (the sanitizers' runtimes linked into the program: it runs as it is, whatever the environment loads next to it)
    build = subprocess.run(
        [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan",
         "-I", os.path.join(ROOT, "t41_sdr_amd", "csrc"), os.path.join(ROOT, "tests", "pan_map_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    # the three maps; 4096 channels with nobody (two sizes of rows) and with 2 listed; 4 sizes x (nobody, one on the last row,
    # all reversed); the sets' table and 4 rebuilds; the map the refusals start from; 5 + 1 + 5 + 15 + 3 + 2 refusals; 1
    # accepted and 4 refused with the panadapter on
    walked = 3 + 3 + 4 * 3 + (1 + 4) + 1 + (5 + 1 + 5 + 15 + 3 + 2) + (1 + 4)
    assert "panadapter map lists: %d maps walked, no violation" % walked in run.stdout
