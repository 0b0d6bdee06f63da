"""The CW filter map's lists (t41_sdr_amd/csrc/rx_stageparams.hpp): build_cw_filter_lists() turns the indices of
t41rx_set_cw_filter_map and the output map's rows into the ascending list of filtered channels and the row map of each of
the two back kernels, and refuses what the setter refuses.  tests/stage_params_check.cpp walks it -- every map over
{0..5}^n for n <= 4, sizes 1 / 7 / 8 / 9 / 16 / 17 / 64 / 65 with random maps, nobody and everybody filtered, each with no
output map, the identity, all muted and a random one; every refusal, which leaves `out` as it was; this test builds it with
the host compiler and the address / undefined-behaviour sanitizers and runs it.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_filter_lists_hold_for_every_map(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the stage params check is a plain C++17 program")
    exe = str(tmp_path / "stage_params_check")
    # (the sanitizers' runtimes linked into the program: it runs as it is, whatever the environment loads next to it)
    build = subprocess.run(
        [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan",
         "-I", os.path.join(ROOT, "t41_sdr_amd", "csrc"), os.path.join(ROOT, "tests", "stage_params_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    # (6 + 6^2 + 6^3 + 6^4 small maps and 8 sizes x 5 kinds) x 4 output maps; per size 4 + 1 + 1 refusals of n and NULL,
    # 3 places x 4 values x 2 of the range, 3 of the tables, and the all-off map without tables
    walked = (6 + 6 ** 2 + 6 ** 3 + 6 ** 4 + 8 * 5) * 4 + 8 * (6 + 24 + 3 + 1)
    assert "stage params lists: %d maps walked, no violation" % walked in run.stdout
