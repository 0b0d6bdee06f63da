"""What the noise reduction reads per channel under parameter sets loaded next to the stages
(t41_sdr_amd/csrc/rx_stagesets.hpp): build_stage_sets() turns the sets' noise-reduction values, the channels' table, the
optional noise-reduction map and the optional stage map into every channel's effective kind and notch, its row of the
device table and the lists of the two launches, and refuses what the setters refuse.  tests/stage_sets_check.cpp walks it
against a restatement -- every pair of sets over the eight (kind, notch) codes with a passing and a failing pass band on up
to three channels, random sets at 15 / 16 / 17 / 19 / 33 / 65 channels, each without a map, with every all-equal map and
random maps, each with no stage map, the identity, nobody listed and a random one; every refusal, which leaves `out` as it
was.  This test builds it with the host compiler and the address / undefined-behaviour sanitizers and runs it.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_sets_lists_hold_for_every_case(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the stage sets check is a plain C++17 program")
    exe = str(tmp_path / "stage_sets_check")
    # (the sanitizers' runtimes linked into the program: it runs as it is, whatever the environment loads next to it)
    build = subprocess.run(
        [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan",
         "-I", os.path.join(ROOT, "t41_sdr_amd", "csrc"), os.path.join(ROOT, "tests", "stage_sets_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    # (16 one-set cases x 3 tables + 256 two-set cases x (2 + 4 + 8 tables) + 6 sizes x 3 random) x 4 stage maps x (no map
    # + 8 all-equal + 2 random maps); 8 refusals of counts and pointers, 3 places x 4 values x 3 arrays, 2 of a set's own
    # values, 2 of the spectral check and the accepted failing set nobody names
    walked = (16 * 3 + 256 * 14 + 6 * 3) * 4 * 11 + 8 + 36 + 2 + 2 + 1
    m = re.search(r"stage sets: (\d+) cases walked, no violation", run.stdout)
    assert m and int(m.group(1)) == walked, run.stdout
