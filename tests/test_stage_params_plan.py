"""The CW filter map in the call plan (t41_sdr_amd/csrc/rx_plan.hpp: CallFacts::cw_unfiltered, Back::cw_mixed).
tests/stage_params_plan_check.cpp walks every CallFacts combination, cw_unfiltered included: without the new fact every
plan is what it was (against plan_call() with the fact cleared, and the back end against the expression as it stood);
with it nothing but the back end moves, cw_mixed occurs exactly at 192 kS/s with some channel filtered and some not, an
all-off map never plans a CW back end, and the back end's invariants of tests/call_plan_check.cpp hold with cw_mixed among
the hand-over back ends.  Built with the host compiler and the address / undefined-behaviour sanitizers and run as it is,
like tests/test_call_plan.py.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_params_plan_holds_for_every_combination(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the stage params plan check is a plain C++17 program")
    exe = str(tmp_path / "stage_params_plan_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan",
         "-I", os.path.join(ROOT, "t41_sdr_amd", "csrc"), os.path.join(ROOT, "tests", "stage_params_plan_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    # 4 lengths x 4 families x 2^22 switches x 2 frame counts
    assert "stage params plan: %d plans walked, no violation" % (4 * 4 * (1 << 22) * 2) in run.stdout
