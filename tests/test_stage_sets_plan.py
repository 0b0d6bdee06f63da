"""The plan of a call with parameter sets loaded next to the chain-splitting stages (t41_sdr_amd/csrc/rx_plan.hpp:
CallFacts::stage_sets).  tests/stage_sets_plan_check.cpp walks every CallFacts -- both ends of the fft_length range, the
four demodulator families, every combination of the twenty-two switches, calls of three and of four frames.  With the fact
false the plan is held to the expectations tests/call_plan_check.cpp states for the plan before the fact existed; with it
true, sets and a stage at fft_length 512 make a valid call that takes the tap kernel in its set form, hands over and ends
in the back end of the same call without sets, and every other call plans as with the fact false.  This test builds the
program with the host compiler and runs it.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_sets_plan_holds_for_every_call(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the stage sets plan check is a plain C++17 program")
    exe = str(tmp_path / "stage_sets_plan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "t41_sdr_amd", "csrc"),
                            os.path.join(ROOT, "tests", "stage_sets_plan_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    # 2 lengths x 4 families x (2^22 switch combinations less the quarter with cw_unfiltered and no filter) x 2 call lengths;
    # staged: length 512, sets on, 15 free switches, the 47 non-empty (stages, cw_unfiltered) combinations
    walked = 2 * 4 * (2 ** 22 * 3 // 4) * 2
    staged = 4 * 2 * 2 ** 15 * 47
    assert "stage sets plan: %d facts walked, %d staged calls, no violation" % (walked, staged) in run.stdout
