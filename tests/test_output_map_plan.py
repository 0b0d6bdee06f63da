"""The output map in the call plan (t41_sdr_amd/csrc/rx_plan.hpp: CallFacts::omap, KernelForm::omap_form).
tests/output_map_plan_check.cpp walks every CallFacts combination, omap included: without a map every plan is what it is
for the same facts with omap cleared; with one, a call at fft_length 512 takes the fused twin or the hand-over, exactly
one of them, the long lengths are invalid with a text, and every form named is compiled.  Built with the host compiler
and the address / undefined-behaviour sanitizers and run as it is, like tests/test_call_plan.py.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_output_map_plan_holds_for_every_combination(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the output map plan check is a plain C++17 program")
    exe = str(tmp_path / "output_map_plan_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan",
         "-I", os.path.join(ROOT, "t41_sdr_amd", "csrc"), os.path.join(ROOT, "tests", "output_map_plan_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    # 4 lengths x 4 families x 2^21 switches x 2 frame counts
    assert "output map plan: %d plans walked, no violation" % (4 * 4 * (1 << 21) * 2) in run.stdout
