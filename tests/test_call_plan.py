"""The call plan (t41_sdr_amd/csrc/rx_plan.hpp): plan_call() decides which kernels a process call runs, and every consumer
reads its answer.  tests/call_plan_check.cpp walks every CallFacts combination and checks what the consumers rely on;
this test builds it with the host compiler and the address / undefined-behaviour sanitizers and runs it.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_call_plan_holds_for_every_combination(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the call plan check is a plain C++17 program")
    exe = str(tmp_path / "call_plan_check")
    # (the sanitizers' runtimes linked into the program: it runs as it is, whatever the environment loads next to it)
    build = subprocess.run(
        [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan",
         "-I", os.path.join(ROOT, "t41_sdr_amd", "csrc"), os.path.join(ROOT, "tests", "call_plan_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    # 4 lengths x 4 families x 2^20 switches x 4 frame counts
    assert "call plan: %d plans walked, no violation" % (4 * 4 * (1 << 20) * 4) in run.stdout
