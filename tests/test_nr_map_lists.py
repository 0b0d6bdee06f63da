"""The noise-reduction map's lists (t41_sdr_amd/csrc/rx_nrmap.hpp): build_nr_map_lists() turns the two arrays of
t41rx_set_nr_map and the stage map into the spectral list with its kinds, the Xanr() list sorted into its three classes and
the table of workgroups over it, and refuses what the setter refuses.  tests/nr_map_check.cpp walks it -- every map over
({0..3} x {0, 1})^n for n <= 3, sizes 1 / 15 / 16 / 17 / 33 / 64 / 65 with random maps, the empty map, every combination
alone, a class of exactly 1, 16 and 17 channels, each with no stage map, the identity, nobody listed and a random one;
every refusal, which leaves `out` as it was; this test builds it with the host compiler and the address /
undefined-behaviour sanitizers and runs it.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nr_map_lists_hold_for_every_map(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the nr map check is a plain C++17 program")
    exe = str(tmp_path / "nr_map_check")
    # (the sanitizers' runtimes linked into the program: it runs as it is, whatever the environment loads next to it)
    build = subprocess.run(
        [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-static-libasan", "-static-libubsan",
         "-I", os.path.join(ROOT, "t41_sdr_amd", "csrc"), os.path.join(ROOT, "tests", "nr_map_check.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    # (8 + 8^2 + 8^3 small maps, 7 sizes x (2 random + 8 combinations), and 3 classes x the 16 (size, count) pairs with
    # count <= size) x 4 stage maps; per size 4 + 1 + 3 refusals of n and NULL and 3 places x 4 values x 2 arrays
    walked = (8 + 8 ** 2 + 8 ** 3 + 7 * 10 + 3 * 16) * 4 + 7 * (8 + 24)
    assert "nr map lists: %d maps walked, no violation" % walked in run.stdout
