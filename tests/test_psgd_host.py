"""The host rules of the minibatch unit (csrc/spfm_psgd_host.h: step sizes, the tabulated epoch,
the shares of a sharded epoch, the permutation and CSR checks of the pair fit and its sampler):
the stand-alone checker tools/check_psgd_host.cpp, built with the host sanitizers and run as a
program of its own (nothing of it is loaded into this process)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_psgd_host_rules_match_the_loops_they_replaced(tmp_path):
    exe = str(tmp_path / "check_psgd_host")
    build = subprocess.run(
        # (the sanitizer runtimes linked in: the program runs whatever else the environment loads)
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
         os.path.join(ROOT, "tools", "check_psgd_host.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"
