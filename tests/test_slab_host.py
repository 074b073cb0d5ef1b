"""The partition rule of the row-wise read-only units (csrc/spfm_slab_host.h): the stand-alone
checker tools/check_slab_host.cpp, built with the host sanitizers and run as a program of its own
(nothing of it is loaded into this process)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_slab_end_matches_the_loops_it_replaced(tmp_path):
    exe = str(tmp_path / "check_slab_host")
    build = subprocess.run(
        # (the sanitizer runtimes linked in: the program runs whatever else the environment loads)
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
         os.path.join(ROOT, "tools", "check_slab_host.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "ok"
