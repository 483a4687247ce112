"""The staging driver every host batch entry point runs on (csrc/mic_staged.h), without a device: tests/staged_pipeline/driver.cpp
is a plain C++ program that fakes the transfers with real IoReqs completed by helper threads, and checks in every callback what
the header promises -- run(k) in order and never after a failure; up[k] and down[k - 2] complete when run(k) starts; upload(k + 1)
between the return of run(k - 1) and the start of run(k), into half (k + 1) & 1; next_up the request of upload(k + 1) or null;
nothing in flight at the return; the first failure's code returned."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (1, 2, 3, 5)
# a callback of part k that returns an error (upload, run), a transfer of part k that fails (up, down): every part of every length
CASES = [(n, "none", 0) for n in PARTS] + [(n, what, k) for n in PARTS for what in ("upload", "run", "up", "down") for k in range(n)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("staged") / "driver")
    cmd = [cxx, "-std=c++17", "-pthread", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "medical-image-codec_amd", "csrc"),
           os.path.join(ROOT, "tests", "staged_pipeline", "driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("parts,what,k", CASES)
def test_the_driver_keeps_its_protocol(driver, parts, what, k):
    r = subprocess.run([driver, str(parts), what, str(k)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
