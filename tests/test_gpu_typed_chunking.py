"""Typed crops over several sub-batches: the temporal MIC2 staging tensor carries the running sums across the seams, strip files
gather typed samples slab by slab (tests/typed_chunking_check.py, in a process of its own because the workspace ceiling is read once)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_typed_crops_across_sub_batch_seams():
    """7 MiB hold three frames of 150 x 70 (tests/test_gpu_mic2_crops.py::test_sub_batch_seams_under_a_small_workspace has the
    arithmetic): 11 frames take four sub-batches; the 23 strips of the five strip files take at least as many"""
    env = dict(os.environ, MIC_HIP_WS_BUDGET_MB="7")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "typed_chunking_check.py")], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "typed crop seams ok" in r.stdout, r.stdout + r.stderr
