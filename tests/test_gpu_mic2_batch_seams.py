"""The sub-batch seams of the MIC2 whole-volume batches, in a child process under a small workspace ceiling."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_sub_batch_seams_under_a_small_workspace(gpu_ready):
    """tests/mic2_batch_chunking_check.py in a fresh process with a 7 MiB workspace ceiling: 150 x 70 frames go three to a sub-batch,
    160 x 96 frames two, the small ones three (the arithmetic of test_gpu_mic2_multi_crops.py's seam test), and the script's volumes
    are ordered so that the cuts fall inside temporal volumes, behind a frame 0, between volumes and around an independent volume.
    MIC_HIP_PIPELINE_PARTS=3 as in the other host doors' seam runs: here the parts are the sub-batches whatever it says."""
    env = dict(os.environ, MIC_HIP_WS_BUDGET_MB="7", MIC_HIP_PIPELINE_PARTS="3")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mic2_batch_chunking_check.py")], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "mic2 batch seams ok" in r.stdout, r.stdout + r.stderr
