"""Run by tests/test_gpu_wavelet_mixed.py::test_sub_batches_under_a_small_workspace in a child process with MIC_HIP_WS_BUDGET_MB set
small, so that the WaveletV2 jobs calls cut the tiling list into several sub-batches: each call runs exactly the sub-batches
mic_hip_wavelet_v2_batch_plan counts for its jobs, and every file and image is still the oracle's."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry
mic = entry.load_package()
from oracle import mico
import wavelet_mixed_frames as F

mb = int(os.environ["MIC_HIP_WS_BUDGET_MB"])
for jobs in (F.tiling_jobs(), F.tiling_jobs()[::-1]):
    want = [mico.wavelet_v2_compress(img, mv, lv) for img, mv, lv in jobs]
    plan = mic.wavelet_v2_batch_plan([j[0].shape for j in jobs])              # (budget 0: the call's own ceiling, the environment's)
    assert plan.tolist() == F.plan([j[0].shape for j in jobs], mb << 20) and len(plan) - 1 >= 3, plan
    res, stats = mic.wavelet_v2_compress_jobs([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
    assert stats["sub_batches"] == stats["chains"] == len(plan) - 1, (stats, plan)
    assert [(st, f) for st, f, _ in res] == want
    good = [k for k, (rc, _) in enumerate(want) if rc == 0]
    dplan = mic.wavelet_v2_batch_plan([jobs[k][0].shape for k in good])
    back, dstats = mic.wavelet_v2_decompress_jobs([want[k][1] for k in good])
    assert dstats["sub_batches"] == dstats["chains"] == len(dplan) - 1 >= 3 and dstats["frames_done"] == len(good), (dstats, dplan)
    for k, (st, img, _) in zip(good, back):
        assert st == 0 and np.array_equal(img, jobs[k][0]), k
print("wavelet mixed seams ok: %d sub-batches" % (len(mic.wavelet_v2_batch_plan([j[0].shape for j in F.tiling_jobs()])) - 1))
