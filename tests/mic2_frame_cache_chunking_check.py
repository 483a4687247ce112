"""Run by tests/test_gpu_mic2_frame_cache.py::test_sub_batch_seams_under_a_small_workspace in a child process with
MIC_HIP_WS_BUDGET_MB set small, so that a cached MIC2 crop call cuts its units into sub-batches of `per` (2 .. 5) frames of 64 x 33:
the whole-frame sum of a temporal run then crosses the seams through the carry frame in the session's workspace.  Every crop must
equal the padded source volume, cold and warm.  Cases: a run of all 16 frames; an anchor in the arena whose run's first residual
lies in the second sub-batch; a bypassed frame in the middle sub-batch; an independent file."""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry
mic = entry.load_package()
import mic2_crop_volumes as V
import mic2_frame_cache_volumes as FV

mb = int(os.environ.get("MIC_HIP_WS_BUDGET_MB", "0"))
assert mb, "meant to run with a small workspace budget"
files = FV.make_files(mic, "wave")
vol = files["vol"]
n, h, w = vol.shape
cuts, _ = mic.mic2_batch_plan([(w, h, n)], mb << 20)
per = int(cuts[1])
assert 2 <= per <= 5 and -(-n // per) >= 3, (mb, cuts)


def read(rd, xyz, cw, ch, cd):
    got, st, stats = FV.read_native(lambda *a: rd.read_crops(*a), xyz, cw, ch, cd)
    want = V.expected(vol, xyz, cw, ch, cd)
    for i in range(len(xyz)):
        assert np.array_equal(got[i], want[i]), (xyz[i], cd)
    assert (st == 0).all(), st
    return stats


for temporal in (True, False):
    data = files["files"][temporal]
    # every frame, one run from frame 0 on: cold it is cut at least twice, warm nothing is decoded
    whole = [(-3, -2, 0), (40, 20, 0), (10, 5, -4), (0, 0, 3)]
    with mic.Mic2Reader(data) as rd, mic.FrameCache(w, h, n) as cache:
        rd.set_cache(cache)
        stats = read(rd, whole, 30, 18, n)
        assert stats["frames_decoded"] == n and stats["slabs"] == -(-n // per) >= 3, stats
        assert rd.cache_probe(np.arange(n)).all()
        stats = read(rd, whole, 30, 18, n)
        assert stats["frames_decoded"] == 0 and stats["slabs"] == 0, stats
        rd.set_cache(None)
    if not temporal:
        continue
    # the anchor in the arena, the run's first residual in the second sub-batch: frame 12 is resident; the call names frame
    # per - 1, whose chain from frame 0 fills the first sub-batch, and frame 14, whose residuals 13 and 14 lie in the second
    with mic.Mic2Reader(data) as rd, mic.FrameCache(w, h, n) as cache:
        rd.set_cache(cache)
        read(rd, FV.at_frames([12]), 20, 10, 1)
        assert rd.cache_probe(np.arange(n)).nonzero()[0].tolist() == [12]
        stats = read(rd, FV.at_frames([per - 1, 14], x=-1, y=20), 20, 17, 1)
        assert stats["frames_decoded"] == per + 2 and stats["slabs"] == 2, stats
        assert rd.cache_probe(np.arange(n)).nonzero()[0].tolist() == [per - 1, 12, 14]
        stats = read(rd, FV.at_frames([per - 1, 12, 14], x=30, y=1), 20, 17, 1)
        assert stats["frames_decoded"] == 0 and stats["slabs"] == 0, stats
        # ... and a run that starts behind an anchor in the arena and crosses seams itself: frame 11 behind frame per - 1
        stats = read(rd, FV.at_frames([11], x=5, y=5), 20, 17, 1)
        assert stats["frames_decoded"] == 12 - per and stats["slabs"] == -(-(12 - per) // per) >= 2, stats
        rd.set_cache(None)
    # one slot: the first named frame is kept, the others are bypassed -- frame per + 1 in the middle sub-batch of three, summed
    # into the slab and gathered from there
    with mic.Mic2Reader(data) as rd, mic.FrameCache(w, h, 1) as cache:
        rd.set_cache(cache)
        frames = [1, per + 1, 2 * per + 1]
        stats = read(rd, FV.at_frames(frames, x=w - 9, y=-3), 20, 17, 1)
        assert stats["frames_decoded"] == 2 * per + 2 and stats["slabs"] == 3, stats
        assert rd.cache_probe(np.arange(n)).nonzero()[0].tolist() == [1]
        st = cache.stats()
        assert (st["misses"], st["bypassed"]) == (1, 2), st
        stats = read(rd, FV.at_frames(frames, x=3, y=3), 20, 17, 1)       # warm: frame 1 hits and anchors the other two
        assert stats["frames_decoded"] == 2 * per and stats["slabs"] == 2, stats
        rd.set_cache(None)
    # a typed tensor across the seams: no staging tensor, the gather converts out of slots and slab alike
    import out_spec_ref as R
    a, b = R.PAIRS[0]
    spec = mic.OutSpec("f32", affine=[(a, b)], pad=-3.0)
    xyz = [(-3, -2, 1), (40, 20, n - 3)]
    with mic.Mic2Reader(data) as rd, mic.FrameCache(w, h, 3) as cache:
        rd.set_cache(cache)
        for _ in range(2):
            buf = R.Buffer(len(xyz) * 4 * 18 * 30, "f32")
            st, stats = rd.read_crops(xyz, 30, 18, 4, buf.ptr, buf.nbytes, spec=spec)
            want = R.convert(V.expected(vol, xyz, 30, 18, 4), "f32", a, b, pad=-3.0, outside=FV.outside(vol, xyz, 30, 18, 4))
            assert np.array_equal(buf.bits().reshape(want.shape), want) and (st == 0).all()
        rd.set_cache(None)
print("mic2 frame cache seams ok")
