"""mic_hip_mic2_crop_plan (csrc/mic_mic2_crops.hip), the host planner behind the MIC2 crop calls, against a plan made by enumerating
every crop's coordinates in numpy.  No device is needed."""
import ctypes as C

import numpy as np
import pytest

import mic2_crop_volumes as V

W, H, N = 150, 70, 11


@pytest.mark.parametrize("temporal", [False, True])
@pytest.mark.parametrize("shape", V.SHAPES)
def test_plan_equals_the_enumerated_one(mic, temporal, shape):
    cw, ch, cd = shape
    xyz = V.origins(W, H, N, cw, ch, cd)
    frames, pieces = mic.mic2_crop_plan(W, H, N, temporal, xyz, cw, ch, cd)
    want_frames, want_pieces = V.brute_plan(W, H, N, temporal, xyz, cw, ch, cd)
    assert frames.tolist() == want_frames and pieces == want_pieces and pieces > 0
    assert frames.dtype == np.uint32
    for o in xyz:                                                         # ... and crop by crop
        f1, p1 = mic.mic2_crop_plan(W, H, N, temporal, [o], cw, ch, cd)
        assert (f1.tolist(), p1) == V.brute_plan(W, H, N, temporal, [o], cw, ch, cd), o


def test_faces_outside_duplicates_and_nothing(mic):
    plan = lambda t, xyz, s: (lambda f, p: (f.tolist(), p))(*mic.mic2_crop_plan(W, H, N, t, xyz, *s))
    for t in (False, True):
        assert plan(t, [], (48, 40, 3)) == ([], 0)                        # n = 0
        for o in [(W, 0, 0), (-48, 0, 0), (0, H, 0), (0, -40, 0), (0, 0, N), (0, 0, N + 5), (0, 0, -3), (0, 0, -9)]:
            assert plan(t, [o], (48, 40, 3)) == ([], 0), o               # wholly outside: nothing to decode
        assert plan(t, [(0, 0, 0)], (W, H, N)) == (list(range(N)), N)     # the whole volume
        assert plan(t, [(-1, -1, -1)], (W + 2, H + 2, N + 2)) == (list(range(N)), N)
        assert plan(t, [(W - 1, H - 1, N - 1)], (1, 1, 1)) == ([N - 1] if not t else list(range(N)), 1)
        assert plan(t, [(W - 1, H - 1, N - 1)], (5, 5, 5)) == ([N - 1] if not t else list(range(N)), 1)
    assert plan(False, [(3, 3, 4)] * 3, (17, 5, 4)) == ([4, 5, 6, 7], 12)  # duplicates: each frame once, every piece counted
    assert plan(True, [(3, 3, 4)] * 3, (17, 5, 4)) == (list(range(8)), 12)
    assert plan(False, [(0, 0, 8), (0, 0, -2)], (1, 1, 4)) == ([0, 1, 8, 9, 10], 5)
    assert plan(True, [(0, 0, 8), (0, 0, -2)], (1, 1, 4)) == (list(range(11)), 5)   # temporal: 0 .. the last overlapped frame


def test_a_short_frame_list_is_a_capacity_error_with_the_counts(mic):
    xyz = [(0, 0, 2), (5, 5, 6)]
    for t, want in ((False, 6), (True, 9)):
        with pytest.raises(mic.MicError) as e:
            mic.mic2_crop_plan(W, H, N, t, xyz, 17, 5, 3, cap=want - 1)
        assert e.value.code == mic.MIC_ERR_CAPACITY and e.value.nframes == want and e.value.pieces == 6
        frames, pieces = mic.mic2_crop_plan(W, H, N, t, xyz, 17, 5, 3, cap=want)
        assert frames.size == want and pieces == 6
    # the list is left alone when it is too short
    a = np.asarray(xyz, dtype=np.int32)
    out = np.full(4, 77, dtype=np.uint32)
    nf, npc = C.c_uint64(0), C.c_uint64(0)
    rc = mic.lib().mic_hip_mic2_crop_plan(W, H, N, 0, a.ctypes.data, 2, 17, 5, 3, out.ctypes.data, 4, C.byref(nf), C.byref(npc))
    assert rc == mic.MIC_ERR_CAPACITY and (out == 77).all() and (nf.value, npc.value) == (6, 6)


def test_argument_errors(mic):
    a = np.asarray([(0, 0, 0)], dtype=np.int32)
    out = np.zeros(16, dtype=np.uint32)
    nf, npc = C.c_uint64(0), C.c_uint64(0)

    def call(w=W, h=H, n_frames=N, xyz=a.ctypes.data, n=1, cw=8, ch=8, cd=2, frames=out.ctypes.data, cap=16):
        return mic.lib().mic_hip_mic2_crop_plan(w, h, n_frames, 0, xyz, n, cw, ch, cd, frames, cap, C.byref(nf), C.byref(npc))
    assert call() == mic.MIC_OK and (nf.value, npc.value) == (2, 2)
    for kw in (dict(cw=0), dict(ch=0), dict(cd=0), dict(cd=-1), dict(cw=-4), dict(n=-1), dict(w=0), dict(h=-1), dict(n_frames=-1),
               dict(xyz=None), dict(frames=None)):
        assert call(**kw) == mic.MIC_ERR_ARGS, kw
    assert call(xyz=None, n=0) == mic.MIC_OK and (nf.value, npc.value) == (0, 0)
    assert call(frames=None, cap=0) == mic.MIC_ERR_CAPACITY and (nf.value, npc.value) == (2, 2)   # counting only
