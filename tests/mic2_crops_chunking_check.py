"""Run by tests/test_gpu_mic2_crops.py::test_sub_batch_seams_under_a_small_workspace in a child process with MIC_HIP_WS_BUDGET_MB set
small, so that the MIC2 crop calls cut the frames into sub-batches of three: the temporal sum's carry then crosses the seams inside
the crop tensor, and an independent file's pieces are gathered slab by slab, each from its frame's slot in the slab.  Every crop must
equal the padded source volume.  Last, a temporal file with a frame that fails: the call stops behind the sub-batch that holds it."""
import importlib, os, struct, sys
import numpy as np
import pytest
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry
mic = entry.load_package(); synth = importlib.import_module("medical_image_codec_amd.synth")
import mic2_crop_volumes as V

assert os.environ.get("MIC_HIP_WS_BUDGET_MB"), "meant to run with a small workspace budget"
vol, maxv = V.volume_12bit(synth)
n, h, w = vol.shape
for temporal in (True, False):
    data = mic.compress_multi_frame(vol, w, h, maxv, temporal=temporal)
    assert np.array_equal(mic.decompress_multi_frame(data), vol)
    m = V.Mic2File(data)
    rd = mic.Mic2Reader(data)
    sess = mic.Session(4, w * h)
    d_file = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    doors = [lambda *a: mic.mic2_read_crops(data, *a), lambda *a: rd.read_crops(*a),
             lambda *a: sess.mic2_read_crops(m.head(), d_file.data_ptr(), len(data), *a)]
    for cw, ch, cd in V.SHAPES:
        # the shared origins hold crops with z < 0; these start behind the first sub-batch, inside the second and the third, and one
        # spans three seams
        xyz = V.origins(w, h, n, cw, ch, cd) + [(9, 9, 4), (40, 20, 7), (3, 30, 9), (11, 2, 1)]
        want = V.expected(vol, xyz, cw, ch, cd)
        frames, pieces = mic.mic2_crop_plan(w, h, n, temporal, xyz, cw, ch, cd)
        for k, door in enumerate(doors):
            t = torch.full((len(xyz), cd, ch, cw, 2), 0xA5, dtype=torch.uint8, device="cuda")
            st, stats = door(xyz, cw, ch, cd, t.data_ptr(), t.numel())
            got = t.cpu().numpy().view("<u2")[..., 0]
            for i in range(len(xyz)):
                assert np.array_equal(got[i], want[i]), (temporal, k, (cw, ch, cd), xyz[i])
            assert (st == 0).all() and stats["frames_decoded"] == frames.size and stats["pieces"] == pieces, (temporal, k, stats)
            assert stats["slabs"] == -(-frames.size // 3) >= 3, (temporal, k, stats)     # three frames a sub-batch
    # the slot of a frame in its sub-batch's slab, at the smallest seam: every frame is decoded, so plan index = frame and the
    # sub-batches are frames 0-2, 3-5, 6-8, 9-10.  One crop lies wholly inside the last sub-batch, one spans the first seam; a frame
    # is its neighbour rolled by 3 columns, so a wrong slot shows as a wrong frame
    cw, ch, cd = 48, 40, 2
    xyz = [(3 * z, z, z) for z in range(0, n - 1, 2)] + [(30, 10, 9), (60, 20, 2)]
    want = V.expected(vol, xyz, cw, ch, cd)
    assert not np.array_equal(want[-2][0], want[-2][1]) and not np.array_equal(want[-1][0], want[-1][1])
    frames, pieces = mic.mic2_crop_plan(w, h, n, temporal, xyz, cw, ch, cd)
    assert frames.tolist() == list(range(n))
    for k, door in enumerate(doors):
        t = torch.full((len(xyz), cd, ch, cw, 2), 0xA5, dtype=torch.uint8, device="cuda")
        st, stats = door(xyz, cw, ch, cd, t.data_ptr(), t.numel())
        got = t.cpu().numpy().view("<u2")[..., 0]
        for i in range(len(xyz)):
            assert np.array_equal(got[i], want[i]), (temporal, k, xyz[i])
        assert (st == 0).all() and stats["pieces"] == pieces and stats["slabs"] == 4, (temporal, k, stats)
    # a crop deep in the stack alone: a temporal file still sums from frame 0, an independent one decodes its own frames only
    t = torch.full((1, 2, 40, 48, 2), 0xA5, dtype=torch.uint8, device="cuda")
    st, stats = mic.mic2_read_crops(data, [(30, 10, 8)], 48, 40, 2, t.data_ptr(), t.numel())
    assert np.array_equal(t.cpu().numpy().view("<u2")[..., 0], V.expected(vol, [(30, 10, 8)], 48, 40, 2)) and (st == 0).all()
    assert (stats["frames_decoded"], stats["slabs"]) == ((10, 4) if temporal else (2, 1)), stats
    if temporal:
        # frame 5 fails: its table entry points at a well-formed residual stream of a 150 x 69 frame, appended to the file, which
        # expands to the wrong number of symbols (multiframecompress.go:170-172).  The sub-batches of frames 0-2 and 3-5 run and the
        # call stops there (`slabs` counts the chains that ran); crops that end in front of frame 5 are exact, the others carry the
        # code decompress_multi_frame gives
        short = V.Mic2File(mic.compress_multi_frame(np.ascontiguousarray(vol[:, : h - 1]), w, h - 1, maxv, temporal=True))
        b, e = short.span(5)
        md = V.Mic2File(data)
        struct.pack_into("<II", md.data, 20 + 8 * 5, len(md.data) - md.body, e - b)
        bad = bytes(md.data + short.data[b:e])
        with pytest.raises(mic.MicError) as err:
            mic.decompress_multi_frame(bad)
        code = err.value.code
        assert code == mic.MIC_ERR_CORRUPT
        xyz = [(30, 10, 0), (60, 20, 2), (30, 10, 4), (30, 10, 8)]            # last frames 1, 3, 5, 9
        want = V.expected(vol, xyz, 48, 40, 2)
        rd2 = mic.Mic2Reader(bad)
        for k, door in enumerate([lambda *a: mic.mic2_read_crops(bad, *a), lambda *a: rd2.read_crops(*a)]):
            t = torch.full((len(xyz), 2, 40, 48, 2), 0xA5, dtype=torch.uint8, device="cuda")
            st, stats = door(xyz, 48, 40, 2, t.data_ptr(), t.numel())
            got = t.cpu().numpy().view("<u2")[..., 0]
            assert st.tolist() == [0, 0, code, code], (k, st, code)
            assert np.array_equal(got[:2], want[:2]), k
            assert (stats["frames_decoded"], stats["slabs"]) == (10, 2), (k, stats)
        rd2.close()
    rd.close(); sess.close()
print("mic2 crop seams ok")
