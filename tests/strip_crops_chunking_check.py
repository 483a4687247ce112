"""Run by tests/test_gpu_strip_crops.py::test_sub_batch_seams_under_a_small_workspace in a child process with MIC_HIP_WS_BUDGET_MB set
small, so that the strip-file crop calls cut the planned strips into sub-batches of two: strips of different files, widths and
predictors then share a slab or fall on either side of a seam, and the pieces are gathered slab by slab.  Every crop must equal the
padded source image."""
import importlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry
mic = entry.load_package(); synth = importlib.import_module("medical_image_codec_amd.synth")
import strip_crop_files as F

assert os.environ.get("MIC_HIP_WS_BUDGET_MB"), "meant to run with a small workspace budget"
files = F.build(synth, lambda img, maxv, strips, states: mic.compress_parallel_strips(img, img.shape[1], img.shape[0], maxv, strips, states),
                lambda img, maxv, strips: mic.compress_parallel_strips_adaptive(img, img.shape[1], img.shape[0], maxv, strips))
datas = [d for _, _, d in files]
sess = mic.Session(4, 96 * 70)
d_files = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() for d in datas]
heads, ptrs, lens = [mic.strips_head(d) for d in datas], [t.data_ptr() for t in d_files], [len(d) for d in datas]
doors = [lambda *a: mic.strips_read_crops(datas, *a), lambda *a: sess.strips_read_crops(heads, ptrs, lens, *a)]
most = 0
for cw, ch in F.SHAPES:
    xyf = F.origins(files, cw, ch)
    want = F.expected(files, xyf, cw, ch)
    units, pieces, _ = mic.strips_crop_plan(datas, xyf, cw, ch)
    for k, door in enumerate(doors):
        t = torch.full((len(xyf), ch, cw, 2), 0xA5, dtype=torch.uint8, device="cuda")
        st, bad, stats = door(xyf, cw, ch, t.data_ptr(), t.numel())
        got = t.cpu().numpy().view("<u2")[..., 0]
        for i in range(len(xyf)):
            assert np.array_equal(got[i], want[i]), (k, (cw, ch), xyf[i])
        assert (st == 0).all() and stats["strips_decoded"] == len(units) and stats["pieces"] == pieces, (k, stats)
        assert stats["slabs"] == -(-len(units) // 2), (k, stats)            # two strips a sub-batch
        most = max(most, stats["slabs"])
assert most >= 3, most
# one crop inside one strip: one unit, one chain
t = torch.full((1, 4, 8, 2), 0xA5, dtype=torch.uint8, device="cuda")
st, bad, stats = mic.strips_read_crops(datas, [(30, 10, 0)], 8, 4, t.data_ptr(), t.numel())
assert np.array_equal(t.cpu().numpy().view("<u2")[..., 0], F.expected(files, [(30, 10, 0)], 8, 4)) and (st == 0).all()
assert (stats["strips_decoded"], stats["slabs"]) == (1, 1), stats
# Sub-batches whose largest pieces differ: the gather's grid y follows the largest piece of each sub-batch.  Crops of 65 x 64 over
# the five files and a sixth of one 96 x 70 strip: the first crop touches the first unit, strip 0 of A, in its corner pixel alone
# (a 1 x 1 piece, one row chunk), the last lies wholly inside the last unit (a 65 x 64 piece, two row chunks); B's and C's strips
# lie between them.
one = mic.compress_parallel_strips(files[0][1], 96, 70, 4095, 1, 2)
px, w, h = mic.decompress_parallel_strips(one)
assert (w, h) == (96, 70) and np.array_equal(np.asarray(px).reshape(70, 96), files[0][1])   # the whole-image decode is the source
files6, datas6 = files + [("F", files[0][1], bytes(one))], datas + [bytes(one)]
xyf = [(-64, -63, 0), (0, 0, 1), (20, 3, 2), (10, 3, 5)]
want = F.expected(files6, xyf, 65, 64)
assert np.count_nonzero(want[0]) <= 1 and want[0, 63, 64] == files[0][1][0, 0] and np.array_equal(want[3], files[0][1][3:67, 10:75])
units, pieces, _ = mic.strips_crop_plan(datas6, xyf, 65, 64)
assert len(units) >= 7 and tuple(units[0]) == (0, 0) and tuple(units[-1]) == (5, 0), units
d_one = torch.from_numpy(np.frombuffer(datas6[5], dtype=np.uint8).copy()).cuda()
for k, door in enumerate([lambda *a: mic.strips_read_crops(datas6, *a),
                          lambda *a: sess.strips_read_crops(heads + [mic.strips_head(datas6[5])], ptrs + [d_one.data_ptr()], lens + [len(datas6[5])], *a)]):
    t = torch.full((len(xyf), 64, 65, 2), 0xA5, dtype=torch.uint8, device="cuda")
    st, bad, stats = door(xyf, 65, 64, t.data_ptr(), t.numel())
    assert (st == 0).all() and stats["strips_decoded"] == len(units) and stats["pieces"] == pieces and stats["slabs"] >= 2, (k, stats)
    assert stats["slabs"] == -(-len(units) // 2), (k, stats)                # two strips a sub-batch: first and last unit apart
    assert np.array_equal(t.cpu().numpy().view("<u2")[..., 0], want), k
sess.close()
print("strip crop seams ok")
