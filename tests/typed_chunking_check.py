"""Run by tests/test_gpu_typed_chunking.py in a child process with MIC_HIP_WS_BUDGET_MB set small, so that the typed crop calls cut
their units into several sub-batches.  A temporal MIC2 volume's running sums then cross the seams inside the u16 staging tensor, and
the convert kernel writes the typed tensor behind the last sub-batch; strip files gather typed samples slab by slab.  Every crop must
equal the host reference (out_spec_ref.py) applied to the padded source."""
import importlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry
mic = entry.load_package(); synth = importlib.import_module("medical_image_codec_amd.synth")
import mic2_crop_volumes as V
import out_spec_ref as R
import strip_crop_files as F

assert os.environ.get("MIC_HIP_WS_BUDGET_MB"), "meant to run with a small workspace budget"
PAIR = R.PAIRS[2]
assert R.exact_pair(*PAIR)

# a temporal volume (and the independent one beside it): 11 frames, three a sub-batch
vol, maxv = V.volume_12bit(synth)
n, h, w = vol.shape
for temporal in (True, False):
    data = mic.compress_multi_frame(vol, w, h, maxv, temporal=temporal)
    assert np.array_equal(mic.decompress_multi_frame(data), vol)
    m = V.Mic2File(data)
    rd = mic.Mic2Reader(data)
    sess = mic.Session(4, w * h)
    d_file = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    doors = [lambda *a, **k: mic.mic2_read_crops(data, *a, **k), lambda *a, **k: rd.read_crops(*a, **k),
             lambda *a, **k: sess.mic2_read_crops(m.head(), d_file.data_ptr(), len(data), *a, **k)]
    for cw, ch, cd in [(48, 40, 3), (17, 5, 4)]:
        # the shared origins, and crops that start behind the first sub-batch, inside the second and the third; one spans three seams
        xyz = V.origins(w, h, n, cw, ch, cd) + [(9, 9, 4), (40, 20, 7), (3, 30, 9), (11, 2, 1)]
        x = V.expected(vol, xyz, cw, ch, cd)
        outside = np.zeros(x.shape, dtype=bool)
        for i, (cx, cy, cz) in enumerate(xyz):
            xs, ys, zs = np.arange(cx, cx + cw), np.arange(cy, cy + ch), np.arange(cz, cz + cd)
            outside[i] = ((zs < 0) | (zs >= n))[:, None, None] | ((ys < 0) | (ys >= h))[None, :, None] | ((xs < 0) | (xs >= w))[None, None, :]
        for dtype in ("f32", "bf16"):
            want = R.convert(x, dtype, *PAIR, pad=-3.0, outside=outside)
            R.assert_no_subnormals(want, dtype)
            spec = mic.OutSpec(dtype, affine=[PAIR], pad=-3.0)
            for k, door in enumerate(doors):
                buf = R.Buffer(x.size, dtype)
                st, stats = door(xyz, cw, ch, cd, buf.ptr, buf.nbytes, spec=spec)
                got = buf.bits().reshape(want.shape)
                for i in range(len(xyz)):
                    assert np.array_equal(got[i], want[i]), (temporal, dtype, k, (cw, ch, cd), xyz[i])
                assert (st == 0).all() and stats["slabs"] >= 3, (temporal, dtype, k, stats)
    rd.close(); sess.close()

# strip files: 23 strips of five files, a few a sub-batch
files = F.build(synth, lambda img, maxv, strips, states: mic.compress_parallel_strips(img, img.shape[1], img.shape[0], maxv, strips, states),
                lambda img, maxv, strips: mic.compress_parallel_strips_adaptive(img, img.shape[1], img.shape[0], maxv, strips))
datas = [d for _, _, d in files]
sess = mic.Session(4, 96 * 70)
d_files = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() for d in datas]
heads = [bytes(d[: F.StripFile(d).body]) for d in datas]
doors = [lambda *a, **k: mic.strips_read_crops(datas, *a, **k),
         lambda *a, **k: sess.strips_read_crops(heads, [t.data_ptr() for t in d_files], [len(d) for d in datas], *a, **k)]
for cw, ch in [(33, 9), (128, 80)]:
    xyf = F.origins(files, cw, ch)
    x = F.expected(files, xyf, cw, ch)
    outside = R.outside_mask(xyf, lambda i: files[xyf[i][2]][1].shape[1], lambda i: files[xyf[i][2]][1].shape[0], cw, ch)
    for dtype in ("f32", "bf16"):
        want = R.convert(x, dtype, *PAIR, pad=-3.0, outside=outside)
        R.assert_no_subnormals(want, dtype)
        spec = mic.OutSpec(dtype, affine=[PAIR], pad=-3.0)
        for k, door in enumerate(doors):
            buf = R.Buffer(x.size, dtype)
            st, bad, stats = door(xyf, cw, ch, buf.ptr, buf.nbytes, spec=spec)
            got = buf.bits().reshape(want.shape)
            for i in range(len(xyf)):
                assert np.array_equal(got[i], want[i]), (dtype, k, (cw, ch), xyf[i])
            assert (st == 0).all() and stats["slabs"] >= 3, (dtype, k, stats)
sess.close()
print("typed crop seams ok")
