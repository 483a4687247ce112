"""Run by tests/test_gpu_wsi_scaled.py in a child process with MIC_HIP_WS_BUDGET_MB set small, so that the staging tensor of a scaled
patch call (a quarter of the ceiling at most) does not hold the source rectangles of all its patches: the call is cut into consecutive
patch groups, each one native call and one resample launch.  Every patch must still equal the host reference (scaled_ref.py);
stats.slabs sums over the groups, tiles_decoded and pieces stay the whole call's plan counts for the source extent."""
import importlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry
mic = entry.load_package()
import out_spec_ref as R
import scaled_ref as SR
import wsi_patch_slides as S

budget = int(os.environ.get("MIC_HIP_WS_BUDGET_MB", "0")) << 20
assert budget, "meant to run with a small workspace budget"
PAIRS = [(0.5, 3.0), (2.0, -100.0), (0.0625, -8.0)]
scale, (pw, ph) = (7, 3), (71, 37)
sw, sh = mic.wsi_scaled_extent(pw, ph, scale)

for fmt in ("rgb", "grey16"):
    img, data = S.make_file(mic, fmt)
    kw = S.fmt_args(fmt)
    C, spx = (3, 3) if fmt == "rgb" else (1, 2)
    xy = S.origins(S.W, S.H, S.TILE, S.TILE, sw, sh)
    xy = xy + [(x + 5, y + 3) for x, y in xy]
    per_group = max(1, budget // 4 // (sw * sh * spx))
    groups = -(-len(xy) // per_group)
    assert groups >= 2, (fmt, per_group, len(xy))
    want, outside = SR.resample(img, xy, pw, ph, *scale)
    tiles, pieces = mic.wsi_patch_plan(S.W, S.H, S.TILE, S.TILE, xy, sw, sh)
    rd = mic.WsiReader(data)
    sess = mic.Session(64, S.TILE * S.TILE)
    d_px = torch.from_numpy(np.ascontiguousarray(img).view(np.uint8).reshape(-1).copy()).cuda()
    sess.wsi_encode(d_px.data_ptr(), S.W, S.H, tile_w=S.TILE, tile_h=S.TILE, levels=S.LEVELS, **kw)
    q = [(x, y, 0, 0) for x, y in xy]
    doors = [("file", lambda *a, **k: mic.wsi_read_patches(data, 0, xy, *a, **k)), ("reader", lambda *a, **k: rd.read_patches(0, xy, *a, **k)),
             ("session", lambda *a, **k: sess.wsi_read_patches(0, xy, *a, **k)),
             ("files", lambda *a, **k: mic.wsi_multi_read_patches([data], q, *a, **kw, **k)),
             ("readers", lambda *a, **k: mic.wsi_readers_read_patches([rd], q, *a, **kw, **k))]
    pairs = PAIRS[:C]
    x = want.reshape(want.shape[:3] + (C,)).astype(np.uint16)
    pr = np.asarray(pairs, dtype=np.float64).reshape(1, 1, 1, C, 2)
    typed = R.convert(x, "bf16", pr[..., 0], pr[..., 1], pad=-3.0, outside=np.repeat(outside[..., None], C, axis=3))
    typed = np.ascontiguousarray(typed.transpose(0, 3, 1, 2)) if C == 3 else typed[..., 0]
    for door, call in doors:
        for spec, exp, dtype in [(None, np.ascontiguousarray(want).view(np.uint8).reshape(len(xy), -1), "u8"),
                                 (mic.OutSpec("bf16", channels_first=True, affine=pairs, pad=-3.0), typed.reshape(len(xy), -1), "bf16")]:
            buf = R.Buffer(exp.size, dtype)
            st, stats = call(pw, ph, buf.ptr, buf.nbytes, spec=spec, scale=scale)
            got = buf.bits().reshape(exp.shape)
            for i in range(len(xy)):
                assert np.array_equal(got[i], exp[i]), (fmt, door, dtype, xy[i])
            src = R.Buffer(len(xy) * sw * sh * spx, "u8")
            _, native = call(sw, sh, src.ptr, src.nbytes)                     # the same rectangles in one native call
            assert (st == 0).all() and stats["slabs"] >= groups and stats["slabs"] > native["slabs"], (fmt, door, stats, native, groups)
            assert stats["tiles_decoded"] == len(tiles) == native["tiles_decoded"] and stats["pieces"] == pieces == native["pieces"], (fmt, door, stats)
    rd.close(); sess.close()
print("scaled patch groups ok")
