"""Run by tests/test_gpu_mic2_multi_crops.py::test_sub_batch_seams_under_a_small_workspace in a child process with
MIC_HIP_WS_BUDGET_MB set small, so that the MIC2 crop calls over many volumes cut their units into sub-batches of two or three.  The
cut rule is restated here (mic2_multi_volumes.cuts_of) and `slabs` must equal it; from the restated cuts the script asserts that a
cut falls (a) inside a temporal volume before a crop's first frame -- the carry is parked in slice(zf) --, (b) inside a temporal
volume within a crop's z range, (c) right behind a temporal volume's frame 0, and (d) that one sub-batch holds the tail of a
temporal volume, all of an independent volume and the head of the next temporal volume.  Every crop must equal the padded source;
then the run is repeated with frame 5 of the first temporal volume damaged."""
import importlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry
mic = entry.load_package(); synth = importlib.import_module("medical_image_codec_amd.synth")
import mic2_multi_volumes as M

budget = int(os.environ.get("MIC_HIP_WS_BUDGET_MB", "0")) << 20
assert budget, "meant to run with a small workspace budget"
cw, ch, cd = 48, 40, 3
# (volume, temporal, crops): the first temporal volume's crops reach frame 9, so ten of its units go three to a sub-batch and the
# tenth shares one with the one-frame independent volume and frame 0 of the narrow temporal volume
made = {k: f(synth) for k, f in (("xr12", M.volume_12bit), ("wrap16", M.volume_16bit), ("narrow", M.volume_narrow), ("tiny", M.volume_tiny))}
order = [("xr12", True, [(20, 10, 2), (9, 9, 4), (40, 20, 7), (-5, 10, -1), (3, 30, 0), (110, 40, 5), (60, -3, 6)]),
         ("tiny", False, [(0, 0, 0), (-3, -2, -1)]),
         ("narrow", True, [(0, 0, 0), (-10, -30, 1), (30, 5, 2)]),
         ("wrap16", True, [(20, 10, 2), (0, 0, 0), (140, 80, 3), (33, 21, 4)]),
         ("xr12", False, [(20, 10, 2), (0, 0, 0), (9, 9, 4), (40, 20, 8), (3, 30, 9)]),
         ("tiny", True, [(0, 0, 0)]),
         ("wrap16", False, [(5, 5, 1), (100, 60, 4)])]
vols = [made[k][0] for k, _, _ in order]
files = []
for k, temporal, _ in order:
    vol, maxv = made[k]
    data = mic.compress_multi_frame(vol, vol.shape[2], vol.shape[1], maxv, temporal=temporal)
    assert np.array_equal(mic.decompress_multi_frame(data), vol)
    files.append(data)
xyzv = M.interleave([c for _, _, c in order])
want = M.expected_multi(vols, xyzv, cw, ch, cd)
units, pieces, fs = mic.mic2_multi_crop_plan(files, xyzv, cw, ch, cd)
assert (fs == 0).all()
units = [tuple(u) for u in units.tolist()]
px = [vols[v].shape[1] * vols[v].shape[2] for v, f in units]
cuts = M.cuts_of(px, budget)
sizes = [b - a for a, b in zip(cuts, cuts[1:])]
assert set(sizes) <= {1, 2, 3} and 2 in sizes and 3 in sizes, sizes       # two or three frames a sub-batch

# where the restated cuts fall
temporal_of = [t for _, t, _ in order]
frames_of = lambda v: [f for vv, f in units if vv == v]


def zrange(v):
    """(first, last) frame inside volume v of each of its crops (every one of them overlaps it)"""
    n, h, w = vols[v].shape
    out = []
    for x, y, z in M.crops_of(xyzv, v)[1]:
        assert x < w and x + cw > 0 and y < h and y + ch > 0 and max(z, 0) <= min(z + cd, n) - 1
        out.append((max(z, 0), min(z + cd, n) - 1))
    return out


seen = set()
for c in cuts[1:-1]:
    v, f = units[c]
    if temporal_of[v] and units[c - 1][0] == v:                           # the cut lies inside temporal volume v, in front of its frame f
        seen |= {"a"} if any(zf >= f for zf, k in zrange(v)) else set()
        seen |= {"b"} if any(zf < f <= k for zf, k in zrange(v)) else set()
        seen |= {"c"} if f == 1 else set()
for a, b in zip(cuts, cuts[1:]):
    groups = []                                                           # the sub-batch's runs of one volume: (volume, its frames here)
    for v, f in units[a:b]:
        if groups and groups[-1][0] == v:
            groups[-1][1].append(f)
        else:
            groups.append((v, [f]))
    for (l, lf), (i, fi), (r, rf) in zip(groups, groups[1:], groups[2:]):
        tail = temporal_of[l] and lf[0] > 0 and lf[-1] == frames_of(l)[-1]
        head = temporal_of[r] and rf[0] == 0 and rf[-1] < frames_of(r)[-1]
        if tail and head and not temporal_of[i] and fi == frames_of(i):
            seen.add("d")
assert seen == {"a", "b", "c", "d"}, (seen, cuts, units)


def run(files, want, expect_status):
    rds = [mic.Mic2Reader(f) for f in files]
    sess = mic.Session(4, 150 * 70)
    d_files = [torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy()).cuda() for f in files]
    heads = [M.Mic2File(f).head() for f in files]
    doors = [lambda *a: mic.mic2_multi_read_crops(files, *a), lambda *a: mic.mic2_readers_read_crops(rds, *a),
             lambda *a: sess.mic2_multi_read_crops(heads, [d.data_ptr() for d in d_files], [len(f) for f in files], *a)]
    for k, door in enumerate(doors):
        t = torch.full((len(xyzv), cd, ch, cw, 2), 0xA5, dtype=torch.uint8, device="cuda")
        st, bad, stats = door(xyzv, cw, ch, cd, t.data_ptr(), t.numel())
        got = t.cpu().numpy().view("<u2")[..., 0]
        assert stats == dict(frames_decoded=len(units), pieces=pieces, slabs=len(cuts) - 1, volumes_read=len(files)), (k, stats, cuts)
        for i, c in enumerate(xyzv):
            code, frame = expect_status(c)
            assert (st[i], bad[i]) == (code, frame), (k, c, st[i], bad[i])
            if code == 0:
                assert np.array_equal(got[i], want[i]), (k, c)
    for r in rds:
        r.close()
    sess.close()


run(files, want, lambda c: (0, -1))

# frame 5 of the first temporal volume damaged: its dependants fail, everything else -- volumes decoded in later sub-batches
# included -- is exact
m = M.Mic2File(files[0])
b, e = m.span(5)
m.data[(b + e) // 2] ^= 0x5A
damaged = bytes(m.data)
try:
    code, dec = mic.MIC_OK, np.asarray(mic.decompress_multi_frame(damaged)).reshape(vols[0].shape)
except mic.MicError as err:
    code, dec = err.code, None
want2 = want if dec is None else M.expected_multi([dec] + vols[1:], xyzv, cw, ch, cd)
last = {tuple(c): k for c, (zf, k) in zip(M.crops_of(xyzv, 0)[1], zrange(0))}
assert len(last) == len(order[0][2]) and 0 < sum(k >= 5 for k in last.values()) < len(last)
assert any(units[c][0] > 0 for c in cuts[1:-1])                           # (volumes behind it start in later sub-batches)
run([damaged] + files[1:], want2, lambda c: (code, 5) if c[3] == 0 and code and last[tuple(c[:3])] >= 5 else (0, -1))

# Sub-batches whose largest pieces differ: the gather's grid y follows the largest piece of each sub-batch.  Independent volumes
# only (temporal ones are not gathered), crops of 65 x 64: such a piece takes two row chunks, the 1 x 1 and 25 x 4 pieces of the
# first sub-batch one.  The first crop touches the first unit -- the 7 x 35 frame -- in its corner pixel alone, the last one lies
# wholly inside the last unit, frame 5 of the 160 x 96 volume.
names = ["tiny", "narrow", "xr12", "wrap16"]
vols2 = [made[k][0] for k in names]
files2 = [mic.compress_multi_frame(v, v.shape[2], v.shape[1], made[k][1], temporal=False) for k, v in zip(names, vols2)]
for f, v in zip(files2, vols2):
    assert np.array_equal(mic.decompress_multi_frame(f), v)                # the whole-volume decode is the source
xyzv2 = [(-64, -63, 0, 0), (-40, -60, 0, 1), (10, 3, 0, 2), (10, 3, 3, 2), (20, 10, 3, 3)]
want3 = M.expected_multi(vols2, xyzv2, 65, 64, 3)
assert np.count_nonzero(want3[0]) <= 1 and want3[0, 0, 63, 64] == vols2[0][0, 0, 0] and (want3[4] == vols2[3][3:6, 10:74, 20:85]).all()
units2, pieces2, _ = mic.mic2_multi_crop_plan(files2, xyzv2, 65, 64, 3)
units2 = [tuple(u) for u in units2.tolist()]
assert len(units2) == 13 and units2[0] == (0, 0) and units2[-1] == (3, 5)
cuts2 = M.cuts_of([vols2[v].shape[1] * vols2[v].shape[2] for v, f in units2], budget)
assert cuts2[1] <= 4 and len(cuts2) - 1 >= 2, cuts2                        # the first sub-batch ends before the large frames' pieces
sess = mic.Session(4, 160 * 96)
d_files2 = [torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy()).cuda() for f in files2]
for k, door in enumerate([lambda *a: mic.mic2_multi_read_crops(files2, *a),
                          lambda *a: sess.mic2_multi_read_crops([M.Mic2File(f).head() for f in files2], [d.data_ptr() for d in d_files2], [len(f) for f in files2], *a)]):
    t = torch.full((len(xyzv2), 3, 64, 65, 2), 0xA5, dtype=torch.uint8, device="cuda")
    st, bad, stats = door(xyzv2, 65, 64, 3, t.data_ptr(), t.numel())
    assert (st == 0).all() and stats["slabs"] == len(cuts2) - 1 and stats["slabs"] >= 2 and stats["pieces"] == pieces2, (k, stats)
    assert np.array_equal(t.cpu().numpy().view("<u2")[..., 0], want3), k
sess.close()
print("mic2 multi crop seams ok")
