"""Typed output of the six MIC2 crop readers (csrc/mic_mic2_crops.hip, the _as doors).  Independent volumes gather straight into the
typed tensor; temporal volumes keep their running sums in a u16 staging tensor and one convert kernel writes the typed samples at the
end of the call.  The expected tensor is the host reference (out_spec_ref.py) applied to the zero-padded volumes, pad where the
coordinates lie outside the volume or the volume is refused; every comparison is array_equal on the raw bits."""
import numpy as np
import pytest

import mic2_multi_volumes as M
import out_spec_ref as R

pytestmark = pytest.mark.gpu

V = M.V
# (volume, temporal): an independent and a temporal volume of each depth in one call, and a refused one in the middle
ORDER = [("xr12", False), ("xr12", True), None, ("wrap16", True), ("wrap16", False)]
PAIRS = [R.PAIRS[0], R.PAIRS[2], R.PAIRS[4], R.PAIRS[1], R.PAIRS[3]]
SHAPES = [(17, 5, 4), (48, 40, 3)]       # crops that span more than one frame; odd and even row pitch


@pytest.fixture(scope="module")
def volumes(mic, synth, gpu_ready):
    out = {}
    for name, make in (("xr12", M.volume_12bit), ("wrap16", M.volume_16bit)):
        vol, maxv = make(synth)
        n, h, w = vol.shape
        files = {}
        for temporal in (False, True):
            data = mic.compress_multi_frame(vol, w, h, maxv, temporal=temporal)
            assert np.array_equal(mic.decompress_multi_frame(data), vol) and M.Mic2File(data).temporal == temporal
            files[temporal] = data
        vol.setflags(write=False)
        out[name] = dict(vol=vol, files=files)
    return out


def _listed(volumes):
    vols = [None if o is None else volumes[o[0]]["vol"] for o in ORDER]
    files = [b"garbage, and not a little of it" if o is None else volumes[o[0]]["files"][o[1]] for o in ORDER]
    return vols, files


class Doors:
    """the three many-volume entry points on one list of files: call(xyzv, cw, ch, cd, d_out, out_cap, spec)"""

    def __init__(self, mic, files):
        import torch
        ok = [bytes(f[:4]) == b"MIC2" for f in files]
        self.rds = [mic.Mic2Reader(f, len(f)) if ok[v] else None for v, f in enumerate(files)]
        self.sess = mic.Session(4, 150 * 70)
        self.keep = [torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy()).cuda() for f in files]
        heads = [M.Mic2File(f).head() if ok[v] else bytes(f) for v, f in enumerate(files)]
        ptrs, lens = [d.data_ptr() for d in self.keep], [len(f) for f in files]
        self.all = [("files", lambda q, cw, ch, cd, d, cap, spec: mic.mic2_multi_read_crops(files, q, cw, ch, cd, d, cap, spec=spec)),
                    ("readers", lambda q, cw, ch, cd, d, cap, spec: mic.mic2_readers_read_crops(self.rds, q, cw, ch, cd, d, cap, spec=spec)),
                    ("session", lambda q, cw, ch, cd, d, cap, spec: self.sess.mic2_multi_read_crops(heads, ptrs, lens, q, cw, ch, cd, d, cap, spec=spec))]

    def close(self):
        for r in self.rds:
            if r is not None:
                r.close()
        self.sess.close()


def _pad(dtype):
    return 3.0 if dtype in ("u8", "u16") else -3.0


def _outside(vol, xyz, cw, ch, cd):
    """(len(xyz), cd, ch, cw) bool: the sample lies outside the volume"""
    n, h, w = vol.shape
    out = np.zeros((len(xyz), cd, ch, cw), dtype=bool)
    for i, (x, y, z) in enumerate(xyz):
        xs, ys, zs = np.arange(x, x + cw), np.arange(y, y + ch), np.arange(z, z + cd)
        out[i] = ((zs < 0) | (zs >= n))[:, None, None] | ((ys < 0) | (ys >= h))[None, :, None] | ((xs < 0) | (xs >= w))[None, None, :]
    return out


def _expected_multi(vols, xyzv, cw, ch, cd, dtype, pairs):
    x = M.expected_multi(vols, xyzv, cw, ch, cd)
    outside = np.ones(x.shape, dtype=bool)                                  # (a refused volume's crops: all pad)
    a, b = np.ones(len(xyzv)), np.zeros(len(xyzv))
    for v, vol in enumerate(vols):
        idx, xyz = M.crops_of(xyzv, v)
        if vol is not None and idx:
            outside[idx] = _outside(vol, xyz, cw, ch, cd)
            a[idx], b[idx] = pairs[v]
    want = R.convert(x, dtype, a[:, None, None, None], b[:, None, None, None], pad=_pad(dtype), outside=outside)
    R.assert_no_subnormals(want, dtype)
    return want


@pytest.mark.parametrize("shape", SHAPES)
def test_one_pair_per_volume_independent_and_temporal_in_one_call(mic, volumes, shape):
    cw, ch, cd = shape
    vols, files = _listed(volumes)
    assert all(R.exact_pair(*p) for p in PAIRS) and len(set(PAIRS)) == len(PAIRS)
    per = [V.origins(150, 70, 11, cw, ch, cd) if v is None else V.origins(v.shape[2], v.shape[1], v.shape[0], cw, ch, cd) for v in vols]
    xyzv = M.interleave(per)
    vidx = np.array([q[3] for q in xyzv])
    doors = Doors(mic, files)
    try:
        for dtype in ("f32", "bf16", "f16", "u8"):
            want = _expected_multi(vols, xyzv, cw, ch, cd, dtype, PAIRS)
            spec = mic.OutSpec(dtype, affine=PAIRS, pad=_pad(dtype))
            for door, call in doors.all:
                buf = R.Buffer(len(xyzv) * cd * ch * cw, dtype)
                st, bad, stats = call(xyzv, cw, ch, cd, buf.ptr, buf.nbytes, spec)
                got = buf.bits().reshape(want.shape)
                for i in range(len(xyzv)):
                    assert np.array_equal(got[i], want[i]), (door, dtype, shape, xyzv[i])
                assert (st[vidx != 2] == mic.MIC_OK).all() and (bad == -1).all(), (door, st, bad)
                assert (st[vidx == 2] != mic.MIC_OK).all() and len(set(st[vidx == 2].tolist())) == 1, (door, st)
                assert stats["volumes_read"] == 4 and stats["slabs"] >= 1, (door, stats)
    finally:
        doors.close()


def _single_doors(mic, data):
    """the three one-volume entry points on one file: call(xyz, cw, ch, cd, d_out, out_cap, spec) -> (status, stats); and what to close"""
    import torch
    rd = mic.Mic2Reader(data, len(data))
    sess = mic.Session(4, 150 * 70)
    d_file = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    head = M.Mic2File(data).head()
    calls = [("file", lambda q, cw, ch, cd, d, cap, spec: mic.mic2_read_crops(data, q, cw, ch, cd, d, cap, spec=spec)),
             ("reader", lambda q, cw, ch, cd, d, cap, spec: rd.read_crops(q, cw, ch, cd, d, cap, spec=spec)),
             ("session", lambda q, cw, ch, cd, d, cap, spec: sess.mic2_read_crops(head, d_file.data_ptr(), len(data), q, cw, ch, cd, d, cap, spec=spec))]
    return calls, (rd, sess, d_file)


@pytest.mark.parametrize("temporal", [False, True])
def test_one_volume_doors(mic, volumes, temporal):
    """one pair, every typed dtype, on the three one-volume doors; a base two bytes off the dword; a misaligned base"""
    cw, ch, cd = 17, 5, 4
    vol, data = volumes["wrap16"]["vol"], volumes["wrap16"]["files"][temporal]
    xyz = V.origins(vol.shape[2], vol.shape[1], vol.shape[0], cw, ch, cd)
    pair = R.PAIRS[1]
    x, outside = V.expected(vol, xyz, cw, ch, cd), _outside(vol, xyz, cw, ch, cd)
    calls, keep = _single_doors(mic, data)
    try:
        for dtype in R.DTYPES:
            want = R.convert(x, dtype, *pair, pad=_pad(dtype), outside=outside)
            R.assert_no_subnormals(want, dtype)
            spec = mic.OutSpec(dtype, affine=[pair], pad=_pad(dtype))
            for door, call in calls:
                for skew in ((0, 2) if R.SAMPLE_BYTES[dtype] == 2 else (0,)):
                    buf = R.Buffer(x.size, dtype, skew=skew)
                    st, stats = call(xyz, cw, ch, cd, buf.ptr, buf.nbytes, spec)
                    assert np.array_equal(buf.bits().reshape(want.shape), want), (door, dtype, skew)
                    assert (st == 0).all() and stats["slabs"] >= 1
        for door, call in calls:
            buf = R.Buffer(x.size, "f32", skew=2)
            with pytest.raises(mic.MicError) as e:
                call(xyz, cw, ch, cd, buf.ptr, buf.nbytes, mic.OutSpec("f32"))
            assert e.value.code == mic.MIC_ERR_ARGS and buf.untouched(), door
    finally:
        keep[0].close()
        keep[1].close()


def test_native_spec_and_no_spec_are_the_native_doors(mic, volumes):
    cw, ch, cd = 48, 40, 3
    vols, files = _listed(volumes)
    per = [V.origins(150, 70, 11, cw, ch, cd)[:6] if v is None else V.origins(v.shape[2], v.shape[1], v.shape[0], cw, ch, cd) for v in vols]
    xyzv = M.interleave(per)
    want = M.expected_multi(vols, xyzv, cw, ch, cd)
    doors = Doors(mic, files)
    try:
        for door, call in doors.all:
            base = None
            for spec in (None, mic.OutSpec("native")):
                buf = R.Buffer(want.size, "u16")
                st, bad, stats = call(xyzv, cw, ch, cd, buf.ptr, buf.nbytes, spec)
                assert np.array_equal(buf.bits().reshape(want.shape), want), door
                base = base or (st.tolist(), bad.tolist(), stats)
                assert (st.tolist(), bad.tolist(), stats) == base, door
    finally:
        doors.close()
    for temporal in (False, True):
        vol, data = volumes["xr12"]["vol"], volumes["xr12"]["files"][temporal]
        xyz = V.origins(150, 70, 11, cw, ch, cd)
        want1 = V.expected(vol, xyz, cw, ch, cd)
        calls, keep = _single_doors(mic, data)
        try:
            for door, call in calls:
                base = None
                for spec in (None, mic.OutSpec("native")):
                    buf = R.Buffer(want1.size, "u16")
                    st, stats = call(xyz, cw, ch, cd, buf.ptr, buf.nbytes, spec)
                    assert np.array_equal(buf.bits().reshape(want1.shape), want1), (door, temporal)
                    base = base or (st.tolist(), stats)
                    assert (st.tolist(), stats) == base, (door, temporal)
        finally:
            keep[0].close()
            keep[1].close()


@pytest.mark.parametrize("temporal", [False, True])
def test_f16_overflow_is_inf(mic, volumes, temporal):
    """the 16-bit volume holds 65535 (and more samples past 65519) in frame 4; pair (1, 0): inf where torch's CPU cast gives inf"""
    vol, data = volumes["wrap16"]["vol"], volumes["wrap16"]["files"][temporal]
    zs, ys, xs = np.nonzero(vol == 65535)
    assert zs.size
    cw, ch, cd = 17, 5, 2
    xyz = [(int(x) - 8, int(y) - 2, int(z) - 1) for z, y, x in zip(zs, ys, xs)]
    x, outside = V.expected(vol, xyz, cw, ch, cd), _outside(vol, xyz, cw, ch, cd)
    want = R.convert(x, "f16", 1.0, 0.0, pad=-3.0, outside=outside)
    assert (want == 0x7C00).sum() >= zs.size and (want < 0x7C00).any()
    buf = R.Buffer(x.size, "f16")
    st, _ = mic.mic2_read_crops(data, xyz, cw, ch, cd, buf.ptr, buf.nbytes, spec=mic.OutSpec("f16", affine=[(1.0, 0.0)], pad=-3.0))
    assert np.array_equal(buf.bits().reshape(want.shape), want) and (st == 0).all()
