"""Typed output of the five MIC3 patch readers (csrc/mic_api_ext.hip, the _as doors; the kernels: csrc/mic_gather.hip).  RGB slides go
through the YCoCg-R inverse and then each channel through its own pair, into an interleaved or a channels-first tensor; greyscale
slides, 16-bit and 8-bit, are one-plane sources like the others.  The expected tensor is the host reference (out_spec_ref.py) applied
to decompress_wsi_level's image, padded and cropped in numpy; every comparison is array_equal on the raw bits."""
import numpy as np
import pytest

import out_spec_ref as R
import wsi_multi_slides as M
import wsi_patch_slides as S

pytestmark = pytest.mark.gpu

CHANNEL_PAIRS = [(0.5, 3.0), (2.0, -100.0), (0.0625, -8.0)]      # r: ties for u8; g: passes both ends of u8; b: negative below 128
PATCHES = [(24, 20), (71, 37)]                                   # (pw, ph): even and odd row pitch; the second spans four tiles


@pytest.fixture(scope="module")
def sets(mic, gpu_ready):
    """fmt -> dict(files = [A, B], levels = [[level image per level] per slide])"""
    out = {}
    for fmt in S.FORMATS:
        files = [M.device_file(mic, name, fmt) for name in ("A", "B")]
        levels = [[mic.decompress_wsi_level(d, l) for l in range(S.Mic3File(d).nlev)] for d in files]
        for name, lv in zip(("A", "B"), levels):
            assert np.array_equal(lv[0], M.image(name, fmt)), (fmt, name)
        out[fmt] = dict(files=files, levels=levels)
    return out


def _pad(dtype):
    return 3.0 if dtype in ("u8", "u16") else -3.0


def _expected(level_of, q, pw, ph, dtype, pair_of, channels_first):
    """q: (x, y, ...) per patch; level_of(i): patch i's level image or None (all pad); pair_of(i): (C, 2) pairs of patch i"""
    first = next(level_of(i) for i in range(len(q)) if level_of(i) is not None)
    C = first.shape[2] if first.ndim == 3 else 1
    x = np.zeros((len(q), ph, pw, C), dtype=np.uint16)
    outside = np.ones((len(q), ph, pw, C), dtype=bool)
    a, b = np.ones((len(q), 1, 1, C)), np.zeros((len(q), 1, 1, C))
    for i, p in enumerate(q):
        img = level_of(i)
        if img is None:
            continue
        x[i] = S.expected(img, [(p[0], p[1])], pw, ph)[0].reshape(ph, pw, C)
        outside[i] = R.outside_mask([p], lambda _: img.shape[1], lambda _: img.shape[0], pw, ph)[0][..., None]
        pr = np.asarray(pair_of(i), dtype=np.float64).reshape(-1, 2)
        a[i, 0, 0, :], b[i, 0, 0, :] = pr[:, 0], pr[:, 1]
    want = R.convert(x, dtype, a, b, pad=_pad(dtype), outside=outside)
    R.assert_no_subnormals(want, dtype)
    if C == 1:
        return want[..., 0]
    return np.ascontiguousarray(want.transpose(0, 3, 1, 2)) if channels_first else want


def _one_slide_doors(mic, img, data, fmt):
    import torch
    rd = mic.WsiReader(data)
    sess = mic.Session(64, S.TILE * S.TILE)
    d_px = torch.from_numpy(np.ascontiguousarray(img).view(np.uint8).reshape(-1).copy()).cuda()
    sess.wsi_encode(d_px.data_ptr(), S.W, S.H, tile_w=S.TILE, tile_h=S.TILE, levels=S.LEVELS, **S.fmt_args(fmt))
    calls = [("file", lambda lv, xy, pw, ph, d, cap, spec: mic.wsi_read_patches(data, lv, xy, pw, ph, d, cap, spec=spec)),
             ("reader", lambda lv, xy, pw, ph, d, cap, spec: rd.read_patches(lv, xy, pw, ph, d, cap, spec=spec)),
             ("session", lambda lv, xy, pw, ph, d, cap, spec: sess.wsi_read_patches(lv, xy, pw, ph, d, cap, spec=spec))]
    return calls, (rd, sess)


@pytest.mark.parametrize("channels_first", [False, True])
def test_rgb_one_slide_through_file_reader_and_session(mic, sets, channels_first):
    st_ = sets["rgb"]
    assert all(R.exact_pair(*p) for p in CHANNEL_PAIRS)
    calls, keep = _one_slide_doors(mic, st_["levels"][0][0], st_["files"][0], "rgb")
    try:
        for level in (0, 1):
            img = st_["levels"][0][level]
            for pw, ph in PATCHES:
                xy = S.origins(img.shape[1], img.shape[0], S.TILE, S.TILE, pw, ph)      # (patches that overhang: pad in all three planes)
                for dtype in ("f32", "bf16", "u8"):
                    want = _expected(lambda i: img, xy, pw, ph, dtype, lambda i: CHANNEL_PAIRS, channels_first)
                    spec = mic.OutSpec(dtype, channels_first=channels_first, affine=CHANNEL_PAIRS, pad=_pad(dtype))
                    assert spec.shape(len(xy), ph, pw, channels=3) == want.shape
                    for door, call in calls:
                        buf = R.Buffer(want.size, dtype)
                        st, stats = call(level, xy, pw, ph, buf.ptr, buf.nbytes, spec)
                        got = buf.bits().reshape(want.shape)
                        for i in range(len(xy)):
                            assert np.array_equal(got[i], want[i]), (door, dtype, level, pw, ph, xy[i])
                        assert (st == 0).all() and stats["slabs"] >= 1
        for door, call in calls:                                                         # a misaligned base, a short tensor
            buf = R.Buffer(2 * 20 * 24 * 3, "bf16", skew=1)
            with pytest.raises(mic.MicError) as e:
                call(0, [(0, 0), (5, 5)], 24, 20, buf.ptr, buf.nbytes, mic.OutSpec("bf16", channels_first=channels_first))
            assert e.value.code == mic.MIC_ERR_ARGS and buf.untouched(), door
            buf = R.Buffer(2 * 20 * 24 * 3, "f32")
            with pytest.raises(mic.MicError) as e:
                call(0, [(0, 0), (5, 5)], 24, 20, buf.ptr, buf.nbytes - 4, mic.OutSpec("f32", channels_first=channels_first))
            assert e.value.code == mic.MIC_ERR_CAPACITY and buf.untouched(), door
    finally:
        keep[0].close()
        keep[1].close()


def _multi_doors(mic, files, fmt):
    rds = [mic.WsiReader(d) for d in files]
    kw = S.fmt_args(fmt)
    calls = [("files", lambda q, pw, ph, d, cap, spec: mic.wsi_multi_read_patches(files, q, pw, ph, d, cap, spec=spec, **kw)),
             ("readers", lambda q, pw, ph, d, cap, spec: mic.wsi_readers_read_patches(rds, q, pw, ph, d, cap, spec=spec, **kw))]
    return calls, rds


@pytest.mark.parametrize("channels_first", [False, True])
def test_rgb_two_slides_with_a_pair_per_slide_and_channel(mic, sets, channels_first):
    st_ = sets["rgb"]
    pairs = R.PAIRS[:6]                                                     # slide 0: r, g, b; slide 1: r, g, b
    assert all(R.exact_pair(*p) for p in pairs) and len(set(pairs)) == 6
    parsed = [S.Mic3File(d) for d in st_["files"]]
    calls, rds = _multi_doors(mic, st_["files"], "rgb")
    try:
        for pw, ph in PATCHES:
            q = M.patch_list(parsed, pw, ph) + [(3, 2, 0, 5), (0, 0, 1, -1)]            # ... and two patches at levels their slides lack
            level_of = lambda i: st_["levels"][q[i][2]][q[i][3]] if 0 <= q[i][3] < len(st_["levels"][q[i][2]]) else None
            for dtype in ("f32", "bf16", "u8"):
                want = _expected(level_of, q, pw, ph, dtype, lambda i: pairs[3 * q[i][2]: 3 * q[i][2] + 3], channels_first)
                spec = mic.OutSpec(dtype, channels_first=channels_first, affine=pairs, pad=_pad(dtype))
                for door, call in calls:
                    buf = R.Buffer(want.size, dtype)
                    st, stats = call(q, pw, ph, buf.ptr, buf.nbytes, spec)
                    got = buf.bits().reshape(want.shape)
                    for i in range(len(q)):
                        assert np.array_equal(got[i], want[i]), (door, dtype, pw, ph, q[i])
                    assert (st[:-2] == 0).all() and (st[-2:] == mic.MIC_ERR_ARGS).all() and stats["slides_read"] == 2, (door, st)
    finally:
        for r in rds:
            r.close()


@pytest.mark.parametrize("fmt", ["grey16", "grey8"])
def test_greyscale_slides_to_f16(mic, sets, fmt):
    st_ = sets[fmt]
    pair = R.PAIRS[2] if fmt == "grey16" else R.PAIRS[4]
    pw, ph = 71, 37
    calls, keep = _one_slide_doors(mic, st_["levels"][0][0], st_["files"][0], fmt)
    mcalls, rds = _multi_doors(mic, st_["files"], fmt)
    try:
        img = st_["levels"][0][0]
        xy = S.origins(img.shape[1], img.shape[0], S.TILE, S.TILE, pw, ph)
        want = _expected(lambda i: img, xy, pw, ph, "f16", lambda i: [pair], False)
        spec = mic.OutSpec("f16", affine=[pair], pad=-3.0)
        for door, call in calls:
            for skew in (0, 2):
                buf = R.Buffer(want.size, "f16", skew=skew)
                st, _ = call(0, xy, pw, ph, buf.ptr, buf.nbytes, spec)
                assert np.array_equal(buf.bits().reshape(want.shape), want) and (st == 0).all(), (door, fmt, skew)
        parsed = [S.Mic3File(d) for d in st_["files"]]
        q = M.patch_list(parsed, pw, ph)
        two = [pair, R.PAIRS[3]]
        want = _expected(lambda i: st_["levels"][q[i][2]][q[i][3]], q, pw, ph, "f16", lambda i: [two[q[i][2]]], False)
        for door, call in mcalls:
            buf = R.Buffer(want.size, "f16")
            st, _ = call(q, pw, ph, buf.ptr, buf.nbytes, mic.OutSpec("f16", affine=two, pad=-3.0))
            assert np.array_equal(buf.bits().reshape(want.shape), want) and (st == 0).all(), (door, fmt)
    finally:
        keep[0].close()
        keep[1].close()
        for r in rds:
            r.close()


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_native_spec_and_no_spec_are_the_native_doors(mic, sets, fmt):
    st_ = sets[fmt]
    pw, ph = 71, 37
    bpp = 3 if fmt == "rgb" else 2 if fmt == "grey16" else 1
    img = st_["levels"][0][0]
    xy = S.origins(img.shape[1], img.shape[0], S.TILE, S.TILE, pw, ph)
    want = S.expected(img, xy, pw, ph)
    calls, keep = _one_slide_doors(mic, img, st_["files"][0], fmt)
    mcalls, rds = _multi_doors(mic, st_["files"], fmt)
    q = M.patch_list([S.Mic3File(d) for d in st_["files"]], pw, ph) + [(3, 2, 0, 5)]
    try:
        for door, call in calls:
            base = None
            for spec in (None, mic.OutSpec("native")):
                buf = R.Buffer(len(xy) * ph * pw * bpp, "u8")
                st, stats = call(0, xy, pw, ph, buf.ptr, buf.nbytes, spec)
                assert buf.bits().tobytes() == np.ascontiguousarray(want).tobytes(), (door, fmt)
                base = base or (st.tolist(), stats)
                assert (st.tolist(), stats) == base, (door, fmt)
        for door, call in mcalls:
            base = None
            for spec in (None, mic.OutSpec("native")):
                buf = R.Buffer(len(q) * ph * pw * bpp, "u8")
                st, stats = call(q, pw, ph, buf.ptr, buf.nbytes, spec)
                base = base or (buf.bits().tobytes(), st.tolist(), stats)
                assert (buf.bits().tobytes(), st.tolist(), stats) == base, (door, fmt)
            assert base[1][-1] == mic.MIC_ERR_ARGS and set(base[1][:-1]) == {0}
    finally:
        keep[0].close()
        keep[1].close()
        for r in rds:
            r.close()
