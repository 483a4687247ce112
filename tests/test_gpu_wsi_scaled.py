"""MIC3 patches at any magnification (csrc/mic_api_ext.hip: the _scaled doors; the kernel: k_resample_patches, csrc/mic_gather.hip).
The value of a scaled patch is exact in integers (include/mic_hip.h), so every comparison is array_equal on raw bits against the host
reference (scaled_ref.py) applied to decompress_wsi_level's image; a typed tensor goes through out_spec_ref.convert with x = v.  The
slides are those of wsi_patch_slides / wsi_multi_slides: 200 x 150 and 90 x 70, three formats."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import out_spec_ref as R
import scaled_ref as SR
import wsi_multi_slides as M
import wsi_patch_slides as S

pytestmark = pytest.mark.gpu

# 16 / 1 with pw = 4: a footprint exactly one tile wide; 1024 / 1023: weights of den - 1 and 1; (71, 37) at 3 / 2 spans four tiles
SCALES = [(2, 1), (3, 2), (7, 3), (16, 1), (1024, 1023), (1024, 64)]
SIZES = [(24, 20), (71, 37), (4, 4), (2, 3)]
CHANNEL_PAIRS = [(0.5, 3.0), (2.0, -100.0), (0.0625, -8.0)]      # (tests/test_gpu_typed_wsi.py)
BPP = {"rgb": 3, "grey8": 1, "grey16": 2}


def _pad(dtype):
    return 3.0 if dtype in ("u8", "u16") else -3.0


@pytest.fixture(scope="module")
def sets(mic, gpu_ready):
    """fmt -> dict(files = [A, B], levels = [[level image per level] per slide]); decoded once, never written to"""
    out = {}
    for fmt in S.FORMATS:
        files = [M.device_file(mic, name, fmt) for name in ("A", "B")]
        levels = [[mic.decompress_wsi_level(d, l) for l in range(S.Mic3File(d).nlev)] for d in files]
        for lv in levels:
            for a in lv:
                a.setflags(write=False)
        out[fmt] = dict(files=files, levels=levels)
    return out


@pytest.fixture(scope="module")
def doors(mic, sets):
    """fmt -> (one-slide calls on slide A, multi calls on [A, B]); a call takes (..., d, cap, spec, scale)"""
    import torch
    out, keep = {}, []
    for fmt in S.FORMATS:
        data, files, kw = sets[fmt]["files"][0], sets[fmt]["files"], S.fmt_args(fmt)
        rd = mic.WsiReader(data)
        rds = [mic.WsiReader(d) for d in files]
        sess = mic.Session(64, S.TILE * S.TILE)
        d_px = torch.from_numpy(np.ascontiguousarray(sets[fmt]["levels"][0][0]).view(np.uint8).reshape(-1).copy()).cuda()
        sess.wsi_encode(d_px.data_ptr(), S.W, S.H, tile_w=S.TILE, tile_h=S.TILE, levels=S.LEVELS, **kw)
        keep += [rd, sess] + rds

        def one(fmt=fmt, data=data, rd=rd, sess=sess):
            return [("file", lambda lv, xy, pw, ph, d, cap, spec, scale: mic.wsi_read_patches(data, lv, xy, pw, ph, d, cap, spec=spec, scale=scale)),
                    ("reader", lambda lv, xy, pw, ph, d, cap, spec, scale: rd.read_patches(lv, xy, pw, ph, d, cap, spec=spec, scale=scale)),
                    ("session", lambda lv, xy, pw, ph, d, cap, spec, scale: sess.wsi_read_patches(lv, xy, pw, ph, d, cap, spec=spec, scale=scale))]

        def multi(files=files, rds=rds, kw=kw):
            return [("files", lambda q, pw, ph, d, cap, spec, scale: mic.wsi_multi_read_patches(files, q, pw, ph, d, cap, spec=spec, scale=scale, **kw)),
                    ("readers", lambda q, pw, ph, d, cap, spec, scale: mic.wsi_readers_read_patches(rds, q, pw, ph, d, cap, spec=spec, scale=scale, **kw))]
        out[fmt] = dict(one=one(), multi=multi(), reader=rd, readers=rds, session=sess)
    yield out
    for k in keep:
        k.close()


_REF = {}


def _ref(fmt, slide, level, img, xy, pw, ph, scale):
    """the reference of one (slide, level), computed once and shared"""
    key = (fmt, slide, level, tuple(map(tuple, xy)), pw, ph, SR.reduce(*scale))      # (1024 / 64 shares 16 / 1's)
    if key not in _REF:
        v, outside = SR.resample(img, xy, pw, ph, *scale)
        v.setflags(write=False)
        outside.setflags(write=False)
        _REF[key] = (v, outside)
    return _REF[key]


def _origins(img, scale, pw, ph, tw=S.TILE, th=S.TILE):
    """wsi_patch_slides.origins for the source extent: tile-aligned, straddling four tiles, overhanging every edge, outside, negative, repeated"""
    sw, sh = SR.extent(pw, ph, *SR.reduce(*scale))
    return S.origins(img.shape[1], img.shape[0], tw, th, sw, sh)


def _native(call, n, pw, ph, bpp, *args):
    """call(*args, d, cap, None, scale) into a poisoned byte buffer -> (n, ph * pw * bpp) bytes, status, stats"""
    buf = R.Buffer(n * ph * pw * bpp, "u8")
    st, stats = call(*args[:-1], buf.ptr, buf.nbytes, None, args[-1])
    return buf.bits().reshape(n, ph * pw * bpp), st, stats


def _bytes_of(v):
    return np.ascontiguousarray(v).view(np.uint8).reshape(len(v), -1)


@pytest.mark.parametrize("scale", SCALES, ids=lambda s: "%d_%d" % s)
@pytest.mark.parametrize("fmt", S.FORMATS)
def test_all_five_doors_equal_the_reference(mic, sets, doors, fmt, scale):
    st_, bpp = sets[fmt], BPP[fmt]
    all_pad = 0
    for pw, ph in SIZES:
        sw, sh = mic.wsi_scaled_extent(pw, ph, scale)
        inside, in_level = 0, 0
        for level in (0, 1):
            img = st_["levels"][0][level]
            xy = _origins(img, scale, pw, ph)
            want, outside = _ref(fmt, 0, level, img, xy, pw, ph, scale)
            inside += sum(1 for i in range(len(xy)) if not outside[i].any())
            in_level += sum(1 for i in range(len(xy)) if not outside[i].all())
            all_pad += sum(1 for i in range(len(xy)) if outside[i].all())
            _, planned = mic.wsi_patch_plan(img.shape[1], img.shape[0], S.TILE, S.TILE, xy, sw, sh)
            for door, call in doors[fmt]["one"]:
                got, st, stats = _native(call, len(xy), pw, ph, bpp, level, xy, pw, ph, scale)
                wb = _bytes_of(want)
                for i in range(len(xy)):
                    assert np.array_equal(got[i], wb[i]), (door, fmt, scale, level, pw, ph, xy[i])
                assert (st == 0).all() and stats["pieces"] == planned and stats["slabs"] >= 1, (door, st, stats)
        # per (scale, size) at least one patch reads its level, and one lies wholly inside wherever level 0 holds the source extent
        assert in_level >= 1 and (inside >= 1 or sw > S.W or sh > S.H), (scale, pw, ph)
        # the multi doors: both slides, levels 0 and 1, shuffled, and a patch at a level its slide lacks
        q, want = [], []
        for slide in (0, 1):
            tw, th = M.GEOMETRY["AB"[slide]][2:4]
            for level in (0, 1):
                img = st_["levels"][slide][level]
                xy = _origins(img, scale, pw, ph, tw, th)
                v, _ = _ref(fmt, slide, level, img, xy, pw, ph, scale)
                q += [(x, y, slide, level) for x, y in xy]
                want += list(_bytes_of(v))
        order = np.random.default_rng(7).permutation(len(q))
        q, want = [q[i] for i in order] + [(3, 2, 0, 5)], [want[i] for i in order] + [np.zeros(ph * pw * bpp, dtype=np.uint8)]
        for door, call in doors[fmt]["multi"]:
            got, st, stats = _native(call, len(q), pw, ph, bpp, q, pw, ph, scale)
            for i in range(len(q)):
                assert np.array_equal(got[i], want[i]), (door, fmt, scale, pw, ph, q[i])
            assert (st[:-1] == 0).all() and st[-1] == mic.MIC_ERR_ARGS and stats["slides_read"] == 2, (door, st, stats)
    assert all_pad > 0                                                        # (counted: the wholly-outside origins of every list)


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_2_1_is_the_pyramid(mic, sets, doors, fmt):
    """2 / 1 from level L at even origins, patches wholly inside, is the native door's level L + 1 (from level 1: where level 2 was built
    from whole 2 x 2 blocks -- level 1 is 100 x 75, its last row has no partner)"""
    st_, bpp = sets[fmt], BPP[fmt]
    pw, ph = 24, 17
    for level in (0, 1):
        up = st_["levels"][0][level + 1]
        uh, uw = up.shape[:2]
        assert (uw, uh) == (st_["levels"][0][level].shape[1] // 2, st_["levels"][0][level].shape[0] // 2)
        xy_up = [(0, 0), (uw - pw, uh - ph), (7, 3), (uw - pw, 0), (13, uh - ph)]
        xy = [(2 * x, 2 * y) for x, y in xy_up]
        for door, call in doors[fmt]["one"]:
            got, st, _ = _native(call, len(xy), pw, ph, bpp, level, xy, pw, ph, (2, 1))
            nat, st1, _ = _native(call, len(xy), pw, ph, bpp, level + 1, xy_up, pw, ph, None)
            assert np.array_equal(got, nat) and (st == 0).all() and (st1 == 0).all(), (door, fmt, level)
            assert np.array_equal(nat, _bytes_of(S.expected(up, xy_up, pw, ph)))
    for door, call in doors[fmt]["multi"]:
        q = [(2 * x, 2 * y, 0, 0) for x, y in [(0, 0), (50, 30), (76, 58)]]
        got, st, _ = _native(call, len(q), pw, ph, bpp, q, pw, ph, (2, 1))
        nat, _, _ = _native(call, len(q), pw, ph, bpp, [(x // 2, y // 2, 0, 1) for x, y, _, _ in q], pw, ph, None)
        assert np.array_equal(got, nat) and (st == 0).all(), (door, fmt)


def _typed_expected(v, outside, dtype, pairs, channels_first, clamp, empty=()):
    """v: (n, ph, pw[, C]) reference samples; outside: (n, ph, pw); pairs: (n, C, 2) per patch; empty: patches that are all pad"""
    C = v.shape[3] if v.ndim == 4 else 1
    x = v.reshape(v.shape[:3] + (C,)).astype(np.uint16)
    out = np.repeat(outside[..., None], C, axis=3).copy()
    for i in empty:
        out[i] = True
    pr = np.asarray(pairs, dtype=np.float64).reshape(len(v), 1, 1, C, 2)
    want = R.convert(x, dtype, pr[..., 0], pr[..., 1], clamp=clamp, pad=_pad(dtype), outside=out)
    R.assert_no_subnormals(want, dtype)
    if C == 1:
        return want[..., 0]
    return np.ascontiguousarray(want.transpose(0, 3, 1, 2)) if channels_first else want


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("fmt", S.FORMATS)
def test_typed_specs(mic, sets, doors, fmt, dtype):
    st_ = sets[fmt]
    C = 3 if fmt == "rgb" else 1
    chan = CHANNEL_PAIRS if fmt == "rgb" else [R.PAIRS[2] if fmt == "grey16" else R.PAIRS[4]]
    assert all(R.exact_pair(*p) for p in chan + R.PAIRS)
    for (pw, ph), scale, channels_first, clamp in [((71, 37), (3, 2), False, None), ((24, 20), (7, 3), True, (-2.0, 60.0))]:
        # one slide: a pair per channel
        for level in (0, 1):
            img = st_["levels"][0][level]
            xy = _origins(img, scale, pw, ph)
            v, outside = _ref(fmt, 0, level, img, xy, pw, ph, scale)
            want = _typed_expected(v, outside, dtype, [chan] * len(xy), channels_first, clamp)
            assert outside.any() and not outside.all()
            spec = mic.OutSpec(dtype, channels_first=channels_first, affine=chan, clamp=clamp, pad=_pad(dtype))
            assert spec.shape(len(xy), ph, pw, channels=C) == want.shape
            for door, call in doors[fmt]["one"]:
                buf = R.Buffer(want.size, dtype)
                st, _ = call(level, xy, pw, ph, buf.ptr, buf.nbytes, spec, scale)
                got = buf.bits().reshape(want.shape)
                for i in range(len(xy)):
                    assert np.array_equal(got[i], want[i]), (door, fmt, dtype, scale, level, xy[i])
                assert (st == 0).all()
        # two slides and a refused one: a pair per (slide, channel); a bad level; pad on exactly those and the wholly-outside mask
        pairs = (R.PAIRS[:6] + CHANNEL_PAIRS) if C == 3 else [R.PAIRS[2], R.PAIRS[3], R.PAIRS[4]]
        q, vs, outs, prs = [], [], [], []
        for slide in (0, 1):
            tw, th = M.GEOMETRY["AB"[slide]][2:4]
            for level in (0, 1):
                img = st_["levels"][slide][level]
                xy = _origins(img, scale, pw, ph, tw, th)
                v, outside = _ref(fmt, slide, level, img, xy, pw, ph, scale)
                q += [(x, y, slide, level) for x, y in xy]
                vs.append(v); outs.append(outside); prs += [pairs[C * slide: C * slide + C]] * len(xy)
        empty = [len(q), len(q) + 1]
        q += [(3, 2, 0, 5), (0, 0, 2, 0)]                                       # a level slide A lacks; slide 2 does not parse
        v = np.concatenate(vs + [np.zeros((2,) + vs[0].shape[1:], dtype=vs[0].dtype)])
        outside = np.concatenate(outs + [np.ones((2, ph, pw), dtype=bool)])
        prs += [pairs[:C], pairs[2 * C: 3 * C]]
        want = _typed_expected(v, outside, dtype, prs, channels_first, clamp, empty)
        spec = mic.OutSpec(dtype, channels_first=channels_first, affine=pairs, clamp=clamp, pad=_pad(dtype))
        files = st_["files"] + [b"not a MIC3 file at all" * 8]
        kw = S.fmt_args(fmt)
        rds = doors[fmt]["readers"] + [None]
        for door, call in [("files", lambda *a: mic.wsi_multi_read_patches(files, *a, spec=spec, scale=scale, **kw)),
                           ("readers", lambda *a: mic.wsi_readers_read_patches(rds, *a, spec=spec, scale=scale, **kw))]:
            buf = R.Buffer(want.size, dtype)
            st, stats = call(q, pw, ph, buf.ptr, buf.nbytes)
            got = buf.bits().reshape(want.shape)
            for i in range(len(q)):
                assert np.array_equal(got[i], want[i]), (door, fmt, dtype, scale, q[i])
            assert (st[:-2] == 0).all() and st[-2] == mic.MIC_ERR_ARGS and st[-1] != 0 and stats["slides_read"] == 2, (door, st, stats)


def test_the_accumulator_reaches_its_peak(mic, gpu_ready):
    """a 16-bit slide with a constant-65535 tile, read at 1024 / 64 and 1024 / 1023: S reaches 1024^2 * 65535, past 32 bits"""
    import torch
    w, h = 128, 64
    yy, xx = np.mgrid[0:h, 0:w]
    img = ((xx + 2 * yy) * 19).astype(np.uint16)
    img[:, :64] = 65535
    data = mic.compress_wsi(img, w, h, tile_w=64, tile_h=64, levels=1, channels=1, bits_per_sample=16)
    assert np.array_equal(mic.decompress_wsi_level(data, 0), img)
    rd = mic.WsiReader(data)
    sess = mic.Session(64, 64 * 64)
    sess.wsi_encode(torch.from_numpy(img.view(np.uint8).reshape(-1).copy()).cuda().data_ptr(), w, h, tile_w=64, tile_h=64, levels=1, channels=1, bits_per_sample=16)
    calls = [lambda *a, **k: mic.wsi_read_patches(data, 0, *a, **k), lambda *a, **k: rd.read_patches(0, *a, **k),
             lambda *a, **k: sess.wsi_read_patches(0, *a, **k)]
    try:
        for scale, (pw, ph), xy in [((1024, 64), (4, 4), [(0, 0), (32, 0)]), ((1024, 1023), (4, 4), [(0, 0), (59, 59), (61, 3)]),
                                    ((1024, 1023), (63, 63), [(0, 0)])]:
            want, outside = SR.resample(img, xy, pw, ph, *scale)
            assert (want[0] == 65535).all() and not outside.any()
            for k, call in enumerate(calls):
                for dtype in (None, "f32"):
                    buf = R.Buffer(want.size, dtype or "u16")
                    st, _ = call(xy, pw, ph, buf.ptr, buf.nbytes, spec=mic.OutSpec(dtype) if dtype else None, scale=scale)
                    exp = want if dtype is None else R.convert(want, dtype)
                    assert np.array_equal(buf.bits().reshape(want.shape), exp) and (st == 0).all(), (k, scale, dtype)
    finally:
        rd.close()
        sess.close()


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_scale_one_is_the_as_door(mic, sets, doors, fmt):
    st_, bpp = sets[fmt], BPP[fmt]
    pw, ph = 71, 37
    img = st_["levels"][0][0]
    xy = S.origins(img.shape[1], img.shape[0], S.TILE, S.TILE, pw, ph)
    q = M.patch_list([S.Mic3File(d) for d in st_["files"]], pw, ph) + [(3, 2, 0, 5)]
    C = 3 if fmt == "rgb" else 1
    typed = mic.OutSpec("bf16", channels_first=True, affine=CHANNEL_PAIRS[:C], pad=-3.0)
    for spec, dtype, count in [(None, "u8", bpp), (typed, "bf16", C)]:
        for kind, args, n in [("one", (0, xy, pw, ph), len(xy)), ("multi", (q, pw, ph), len(q))]:
            for door, call in doors[fmt][kind]:
                base = None
                for scale in (None, (1, 1), (6, 6), (2048, 2048)):
                    buf = R.Buffer(n * ph * pw * count, dtype)
                    st, stats = call(*args, buf.ptr, buf.nbytes, spec, scale)
                    base = base or (buf.bits().tobytes(), st.tolist(), stats)
                    assert (buf.bits().tobytes(), st.tolist(), stats) == base, (door, fmt, dtype, scale)
    want = S.expected(img, xy, pw, ph)
    got, _, _ = _native(doors[fmt]["one"][0][1], len(xy), pw, ph, bpp, 0, xy, pw, ph, (6, 6))
    assert np.array_equal(got, _bytes_of(want))


@pytest.mark.parametrize("fmt", ["rgb", "grey16"])
def test_a_damaged_tile_fails_the_patches_whose_source_touches_it(mic, sets, fmt):
    st_, bpp = sets[fmt], BPP[fmt]
    f = S.Mic3File(st_["files"][0])
    tile = 5                                                              # level-0 tile (1, 1), all ramp: mode 2
    off, _ = f.plane_spans(tile)[0]
    assert f.blobs[tile][off] == 2
    f.blobs[tile][off] = 9
    data = f.bytes()
    with pytest.raises(mic.MicError) as e:
        mic.decompress_wsi_tile(data, 0, 1, 1)
    code = e.value.code
    assert code == mic.MIC_ERR_CORRUPT
    img = st_["levels"][0][0]
    rd = mic.WsiReader(data)
    try:
        for scale, (pw, ph) in [((3, 2), (24, 20)), ((7, 3), (24, 20))]:
            sw, sh = mic.wsi_scaled_extent(pw, ph, scale)
            xy = _origins(img, scale, pw, ph) + [(64 - sw, 64 - sh), (64 - sw + 1, 64 - sh + 1), (128, 64), (127, 100)]
            want, _ = _ref(fmt, 0, 0, img, xy, pw, ph, scale)
            wb = _bytes_of(want)
            for call in (lambda *a: mic.wsi_read_patches(data, 0, *a, scale=scale), lambda *a: rd.read_patches(0, *a, scale=scale),
                         lambda *a: mic.wsi_multi_read_patches([data], [(x, y, 0, 0) for x, y in a[0]], *a[1:], scale=scale, **S.fmt_args(fmt))):
                buf = R.Buffer(len(xy) * ph * pw * bpp, "u8")
                st, _ = call(xy, pw, ph, buf.ptr, buf.nbytes)[:2]
                got = buf.bits().reshape(len(xy), -1)
                hit = 0
                for i, o in enumerate(xy):
                    touches = tile in mic.wsi_patch_plan(S.W, S.H, S.TILE, S.TILE, [o], sw, sh)[0]
                    hit += touches
                    assert st[i] == (code if touches else mic.MIC_OK), (fmt, scale, o, st[i])
                    if not touches:
                        assert np.array_equal(got[i], wb[i]), (fmt, scale, o)
                assert 0 < hit < len(xy)
    finally:
        rd.close()


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_with_a_tile_cache_the_second_call_decodes_nothing(mic, sets, doors, fmt):
    st_, bpp = sets[fmt], BPP[fmt]
    scale, (pw, ph) = (7, 3), (24, 20)
    img = st_["levels"][0][0]
    xy = _origins(img, scale, pw, ph)
    want = _bytes_of(_ref(fmt, 0, 0, img, xy, pw, ph, scale)[0])
    q = [(x, y, 0, 0) for x, y in xy]
    rd, rds, sess = doors[fmt]["reader"], doors[fmt]["readers"], doors[fmt]["session"]
    kw = S.fmt_args(fmt)
    cases = [(rd.set_cache, lambda d, cap: rd.read_patches(0, xy, pw, ph, d, cap, scale=scale)),
             (rds[0].set_cache, lambda d, cap: mic.wsi_readers_read_patches(rds, q, pw, ph, d, cap, scale=scale, **kw)),
             (sess.set_tile_cache, lambda d, cap: sess.wsi_read_patches(0, xy, pw, ph, d, cap, scale=scale))]
    for k, (attach, call) in enumerate(cases):
        cache = mic.TileCache(S.TILE, S.TILE, slots=32, **kw)
        attach(cache)
        try:
            decoded = []
            sess.set_timing(True)
            for _ in range(2):
                buf = R.Buffer(len(xy) * ph * pw * bpp, "u8")
                st, stats = call(buf.ptr, buf.nbytes)
                assert np.array_equal(buf.bits().reshape(len(xy), -1), want) and (st == 0).all(), (fmt, k)
                decoded.append(stats["tiles_decoded"])
            assert decoded[0] > 0 and decoded[1] == 0, (fmt, k, decoded)
            if k == 2:                                                       # the store's warm call: one gather out of the cache, one resample
                assert [name for name, _ in sess.last_timings()] == ["k_wsi_gather_cached", "k_wsi_resample"]
        finally:
            sess.set_timing(False)
            attach(None)
            cache.close()


def test_argument_checks_come_in_the_native_order(mic, sets, doors):
    """the scale is judged right behind pw, ph and n: before the spec, out_cap and the pointer"""
    fmt = "rgb"
    xy, pw, ph = [(0, 0), (5, 5)], 24, 20
    q = [(0, 0, 0, 0), (5, 5, 1, 1)]
    spec = mic.OutSpec("bf16")
    for kind, args in [("one", (0, xy, pw, ph)), ("multi", (q, pw, ph))]:
        for door, call in doors[fmt][kind]:
            def code(spec_, scale, skew=0, short=0, a=args):
                buf = R.Buffer(2 * ph * pw * 3, "bf16", skew=skew)
                with pytest.raises(mic.MicError) as e:
                    call(*a, buf.ptr, buf.nbytes - short, spec_, scale)
                assert buf.untouched(), door
                return e.value.code
            assert code(spec, (1, 2), short=4) == mic.MIC_ERR_ARGS                      # a bad scale with a bad out_cap
            assert code(spec, (17, 1), short=4) == mic.MIC_ERR_ARGS
            assert code(spec, (3, 2), short=4) == mic.MIC_ERR_CAPACITY                  # ... and the out_cap alone
            assert code(spec, (3, 2), skew=1) == mic.MIC_ERR_ARGS                       # a misaligned base
            assert code(mic.OutSpec("f32", clamp=(1.0, 1.0)), (3, 2)) == mic.MIC_ERR_ARGS
            if kind == "one":
                assert code(spec, (3, 2), a=(S.LEVELS, xy, pw, ph)) == mic.MIC_ERR_ARGS
            buf = R.Buffer(0, "bf16")
            st, stats = call(*((0, [], pw, ph) if kind == "one" else ([], pw, ph)), buf.ptr, 0, spec, (3, 2))   # n = 0 is no error
            assert st.size == 0 and stats["tiles_decoded"] == 0 and stats["slabs"] == 0


def test_patch_groups_under_a_small_workspace():
    """2 MiB of workspace: the staging tensor may take a quarter of it, and the 36 source rectangles of 166 x 87 pixels take 1.5 MiB
    (RGB: three groups) or 1 MiB (16-bit: two) (tests/wsi_scaled_chunking_check.py, in a process of its own because the workspace
    ceiling is read once)"""
    env = dict(os.environ, MIC_HIP_WS_BUDGET_MB="2")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wsi_scaled_chunking_check.py")], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "scaled patch groups ok" in r.stdout, r.stdout + r.stderr
