"""The MIC3 tile cache on the device (include/mic_hip.h: mic_hip_tile_cache_*; the core: read_patches in csrc/mic_api_ext.hip; the
kernels that fill and read pixel slots: csrc/mic_gather.hip, csrc/mic_px_copy.h).  A reader or session with a cache decodes only the
tiles that are not resident and gathers hits and fresh tiles out of the cache; the bytes it writes are those of the uncached doors,
which the existing tests hold against the level images.  Every comparison here is byte for byte.

The slide is wsi_patch_slides' (200 x 150, 64-pixel tiles, 3 levels), so a call is a few hundred microseconds and a test well under a
second; the timings of the feature are tools/bench_wsi_tile_cache.py's (profiles/wsi_tile_cache.json)."""
import threading

import numpy as np
import pytest

import out_spec_ref as R
from tile_cache_model import lru_model
import wsi_multi_slides as M
import wsi_patch_slides as S

pytestmark = pytest.mark.gpu

PATCHES = [(1, 1), (37, 29), (64, 64), (65, 3)]


@pytest.fixture(scope="module")
def slides(mic, gpu_ready):
    """fmt -> dict(img, file, parsed, levels = [level image per level]); decoded once, never written to"""
    out = {}
    for fmt in S.FORMATS:
        img, data = S.make_file(mic, fmt)
        f = S.Mic3File(data)
        levels = [mic.decompress_wsi_level(data, l) for l in range(f.nlev)]
        assert f.nlev == S.LEVELS and np.array_equal(levels[0], img)
        for a in levels:
            a.setflags(write=False)
        out[fmt] = dict(img=img, file=data, parsed=f, levels=levels)
    return out


class _Source:
    """a reader's source that counts its callbacks and the bytes they read, and fails on demand"""

    def __init__(self, data):
        self.data, self.reads, self.fail = data, [], False

    def __call__(self, off, n):
        if self.fail:
            raise OSError("source failure on demand")
        self.reads.append((off, n))
        return self.data[off: off + n]

    def take(self):
        r, self.reads = self.reads, []
        return r


def _bpp(like):
    return like.dtype.itemsize * (3 if like.ndim == 3 else 1)


def _skews(like):
    return (0, 2) if like.dtype == np.uint16 else (0, 1, 2, 3)


def _read(call, xy, pw, ph, like, skew=0):
    """call(xy, pw, ph, d_out, out_cap) -> (status, stats); the patches as an array shaped like S.expected's; the tensor `skew` bytes
    behind an aligned address, the bytes around it checked (out_spec_ref.Buffer)"""
    buf = R.Buffer(len(xy) * ph * pw * _bpp(like), "u8", skew)
    st, stats = call(xy, pw, ph, buf.ptr, buf.nbytes)
    got = buf.bits()
    if like.dtype == np.uint16:
        got = got.view("<u2")
    return got.reshape((len(xy), ph, pw) + like.shape[2:]), st, stats


def _reader_call(rd, level):
    return lambda xy, pw, ph, d, cap: rd.read_patches(level, xy, pw, ph, d, cap)


def _keys(mic, f, level, xy, pw, ph):
    """global tile indices of the tiles the patches touch, ascending: the call's keys in plan order"""
    lw, lh, _, _, first = f.levels[level]
    return [first + int(t) for t in mic.wsi_patch_plan(lw, lh, S.TILE, S.TILE, xy, pw, ph)[0]]


def _blob_bytes(f, keys):
    """file offsets -> 1 over the blobs of `keys`"""
    body = 48 + 20 * f.nlev + 16 * f.total
    offs = np.concatenate([[0], np.cumsum([len(b) for b in f.blobs])])
    want = np.zeros(body + int(offs[-1]), dtype=np.int32)
    for t in keys:
        want[body + offs[t]: body + offs[t + 1]] += 1
    return want


def _fetched(n, reads):
    got = np.zeros(n, dtype=np.int32)
    for off, k in reads:
        got[off: off + k] += 1
    return got


def _delta(after, before):
    return {k: after[k] - before[k] for k in ("hits", "misses", "bypassed", "evictions", "calls")}


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", S.FORMATS)
def test_parity_cold_warm_and_after_eviction(mic, slides, fmt):
    sl = slides[fmt]
    f = sl["parsed"]
    kw = S.fmt_args(fmt)
    plain = mic.WsiReader(sl["file"])
    rd, other = mic.WsiReader(sl["file"]), mic.WsiReader(sl["file"])
    try:
        for level, img in enumerate(sl["levels"]):
            lh, lw = img.shape[:2]
            for pw, ph in PATCHES:
                xy = S.origins(lw, lh, S.TILE, S.TILE, pw, ph)
                want = S.expected(img, xy, pw, ph)
                keys = _keys(mic, f, level, xy, pw, ph)
                half = (len(keys) + 1) // 2
                evict = [(S.TILE * (t % 4), S.TILE * (t // 4)) for t in range(half)]          # `half` tiles of level 0, through the other reader
                base, st0, _ = _read(_reader_call(plain, level), xy, pw, ph, img)
                assert np.array_equal(base, want)
                for skew in _skews(img):
                    cache = mic.TileCache(S.TILE, S.TILE, slots=len(keys), **kw)
                    rd.set_cache(cache)
                    other.set_cache(cache)
                    for what in ("cold", "warm", "evict", "third"):
                        if what == "evict":
                            _read(_reader_call(other, 0), evict, 1, 1, sl["levels"][0])
                            assert rd.cache_probe(keys).sum() == len(keys) - half
                            continue
                        got, st, stats = _read(_reader_call(rd, level), xy, pw, ph, img, skew)
                        assert np.array_equal(got, want), (what, level, pw, ph, skew)
                        assert np.array_equal(st, st0)
                        assert stats["tiles_decoded"] == {"cold": len(keys), "warm": 0, "third": half}[what]
                    rd.set_cache(None)
                    other.set_cache(None)
                    cache.close()
    finally:
        for r in (plain, rd, other):
            r.close()


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", S.FORMATS)
def test_work_really_is_skipped(mic, slides, fmt):
    import torch
    sl = slides[fmt]
    f, img = sl["parsed"], sl["levels"][0]
    src = _Source(sl["file"])
    pw, ph = 37, 29
    a = [(0, 0), (70, 10), (50, 50)]
    b = a + [(130, 70), (10, 100)]
    ka, kb = _keys(mic, f, 0, a, pw, ph), _keys(mic, f, 0, b, pw, ph)
    assert set(ka) < set(kb)
    with mic.TileCache(S.TILE, S.TILE, slots=32, **S.fmt_args(fmt)) as cache, mic.WsiReader(src, len(sl["file"])) as rd:
        rd.set_cache(cache)
        src.take()
        got, st, stats = _read(_reader_call(rd, 0), a, pw, ph, img)
        assert np.array_equal(got, S.expected(img, a, pw, ph)) and stats["tiles_decoded"] == len(ka) and stats["slabs"] >= 1
        assert np.array_equal(_fetched(len(sl["file"]), src.take()), _blob_bytes(f, ka))
        s0 = cache.stats()
        assert s0["misses"] == len(ka) and s0["resident"] == len(ka) and s0["device_bytes"] == 32 * mic.tile_cache_slot_bytes(S.TILE, S.TILE, **S.fmt_args(fmt))
        got, st, stats = _read(_reader_call(rd, 0), a, pw, ph, img)                 # the identical call: nothing is read, nothing decoded
        assert np.array_equal(got, S.expected(img, a, pw, ph)) and (st == 0).all()
        assert src.take() == [] and stats["tiles_decoded"] == 0 and stats["slabs"] == 0
        _, planned = mic.wsi_patch_plan(img.shape[1], img.shape[0], S.TILE, S.TILE, a, pw, ph)
        assert stats["pieces"] == planned
        assert _delta(cache.stats(), s0) == dict(hits=len(ka), misses=0, bypassed=0, evictions=0, calls=1)
        got, st, stats = _read(_reader_call(rd, 0), b, pw, ph, img)                 # A u B behind A: exactly the blobs of B \ A
        assert np.array_equal(got, S.expected(img, b, pw, ph))
        assert np.array_equal(_fetched(len(sl["file"]), src.take()), _blob_bytes(f, sorted(set(kb) - set(ka))))
        assert stats["tiles_decoded"] == len(kb) - len(ka)
        rd.set_cache(None)
    # the session store: what ran, by its timer labels
    sess = mic.Session(64, S.TILE * S.TILE)
    cache = mic.TileCache(S.TILE, S.TILE, slots=32, **S.fmt_args(fmt))
    try:
        d_px = torch.from_numpy(np.ascontiguousarray(sl["img"]).view(np.uint8).reshape(-1).copy()).cuda()
        sess.wsi_encode(d_px.data_ptr(), S.W, S.H, tile_w=S.TILE, tile_h=S.TILE, levels=S.LEVELS, **S.fmt_args(fmt))
        sess.set_tile_cache(cache)
        sess.set_timing(True)
        call = lambda xy, w, h, d, cap: sess.wsi_read_patches(0, xy, w, h, d, cap)
        got, _, stats = _read(call, b, pw, ph, img)
        cold = dict(sess.last_timings())
        assert np.array_equal(got, S.expected(img, b, pw, ph)) and stats["tiles_decoded"] == len(kb)
        assert "k_wsi_cache_fill" in cold and "k_wsi_gather_cached" in cold
        got, _, stats = _read(call, b, pw, ph, img)
        warm = dict(sess.last_timings())
        assert np.array_equal(got, S.expected(img, b, pw, ph)) and stats["tiles_decoded"] == 0 and stats["slabs"] == 0
        assert list(warm) == ["k_wsi_gather_cached"], warm                          # no decode chain, no fill, no slab gather
    finally:
        sess.close()
        cache.close()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb", "grey16"])
def test_capacity_seams_follow_the_host_model(mic, slides, fmt):
    sl = slides[fmt]
    f, img = sl["parsed"], sl["levels"][0]
    pw, ph = 37, 29
    trace = [[(0, 0), (70, 10), (50, 50)], [(130, 70), (10, 100), (50, 50)], [(0, 0), (70, 10), (50, 50)], [(60, 60), (150, 120)], [(130, 70)]]
    keys = [_keys(mic, f, 0, xy, pw, ph) for xy in trace]
    union = sorted(set().union(*keys))
    for nslots in (0, 1, len(union) - 1, len(union)):
        outcome, evictions = mic.tile_cache_plan(nslots, keys)
        resident = set()
        with mic.TileCache(S.TILE, S.TILE, slots=nslots, **S.fmt_args(fmt)) as cache, mic.WsiReader(sl["file"]) as rd:
            rd.set_cache(cache)
            for k, xy in enumerate(trace):
                before = cache.stats()
                got, st, stats = _read(_reader_call(rd, 0), xy, pw, ph, img)
                assert np.array_equal(got, S.expected(img, xy, pw, ph)) and (st == 0).all(), (nslots, k)
                o = outcome[k]
                assert _delta(cache.stats(), before) == dict(hits=int((o == 0).sum()), misses=int((o == 1).sum()), bypassed=int((o == 2).sum()),
                                                             evictions=_model_evictions(nslots, keys, k), calls=1), (nslots, k)
                assert stats["tiles_decoded"] == int((o != 0).sum())
                want = _model_resident(nslots, keys, k)
                assert set(np.asarray(union)[rd.cache_probe(union)].tolist()) == want, (nslots, k)
                assert cache.stats()["resident"] == len(want)
            assert cache.stats()["evictions"] == evictions
            rd.set_cache(None)


def _model_resident(nslots, keys, k):
    """the keys resident behind call k, by the host model of the policy (tile_cache_model.py)"""
    return lru_model(nslots, keys[: k + 1])[2][k]


def _model_evictions(nslots, keys, k):
    return lru_model(nslots, keys[: k + 1])[1] - (lru_model(nslots, keys[:k])[1] if k else 0)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damage", ["mode byte 9", "flipped stream byte", "zero plane length"])
def test_a_damaged_tile_is_never_resident(mic, slides, damage):
    sl = slides["rgb"]
    f = S.Mic3File(sl["file"])
    tile = {"mode byte 9": 0, "flipped stream byte": 5, "zero plane length": 3}[damage]     # level-0 tiles, all ramp: mode 2
    off, n = f.plane_spans(tile)[0]
    assert f.blobs[tile][off] == 2
    if damage == "mode byte 9":
        f.blobs[tile][off] = 9
    elif damage == "flipped stream byte":
        f.blobs[tile][off + 1 + (n - 1) // 2] ^= 0x5A
    else:
        f.blobs[tile][0:4] = bytes(4)
    data = f.bytes()
    img = sl["levels"][0]
    pw, ph = 48, 40
    xy = S.origins(S.W, S.H, S.TILE, S.TILE, pw, ph)
    keys = _keys(mic, f, 0, xy, pw, ph)
    assert tile in keys
    src = _Source(data)
    with mic.TileCache(S.TILE, S.TILE, slots=32) as cache, mic.WsiReader(data) as plain, mic.WsiReader(src, len(data)) as rd:
        base, st0, _ = _read(_reader_call(plain, 0), xy, pw, ph, img)
        failed = bool((st0 != mic.MIC_OK).any())                               # (the flipped stream may still decode)
        rd.set_cache(cache)
        for call in (1, 2):
            src.take()
            got, st, stats = _read(_reader_call(rd, 0), xy, pw, ph, img)
            assert np.array_equal(st, st0), call
            for i in range(len(xy)):
                if st0[i] == mic.MIC_OK:
                    assert np.array_equal(got[i], base[i]) and (tile in _keys(mic, f, 0, [xy[i]], pw, ph) or np.array_equal(got[i], S.expected(img, [xy[i]], pw, ph)[0]))
            bad = (st0 != mic.MIC_OK).any()
            res = rd.cache_probe(keys)
            assert [k for k, r in zip(keys, res) if not r] == ([tile] if bad else []), call
            if call == 2:                                                      # the next call decodes it again, and it alone
                assert stats["tiles_decoded"] == (1 if bad else 0)
                assert np.array_equal(_fetched(len(data), src.take()), _blob_bytes(f, [tile] if bad else []))
        if damage != "flipped stream byte":
            assert failed
        rd.set_cache(None)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def test_a_failing_callback_undoes_the_call(mic, slides):
    sl = slides["rgb"]
    f, img = sl["parsed"], sl["levels"][0]
    src = _Source(sl["file"])
    pw, ph = 37, 29
    pre, a, b = [(150, 120)], [(0, 0), (70, 10)], [(0, 0), (70, 10), (130, 70), (10, 100)]
    union = sorted(set(_keys(mic, f, 0, b, pw, ph)) | set(_keys(mic, f, 0, pre, pw, ph)))
    with mic.TileCache(S.TILE, S.TILE, slots=4) as cache, mic.WsiReader(src, len(sl["file"])) as rd:
        rd.set_cache(cache)
        _read(_reader_call(rd, 0), pre, pw, ph, img)                           # tiles 6 and 10, the oldest entries
        _read(_reader_call(rd, 0), a, pw, ph, img)                             # tiles 0 and 1: the cache is full
        before, res = cache.stats(), rd.cache_probe(union)
        assert res.sum() == 4 and before["evictions"] == 0                     # the next call hits two tiles and would evict two to keep its misses
        out, _ = mic.tile_cache_plan(4, [_keys(mic, f, 0, x, pw, ph) for x in (pre, a, b)])
        assert sorted(set(out[2].tolist())) == [0, 1, 2]                       # (by the policy: hits, kept misses that evict, and a bypassed one)
        src.fail = True
        buf = R.Buffer(len(b) * ph * pw * 3, "u8")
        with pytest.raises(OSError):
            rd.read_patches(0, b, pw, ph, buf.ptr, buf.nbytes)
        assert buf.untouched()
        assert cache.stats() == before and np.array_equal(rd.cache_probe(union), res)
        arr = mic._patch_xy(b)
        rc = mic.lib().mic_hip_wsi_reader_read_patches(rd._h, 0, arr.ctypes.data, len(b), pw, ph, buf.ptr, buf.nbytes, None, None)
        rd._cb.exc = None
        assert rc == mic.MIC_ERR_IO and buf.untouched() and cache.stats() == before
        src.fail = False
        got, st, _ = _read(_reader_call(rd, 0), b, pw, ph, img)
        assert np.array_equal(got, S.expected(img, b, pw, ph)) and (st == 0).all()
        rd.set_cache(None)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
CHANNEL_PAIRS = [(0.5, 3.0), (2.0, -100.0), (0.0625, -8.0)]


def _typed_expected(img, xy, pw, ph, dtype, pairs, channels_first, clamp=None, pad=0.0):
    C = img.shape[2] if img.ndim == 3 else 1
    x = S.expected(img, xy, pw, ph).reshape(len(xy), ph, pw, C).astype(np.uint16)
    outside = R.outside_mask(xy, lambda _: img.shape[1], lambda _: img.shape[0], pw, ph)[..., None] | np.zeros((1, 1, 1, C), dtype=bool)
    pr = np.asarray(pairs, dtype=np.float64).reshape(-1, 2)
    a, b = pr[:, 0].reshape(1, 1, 1, -1), pr[:, 1].reshape(1, 1, 1, -1)
    want = R.convert(x, dtype, a, b, clamp=clamp, pad=pad, outside=outside)
    R.assert_no_subnormals(want, dtype)
    if C == 1:
        return want[..., 0]
    return np.ascontiguousarray(want.transpose(0, 3, 1, 2)) if channels_first else want


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_typed_doors_read_the_native_pixels_of_the_cache(mic, slides, fmt):
    sl = slides[fmt]
    f = sl["parsed"]
    assert all(R.exact_pair(*p) for p in CHANNEL_PAIRS)
    pairs = CHANNEL_PAIRS if fmt == "rgb" else CHANNEL_PAIRS[:1]
    u8_pair = [(0.5, 3.0)] if fmt != "grey16" else [(0.0625, -8.0)]
    specs = [("bf16", dict(channels_first=True, affine=pairs), dict(pairs=pairs, channels_first=True)),
             ("u8", dict(affine=u8_pair, clamp=(10.0, 100.0)), dict(pairs=u8_pair, channels_first=False, clamp=(10.0, 100.0))),
             ("f32", dict(pad=-3.0), dict(pairs=[(1.0, 0.0)], channels_first=False, pad=-3.0))]
    with mic.TileCache(S.TILE, S.TILE, slots=32, **S.fmt_args(fmt)) as cache, mic.WsiReader(sl["file"]) as rd:
        rd.set_cache(cache)
        for level in (0, 1):
            img = sl["levels"][level]
            for pw, ph in ((37, 29), (65, 3)):
                xy = S.origins(img.shape[1], img.shape[0], S.TILE, S.TILE, pw, ph)
                nk = len(_keys(mic, f, level, xy, pw, ph))
                for dtype, skw, ekw in specs:
                    cache.clear()
                    want = _typed_expected(img, xy, pw, ph, dtype, **ekw)
                    spec = mic.OutSpec(dtype, **skw)
                    for what in ("typed cold", "typed warm"):
                        buf = R.Buffer(want.size, dtype)
                        st, stats = rd.read_patches(level, xy, pw, ph, buf.ptr, buf.nbytes, spec=spec)
                        assert np.array_equal(buf.bits().reshape(want.shape), want), (what, dtype, level, pw, ph)
                        assert (st == 0).all() and stats["tiles_decoded"] == (nk if what == "typed cold" else 0)
                    cache.clear()                                              # a typed call right behind a native one: all hits
                    got, _, stats = _read(_reader_call(rd, level), xy, pw, ph, img)
                    assert np.array_equal(got, S.expected(img, xy, pw, ph)) and stats["tiles_decoded"] == nk
                    buf = R.Buffer(want.size, dtype)
                    st, stats = rd.read_patches(level, xy, pw, ph, buf.ptr, buf.nbytes, spec=spec)
                    assert np.array_equal(buf.bits().reshape(want.shape), want) and stats["tiles_decoded"] == 0 and stats["slabs"] == 0
        rd.set_cache(None)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", S.FORMATS)
def test_alignment_seams_of_the_pixel_gather(mic, slides, fmt):
    sl = slides[fmt]
    img = sl["levels"][0]
    with mic.TileCache(S.TILE, S.TILE, slots=32, **S.fmt_args(fmt)) as cache, mic.WsiReader(sl["file"]) as rd:
        rd.set_cache(cache)
        _read(_reader_call(rd, 0), [(0, 0), (64, 0), (0, 64), (64, 64), (128, 0), (128, 64)], 64, 64, img)      # what the patches below touch
        ph = 5
        xy = [(x, y) for x in (0, 1, 2, 3, 61) for y in (0, 62)]               # (y = 62: pieces of two tile rows)
        for pw in (1, 3, 17, 63, 64, 65):
            want = S.expected(img, xy, pw, ph)
            for skew in _skews(img):
                got, st, stats = _read(_reader_call(rd, 0), xy, pw, ph, img, skew)
                assert stats["tiles_decoded"] == 0 and stats["slabs"] == 0          # all hits: only the new kernels ran
                assert np.array_equal(got, want), (pw, skew)
        rd.set_cache(None)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb", "grey16"])
def test_many_readers_in_one_call(mic, slides, fmt):
    kw = S.fmt_args(fmt)
    files = [slides[fmt]["file"], slides[fmt]["file"], M.device_file(mic, "B", fmt), M.device_file(mic, "C", fmt),
             M.device_file(mic, "B", M.OTHER_FORMAT[fmt])]                     # the last one is refused: another sample format
    parsed = [S.Mic3File(d) for d in files]
    srcs = [_Source(d) for d in files]
    rds = [mic.WsiReader(s, len(d)) for s, d in zip(srcs, files)]
    shared = mic.TileCache(S.TILE, S.TILE, slots=64, **kw)
    own = mic.TileCache(*M.GEOMETRY["B"][2:4], slots=64, **kw)
    try:
        rds[0].set_cache(shared)
        rds[1].set_cache(shared)
        rds[2].set_cache(own)
        pw, ph = 24, 20
        q = M.patch_list(parsed, pw, ph)
        bpp = (2 if fmt == "grey16" else 1) * (3 if fmt == "rgb" else 1)
        base = R.Buffer(len(q) * ph * pw * bpp, "u8")
        st0, stats0 = mic.wsi_multi_read_patches(files, q, pw, ph, base.ptr, base.nbytes, **kw)
        want = base.bits()
        assert (st0[[i for i, p in enumerate(q) if p[2] == 4]] == mic.MIC_ERR_ARGS).all() and (st0[[i for i, p in enumerate(q) if p[2] < 4]] == 0).all()
        for s in srcs:
            s.take()
        for call in (1, 2):
            buf = R.Buffer(len(q) * ph * pw * bpp, "u8")
            st, stats = mic.wsi_readers_read_patches(rds, q, pw, ph, buf.ptr, buf.nbytes, **kw)
            assert np.array_equal(buf.bits(), want) and np.array_equal(st, st0), call
            reads = [s.take() for s in srcs]
            assert stats["pieces"] == stats0["pieces"] and stats["slides_read"] == stats0["slides_read"]
            if call == 1:
                assert stats["tiles_decoded"] == stats0["tiles_decoded"] and all(reads[:4]) and not reads[4]
                every = reads[3]
            else:                                                              # nothing through the cached readers; the fourth reads everything again
                assert reads[0] == reads[1] == reads[2] == [] and reads[3] == every and not reads[4]
                assert stats["tiles_decoded"] == int((mic.wsi_multi_patch_plan(files, q, pw, ph, **kw)[0] == 3).sum())
        n0 = sum(1 for _ in parsed[0].blobs)
        assert shared.stats()["resident"] == 2 * rds[0].cache_probe(range(n0)).sum() and rds[0].cache_probe(range(n0)).sum() > 0
        assert own.stats()["resident"] == rds[2].cache_probe(range(len(parsed[2].blobs))).sum() > 0
    finally:
        for r in rds:
            r.close()
        shared.close()
        own.close()


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", S.FORMATS)
def test_session_store_and_its_generations(mic, slides, fmt):
    import torch
    sl = slides[fmt]
    f, img = sl["parsed"], sl["levels"][0]
    pw, ph = 37, 29
    xy = S.origins(S.W, S.H, S.TILE, S.TILE, pw, ph)
    keys = _keys(mic, f, 0, xy, pw, ph)
    sess = mic.Session(64, S.TILE * S.TILE)
    cache = mic.TileCache(S.TILE, S.TILE, slots=32, **S.fmt_args(fmt))
    try:
        d_px = torch.from_numpy(np.ascontiguousarray(sl["img"]).view(np.uint8).reshape(-1).copy()).cuda()
        sess.wsi_encode(d_px.data_ptr(), S.W, S.H, tile_w=S.TILE, tile_h=S.TILE, levels=S.LEVELS, **S.fmt_args(fmt))
        sess.set_tile_cache(cache)
        call = lambda a, w, h, d, cap: sess.wsi_read_patches(0, a, w, h, d, cap)
        for k in (1, 2):
            got, st, stats = _read(call, xy, pw, ph, img)
            assert np.array_equal(got, S.expected(img, xy, pw, ph)) and (st == 0).all()
            assert stats["tiles_decoded"] == (len(keys) if k == 1 else 0)
        assert cache.stats()["resident"] == len(keys) and sess.tile_cache_probe(keys).all()
        # another slide into the same session: the negative (the same tiles are noise, ramp and constant, so the encoder takes it)
        flipped = np.ascontiguousarray((4095 if fmt == "grey16" else 255) - sl["img"])
        d_px2 = torch.from_numpy(flipped.view(np.uint8).reshape(-1).copy()).cuda()
        sess.wsi_encode(d_px2.data_ptr(), S.W, S.H, tile_w=S.TILE, tile_h=S.TILE, levels=S.LEVELS, **S.fmt_args(fmt))
        assert cache.stats()["resident"] == 0 and not sess.tile_cache_probe(keys).any()
        got, st, stats = _read(call, xy, pw, ph, img)
        assert np.array_equal(got, S.expected(flipped, xy, pw, ph)) and stats["tiles_decoded"] == len(keys)
        assert mic.lib().mic_hip_tile_cache_destroy(cache._h) == mic.MIC_ERR_ARGS      # the session is attached
    finally:
        sess.close()                                                           # (detaches)
        cache.close()


# ---- 10 -----------------------------------------------------------------------------------------------------------------------------
def test_two_readers_of_one_file_are_two_owners(mic, slides):
    sl = slides["grey8"]
    f, img = sl["parsed"], sl["levels"][0]
    pw, ph = 37, 29
    a, b = [(0, 0), (70, 10)], [(70, 10), (130, 70), (10, 100)]
    ka, kb = _keys(mic, f, 0, a, pw, ph), _keys(mic, f, 0, b, pw, ph)
    every = list(range(f.total))
    cache = mic.TileCache(S.TILE, S.TILE, slots=32, **S.fmt_args("grey8"))
    ra, rb = mic.WsiReader(sl["file"]), mic.WsiReader(sl["file"])
    try:
        ra.set_cache(cache)
        rb.set_cache(cache)
        _read(_reader_call(ra, 0), a, pw, ph, img)
        got, _, stats = _read(_reader_call(rb, 0), b, pw, ph, img)
        assert stats["tiles_decoded"] == len(kb)                               # rb sees nothing of what ra brought in
        assert np.array_equal(got, S.expected(img, b, pw, ph))
        assert [k for k in every if ra.cache_probe([k])[0]] == ka and [k for k in every if rb.cache_probe([k])[0]] == kb
        assert cache.stats()["resident"] == len(ka) + len(kb)
        ra.close()
        assert cache.stats()["resident"] == len(kb) and rb.cache_probe(kb).all()
        got, _, stats = _read(_reader_call(rb, 0), b, pw, ph, img)
        assert stats["tiles_decoded"] == 0 and np.array_equal(got, S.expected(img, b, pw, ph))
    finally:
        ra.close()
        rb.close()
        cache.close()


# ---- 11 -----------------------------------------------------------------------------------------------------------------------------
def test_two_threads_share_one_cache(mic, slides):
    sl = slides["rgb"]
    img = sl["levels"][0]
    pw, ph = 37, 29
    lists = [[(0, 0), (70, 10), (50, 50)], [(130, 70), (10, 100), (50, 50)], [(60, 60), (150, 120)]]
    cache = mic.TileCache(S.TILE, S.TILE, slots=6)                             # fewer slots than the tiles in play: the threads evict each other
    rds = [mic.WsiReader(sl["file"]), mic.WsiReader(sl["file"])]
    errors, rounds = [], 4

    def work(rd, order):
        try:
            for k in range(rounds):
                xy = lists[(k + order) % len(lists)]
                got, st, _ = _read(_reader_call(rd, 0), xy, pw, ph, img)
                if not (np.array_equal(got, S.expected(img, xy, pw, ph)) and (st == 0).all()):
                    errors.append((order, k))
        except BaseException as e:                                             # (an assertion in a thread would pass unseen)
            errors.append(e)

    try:
        for r in rds:
            r.set_cache(cache)
        ts = [threading.Thread(target=work, args=(r, i)) for i, r in enumerate(rds)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert errors == []
        assert cache.stats()["calls"] == 2 * rounds
    finally:
        for r in rds:
            r.close()
        cache.close()


# ---- 12 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", S.FORMATS)
def test_no_cache_nothing_new(mic, slides, fmt):
    import torch
    sl = slides[fmt]
    pw, ph = 37, 29
    with mic.TileCache(S.TILE, S.TILE, slots=8, **S.fmt_args(fmt)) as cache, mic.WsiReader(sl["file"]) as rd:
        for detached in (False, True):
            if detached:                                                       # ... and a reader that had a cache and let it go
                rd.set_cache(cache)
                _read(_reader_call(rd, 0), [(0, 0)], pw, ph, sl["levels"][0])
                rd.set_cache(None)
                before = cache.stats()
            for level, img in enumerate(sl["levels"]):
                xy = S.origins(img.shape[1], img.shape[0], S.TILE, S.TILE, pw, ph)
                base, st0, stats0 = _read(lambda a, w, h, d, cap: mic.wsi_read_patches(sl["file"], level, a, w, h, d, cap), xy, pw, ph, img)
                got, st, stats = _read(_reader_call(rd, level), xy, pw, ph, img)
                assert np.array_equal(got, base) and np.array_equal(st, st0) and stats == stats0
            if detached:
                assert cache.stats() == before
    sess = mic.Session(64, S.TILE * S.TILE)
    try:
        d_px = torch.from_numpy(np.ascontiguousarray(sl["img"]).view(np.uint8).reshape(-1).copy()).cuda()
        sess.wsi_encode(d_px.data_ptr(), S.W, S.H, tile_w=S.TILE, tile_h=S.TILE, levels=S.LEVELS, **S.fmt_args(fmt))
        sess.set_timing(True)
        img = sl["levels"][0]
        xy = S.origins(S.W, S.H, S.TILE, S.TILE, pw, ph)
        got, st, stats = _read(lambda a, w, h, d, cap: sess.wsi_read_patches(0, a, w, h, d, cap), xy, pw, ph, img)
        base, st0, stats0 = _read(lambda a, w, h, d, cap: mic.wsi_read_patches(sl["file"], 0, a, w, h, d, cap), xy, pw, ph, img)
        assert np.array_equal(got, base) and np.array_equal(st, st0) and stats == stats0
        assert list(dict(sess.last_timings())) == ["k_wsi_gather_patches"]          # the labels of the plain path, and no other
    finally:
        sess.close()
