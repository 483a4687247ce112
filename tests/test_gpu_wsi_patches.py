"""Many patches per call into a device tensor (csrc/mic_api_ext.hip: mic_hip_wsi_read_patches, mic_hip_wsi_reader_read_patches,
mic_hip_session_wsi_read_patches).  The codec is lossless, so the expected value of every patch is the level image of the existing
decompress_wsi_level, padded with zeros and cropped in numpy; at level 0 that image is also compared with the source pixels.

The slides (wsi_patch_slides.slide) hold a ramp, one whole tile of noise, a white and a black whole tile, so that constant planes
(modes 0 / 1) and streams (mode 2) occur among the tiles the patches touch.  Raw planes (mode 3): no noise slide gives one -- the
reference's encoder takes that branch on ErrIncompressible only, and noise wide enough for it makes its normaliser fail first
(checked with the oracle: 8-bit RGB noise and 16-bit greyscale noise of 8 bits and more return an error from CompressWSI, narrower
noise codes as mode 2; tests/test_oracle_wavelet_wsi.py has the same finding) -- so the noise tile's planes are rewritten raw in the
file's bytes (wsi_patch_slides.raw_plane_file), the pixels unchanged, and the oracle decodes that file to the same pixels."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import wsi_patch_slides as S

pytestmark = pytest.mark.gpu

# (47, 3): an odd width, so that every second row of a 16-bit patch starts off a 4-byte boundary -- the grey kernel's dword rows and
# its u16 rows alternate inside one piece
PATCHES = [(48, 40), (130, 70), (1, 1), (47, 3)]
ODD = (47, 3)


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


def _tensor(n, ph, pw, bpp):
    import torch
    return torch.full((max(n, 1), ph, pw, bpp), 0xA5, dtype=torch.uint8, device="cuda")     # (every byte must be overwritten)


def _pixels(t, n, like):
    a = t.cpu().numpy()[:n]
    if like.dtype == np.uint16:
        return a.view("<u2")[..., 0]
    return a if like.ndim == 3 else a[..., 0]


def _read(call, xy, pw, ph, like):
    """call(xy, pw, ph, d_out, out_cap) -> (status, stats); the patches as a numpy array shaped like S.expected's"""
    bpp = like.dtype.itemsize * (3 if like.ndim == 3 else 1)
    t = _tensor(len(xy), ph, pw, bpp)
    st, stats = call(xy, pw, ph, t.data_ptr(), len(xy) * ph * pw * bpp)
    return _pixels(t, len(xy), like), st, stats


def _file_call(mic, data, level):
    return lambda xy, pw, ph, d, cap: mic.wsi_read_patches(data, level, xy, pw, ph, d, cap)


def _touched(mic, sl, level, xy, pw, ph):
    lw, lh = sl["parsed"].levels[level][:2]
    return mic.wsi_patch_plan(lw, lh, S.TILE, S.TILE, xy, pw, ph)


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_patches_equal_the_padded_level_image(mic, slides, fmt):
    sl = slides[fmt]
    seen = set()
    for level, img in enumerate(sl["levels"]):
        lh, lw = img.shape[:2]
        first = sl["parsed"].levels[level][4]
        for pw, ph in PATCHES:
            xy = S.origins(lw, lh, S.TILE, S.TILE, pw, ph)
            got, st, stats = _read(_file_call(mic, sl["file"], level), xy, pw, ph, img)
            want = S.expected(img, xy, pw, ph)
            for i in range(len(xy)):
                assert np.array_equal(got[i], want[i]), (level, pw, ph, xy[i])
            assert (st == mic.MIC_OK).all()
            tiles, pieces = _touched(mic, sl, level, xy, pw, ph)
            assert stats["tiles_decoded"] == tiles.size and stats["pieces"] == pieces and stats["slabs"] >= 1
            for t in tiles:
                seen.update(sl["parsed"].modes(first + int(t)))
    assert {2, 3} <= seen and (0 in seen or 1 in seen), seen            # constant, stream and raw planes were all read
    if fmt != "rgb":
        assert {0, 1} <= seen, seen


def test_each_tile_is_decoded_once(mic, slides):
    sl = slides["rgb"]
    img = sl["levels"][0]
    inside = [(3 + i % 10, 2 + i // 10) for i in range(100)]            # 48 x 40 patches inside tile (0, 0)
    got, st, stats = _read(_file_call(mic, sl["file"], 0), inside, 48, 40, img)
    assert stats["tiles_decoded"] == 1 and stats["pieces"] == 100 and (st == 0).all()
    assert np.array_equal(got, S.expected(img, inside, 48, 40))
    same = [(40, 40)] * 5                                                # straddles four tiles, five times
    got, st, stats = _read(_file_call(mic, sl["file"], 0), same, 48, 40, img)
    assert stats["tiles_decoded"] == 4 and stats["pieces"] == 20 and (st == 0).all()
    for i in range(5):
        assert np.array_equal(got[i], got[0])
    assert np.array_equal(got[0], img[40:80, 40:88])


class _CountingSource:
    def __init__(self, data):
        self.data, self.reads = data, []

    def __call__(self, off, n):
        self.reads.append((off, n))
        return self.data[off: off + n]


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_three_front_doors_give_the_same_bytes(mic, slides, fmt):
    import torch
    sl = slides[fmt]
    f = sl["parsed"]
    level, (pw, ph) = 0, (48, 40)
    img = sl["levels"][level]
    xy = S.origins(img.shape[1], img.shape[0], S.TILE, S.TILE, pw, ph)
    base, st0, stats0 = _read(_file_call(mic, sl["file"], level), xy, pw, ph, img)
    assert np.array_equal(base, S.expected(img, xy, pw, ph))
    # the reader: after the header and index, exactly the blobs of the union's tiles, each byte once
    src = _CountingSource(sl["file"])
    with mic.WsiReader(src, len(sl["file"])) as rd:
        body = 48 + 20 * f.nlev + 16 * f.total
        assert sum(n for _, n in src.reads) == body
        src.reads.clear()
        got, st, stats = _read(lambda a, w, h, d, cap: rd.read_patches(level, a, w, h, d, cap), xy, pw, ph, img)
        reads = list(src.reads)
        oxy = S.origins(img.shape[1], img.shape[0], S.TILE, S.TILE, *ODD)
        odd, ost, _ = _read(lambda a, w, h, d, cap: rd.read_patches(level, a, w, h, d, cap), oxy, *ODD, img)
    assert np.array_equal(got, base) and np.array_equal(st, st0) and stats == stats0
    assert np.array_equal(odd, S.expected(img, oxy, *ODD)) and (ost == 0).all()
    tiles, _ = _touched(mic, sl, level, xy, pw, ph)
    offs = np.concatenate([[0], np.cumsum([len(b) for b in f.blobs])])
    want = np.zeros(len(sl["file"]), dtype=np.int32)
    for t in tiles:
        t = f.levels[level][4] + int(t)
        want[body + offs[t]: body + offs[t + 1]] += 1
    fetched = np.zeros_like(want)
    for off, n in reads:
        fetched[off: off + n] += 1
    assert np.array_equal(fetched, want)
    # the store: the same pixels through Session.wsi_encode; the coded slide stays on the device
    sess = mic.Session(64, S.TILE * S.TILE)
    try:
        d_px = torch.from_numpy(np.ascontiguousarray(sl["img"]).view(np.uint8).reshape(-1).copy()).cuda()
        sess.wsi_encode(d_px.data_ptr(), S.W, S.H, tile_w=S.TILE, tile_h=S.TILE, levels=S.LEVELS, **S.fmt_args(fmt))
        for lv in range(f.nlev):
            li = sl["levels"][lv]
            pts = S.origins(li.shape[1], li.shape[0], S.TILE, S.TILE, pw, ph)
            got, st, stats = _read(lambda a, w, h, d, cap: sess.wsi_read_patches(lv, a, w, h, d, cap), pts, pw, ph, li)
            assert np.array_equal(got, S.expected(li, pts, pw, ph)) and (st == 0).all(), lv
            if lv == level:
                assert np.array_equal(got, base) and stats == stats0
            # the odd width, and (level 0) one sub-batch that holds constant planes (the white and the black tile) beside streams
            # (the noise tile, the ramp).  The store keeps no mode bytes a test can read: that the white and the black tile are
            # constant planes there is inferred from their pixels (one value over the whole tile), not read back.  Raw planes:
            # the store has none -- it is written by the encoder, which never emits mode 3 here (see the module docstring) --
            # so mode 3 is the file door's to cover (test_patches_equal_the_padded_level_image).
            pts = S.origins(li.shape[1], li.shape[0], S.TILE, S.TILE, *ODD)
            if lv == 0:
                pts = pts + [(2 * S.TILE + 3, S.TILE + 5)]                # inside the white tile, which no origin of S.origins reaches
                tiles, _ = _touched(mic, sl, 0, pts, *ODD)
                assert {S.NOISE_TILE, S.WHITE_TILE, S.BLACK_TILE} <= set(int(t) for t in tiles)
            got, st, stats = _read(lambda a, w, h, d, cap: sess.wsi_read_patches(lv, a, w, h, d, cap), pts, *ODD, li)
            assert np.array_equal(got, S.expected(li, pts, *ODD)) and (st == 0).all(), lv
            if lv == 0:
                assert stats["slabs"] == 1 and stats["tiles_decoded"] == tiles.size
    finally:
        sess.close()


def test_the_gather_kernel_is_timed_under_its_name(mic, slides):
    import torch
    sl = slides["grey16"]
    sess = mic.Session(64, S.TILE * S.TILE)
    try:
        d_px = torch.from_numpy(np.ascontiguousarray(sl["img"]).view(np.uint8).reshape(-1).copy()).cuda()
        sess.wsi_encode(d_px.data_ptr(), S.W, S.H, tile_w=S.TILE, tile_h=S.TILE, levels=S.LEVELS, **S.fmt_args("grey16"))
        sess.set_timing(True)
        _read(lambda a, w, h, d, cap: sess.wsi_read_patches(0, a, w, h, d, cap), [(0, 0), (40, 40)], 48, 40, sl["levels"][0])
        assert "k_wsi_gather_patches" in dict(sess.last_timings())
    finally:
        sess.close()


def test_slabs_under_a_small_workspace(mic, slides):
    """A child process with an 8 MB workspace ceiling: a sub-batch of the unit codec then holds six 64 x 64 RGB tiles (about 0.42 MB
    of tier-1 slabs per plane), so the twelve tiles of level 0 take two slabs.  The bytes must be those of the unconstrained call,
    and decompress_wsi_level of the same file must succeed under the same ceiling.  The store door cuts by the same figure: its
    ceiling is the smaller of that workspace bound and of what a 16 GB plane slab holds (far more tiles than twelve), so under 8 MB
    it reports the file door's slab count for the same twelve tiles."""
    sl = slides["rgb"]
    xy = [(x, y) for y in range(-10, S.H, 45) for x in range(-10, S.W, 55)]
    want, st, stats = _read(_file_call(mic, sl["file"], 0), xy, 48, 40, sl["levels"][0])
    assert stats["tiles_decoded"] == 12 and (st == 0).all()
    code = r'''
import sys, hashlib, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import __graft_entry__ as e
mic = e.load_package()
import wsi_patch_slides as S
img, data = S.make_file(mic, "rgb")
assert np.array_equal(mic.decompress_wsi_level(data, 0), img)
xy = %r
t = torch.full((len(xy), 40, 48, 3), 0xA5, dtype=torch.uint8, device="cuda")
st, stats = mic.wsi_read_patches(data, 0, xy, 48, 40, t.data_ptr(), t.numel())
assert (st == 0).all() and stats["tiles_decoded"] == 12 and stats["slabs"] >= 2, stats
got = t.cpu().numpy()
assert np.array_equal(got, S.expected(img, xy, 48, 40))
sess = mic.Session(64, S.TILE * S.TILE)
d_px = torch.from_numpy(img.reshape(-1).copy()).cuda()
sess.wsi_encode(d_px.data_ptr(), S.W, S.H, tile_w=S.TILE, tile_h=S.TILE, levels=S.LEVELS, **S.fmt_args("rgb"))
t2 = torch.full((len(xy), 40, 48, 3), 0xA5, dtype=torch.uint8, device="cuda")
st2, stats2 = sess.wsi_read_patches(0, xy, 48, 40, t2.data_ptr(), t2.numel())
sess.close()
assert (st2 == 0).all() and stats2["tiles_decoded"] == 12, stats2
assert stats2["slabs"] == stats["slabs"] and stats2["slabs"] >= 2, (stats2, stats)
assert np.array_equal(t2.cpu().numpy(), S.expected(img, xy, 48, 40))
print("ok", hashlib.sha256(got.tobytes()).hexdigest())
''' % (ROOT, os.path.join(ROOT, "tests"), xy)
    env = dict(os.environ, MIC_HIP_WS_BUDGET_MB="8")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    import hashlib
    assert r.returncode == 0 and ("ok " + hashlib.sha256(np.ascontiguousarray(want).tobytes()).hexdigest()) in r.stdout, r.stdout + r.stderr


def _tile_code(mic, data, level, tx, ty):
    try:
        return mic.MIC_OK, mic.decompress_wsi_tile(data, level, tx, ty)
    except mic.MicError as e:
        return e.code, None


# (a greyscale blob has no plane lengths -- the blob is the plane -- so the third damage is the RGB slide's alone)
DAMAGE = [("rgb", "mode byte 9"), ("rgb", "flipped stream byte"), ("rgb", "zero plane length"),
          ("grey8", "mode byte 9"), ("grey8", "flipped stream byte")]


@pytest.mark.parametrize("fmt,damage", DAMAGE)
def test_a_damaged_tile_fails_its_patches_only(mic, slides, fmt, damage):
    sl = slides[fmt]
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
    code, px = _tile_code(mic, data, 0, tile % 4, tile // 4)
    if damage != "flipped stream byte":
        assert code == mic.MIC_ERR_CORRUPT
    img = sl["levels"][0]
    if code == mic.MIC_OK:                                                # the flipped stream still decodes: to these pixels
        img = img.copy()
        img[(tile // 4) * 64: (tile // 4) * 64 + px.shape[0], (tile % 4) * 64: (tile % 4) * 64 + px.shape[1]] = px
    pw, ph = 48, 40
    xy = S.origins(S.W, S.H, S.TILE, S.TILE, pw, ph)
    got, st, stats = _read(_file_call(mic, data, 0), xy, pw, ph, img)
    want = S.expected(img, xy, pw, ph)
    hit = 0
    for i, o in enumerate(xy):
        touches = tile in _touched(mic, sl, 0, [o], pw, ph)[0]
        hit += touches
        assert st[i] == (code if touches else mic.MIC_OK), (o, st[i])
        if not touches or code == mic.MIC_OK:
            assert np.array_equal(got[i], want[i]), o
    assert 0 < hit < len(xy)


def test_argument_errors_come_back_before_any_launch(mic, slides):
    import torch
    sl = slides["rgb"]
    t = _tensor(2, 40, 48, 3)
    xy = [(0, 0), (10, 10)]
    cap = 2 * 40 * 48 * 3
    sess = mic.Session(64, S.TILE * S.TILE)
    d_px = torch.from_numpy(sl["img"].reshape(-1).copy()).cuda()
    sess.wsi_encode(d_px.data_ptr(), S.W, S.H, tile_w=S.TILE, tile_h=S.TILE, levels=S.LEVELS)
    rd = mic.WsiReader(sl["file"])
    doors = [lambda lv, a, w, h, d, c: mic.wsi_read_patches(sl["file"], lv, a, w, h, d, c),
             lambda lv, a, w, h, d, c: rd.read_patches(lv, a, w, h, d, c),
             lambda lv, a, w, h, d, c: sess.wsi_read_patches(lv, a, w, h, d, c)]
    try:
        for door in doors:
            for args, want in [((S.LEVELS, xy, 48, 40, t.data_ptr(), cap), mic.MIC_ERR_ARGS), ((-1, xy, 48, 40, t.data_ptr(), cap), mic.MIC_ERR_ARGS),
                               ((0, xy, 0, 40, t.data_ptr(), cap), mic.MIC_ERR_ARGS), ((0, xy, 48, -1, t.data_ptr(), cap), mic.MIC_ERR_ARGS),
                               ((0, xy, 48, 40, t.data_ptr(), cap - 1), mic.MIC_ERR_CAPACITY)]:
                with pytest.raises(mic.MicError) as e:
                    door(*args)
                assert e.value.code == want, args
            st, stats = door(0, [], 48, 40, t.data_ptr(), 0)              # n = 0: nothing to do, and that is no error
            assert st.size == 0 and stats == dict(tiles_decoded=0, pieces=0, slabs=0)
        assert (t.cpu().numpy() == 0xA5).all()                            # none of these calls wrote a byte
        st, stats = doors[0](0, xy, 48, 40, t.data_ptr(), cap)            # ... and the tensor was a good one
        assert (st == 0).all() and np.array_equal(t.cpu().numpy(), S.expected(sl["levels"][0], xy, 48, 40))
    finally:
        rd.close()
        sess.close()
