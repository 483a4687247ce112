"""MIC3 streaming (csrc/mic_api_ext.hip: mic_hip_wsi_writer_*, mic_hip_wsi_reader_*).  The writer takes a slide's rows in pushes of
any size and must hand its sink the file compress_wsi (and the reference) writes, byte for byte, whatever the push schedule and
band size; level-0 tiles reach the sink as soon as their band is coded.  The reader pulls the header and index through a callback
and then only the blobs of the tiles a decode covers, and must return what the flat-buffer decodes return."""
import io
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (format, width, height, tile_w, tile_h, levels): the cases of test_gpu_multi_device_wsi plus levels = 1 and small odd slides
CASES = [
    ("rgb", 2050, 1999, 256, 256, 0),
    ("rgb", 1201, 777, 128, 96, 0),
    ("rgb", 999, 1500, 160, 97, 0),
    ("rgb", 700, 300, 256, 256, 0),
    ("rgb", 3001, 600, 256, 255, 0),
    ("rgb", 1501, 1203, 256, 256, 2),
    ("rgb", 333, 517, 64, 64, 1),
    ("grey8", 1537, 2305, 256, 256, 3),
    ("grey8", 640, 2600, 200, 100, 2),
    ("grey8", 641, 599, 200, 97, 0),
    ("grey16", 777, 1999, 100, 100, 4),
    ("grey16", 901, 1203, 256, 256, 0),
]


def _slide(synth, fmt, w, h, seed):
    if fmt == "rgb":
        grain = np.random.default_rng(seed).integers(-6, 7, (h, w, 3))
        return np.clip(synth.wsi_like(w, h, seed=seed).astype(np.int32) + grain, 0, 255).astype(np.uint8)
    from test_oracle_wavelet_wsi import _grey_slide
    return _grey_slide(synth, w, h, 16 if fmt == "grey16" else 8, seed=seed)


def _fmt_args(fmt):
    return dict(channels=3, bits_per_sample=8) if fmt == "rgb" else dict(channels=1, bits_per_sample=16 if fmt == "grey16" else 8)


def _oracle(mico, fmt, img, tw, th, levels):
    rc, want = mico.wsi_compress(img, tw, th, levels) if fmt == "rgb" else mico.wsi_compress_grey(img, tw, th, levels)
    assert rc == 0
    return want


def _schedules(h, th, seed):
    rng = random.Random(seed)
    out = {"7": [7], "37": [37], "tile_h": [th], "tile_h+1": [th + 1], "whole": [h]}
    rnd = []
    left = h
    while left > 0:
        rnd.append(min(left, rng.randint(1, 3 * th)))
        left -= rnd[-1]
    out["random"] = rnd
    if h <= 600:
        out["1"] = [1]
    return out


def _stream(mic, img, fmt, w, h, tw, th, levels, band, sched):
    """sched: a list of push sizes, repeated (its last entry) until the slide is in"""
    sink = io.BytesIO()
    with mic.WsiWriter(sink, w, h, tile_w=tw, tile_h=th, levels=levels, band_tile_rows=band, **_fmt_args(fmt)) as wr:
        y, i = 0, 0
        while y < h:
            n = min(h - y, sched[min(i, len(sched) - 1)])
            wr.push(img[y: y + n])
            y += n
            i += 1
        n = wr.finish()
    data = sink.getvalue()
    assert len(data) == n
    return data


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-t{c[3]}x{c[4]}-l{c[5]}" for c in CASES])
def test_stream_equals_oracle(mic, mico, synth, gpu_ready, case):
    fmt, w, h, tw, th, levels = case
    img = _slide(synth, fmt, w, h, seed=w % 11 + 5)
    want = _oracle(mico, fmt, img, tw, th, levels)
    assert mic.compress_wsi(img, w, h, tile_w=tw, tile_h=th, levels=levels, **_fmt_args(fmt)) == want
    for name, sched in _schedules(h, th, seed=w + h).items():
        for band in (0, 1, 3):
            if name in ("1", "7") and band != 1:
                continue
            assert _stream(mic, img, fmt, w, h, tw, th, levels, band, sched) == want, (name, band)


def test_tall_slide_and_device_bytes_do_not_depend_on_height(mic, synth, gpu_ready):
    w, h = 1536, 30000
    rng = np.random.default_rng(7)
    img = np.clip(synth.wsi_like(w, 3000, seed=3)[:, :, 1].astype(np.int32)[np.arange(h) % 3000] + rng.integers(-3, 4, (h, w)),
                  0, 255).astype(np.uint8)
    want = mic.compress_wsi(img, w, h, channels=1, bits_per_sample=8)
    for band in (2, 0):
        got = _stream(mic, img, "grey8", w, h, 0, 0, 0, band, [999])
        assert got == want, band
        with mic.WsiWriter(io.BytesIO(), w, h, channels=1, band_tile_rows=band) as tall, \
                mic.WsiWriter(io.BytesIO(), w, 3000, channels=1, band_tile_rows=band) as short:
            assert tall.device_bytes == short.device_bytes > 0, band


class _Recorder:
    def __init__(self):
        self.buf = bytearray()
        self.writes = []

    def __call__(self, off, data):
        end = off + len(data)
        if len(self.buf) < end:
            self.buf.extend(b"\0" * (end - len(self.buf)))
        self.buf[off:end] = bytes(data)
        self.writes.append((off, len(data)))


def test_level0_tiles_reach_the_sink_as_their_band_is_coded(mic, mico, synth, gpu_ready):
    w, h, tw, th = 1201, 777, 128, 96
    img = _slide(synth, "rgb", w, h, seed=9)
    want = mic.compress_wsi(img, w, h, tile_w=tw, tile_h=th)
    hdr = mic.read_wsi_header(want)
    nl, total = len(hdr["levels"]), hdr["total_tiles"]
    data_off = 48 + 20 * nl + 16 * total
    idx = [(int.from_bytes(want[48 + 20 * nl + 16 * t: 56 + 20 * nl + 16 * t], "little"),
            int.from_bytes(want[56 + 20 * nl + 16 * t: 64 + 20 * nl + 16 * t], "little")) for t in range(total)]
    tx = hdr["levels"][0]["tiles_x"]
    rec = _Recorder()
    wr = mic.WsiWriter(rec, w, h, tile_w=tw, tile_h=th, band_tile_rows=1)
    y = 0
    for n in (50, 130, 96, 1, 300, 200):
        wr.push(img[y: y + n])
        y += n
        assert all(off >= data_off for off, _ in rec.writes), "header or index written before finish"
        for ty in range(y // th):
            for t in range(ty * tx, (ty + 1) * tx):
                bo, bl = idx[t]
                assert bytes(rec.buf[data_off + bo: data_off + bo + bl]) == want[data_off + bo: data_off + bo + bl], (y, t)
    assert y == h
    assert wr.finish() == len(want)
    assert bytes(rec.buf) == want
    wr.close()


def test_errors(mic, synth, gpu_ready):
    w, h = 300, 200
    img = _slide(synth, "rgb", w, h, seed=2)
    want = mic.compress_wsi(img, w, h, tile_w=64, tile_h=64)
    sink = io.BytesIO()
    wr = mic.WsiWriter(sink, w, h, tile_w=64, tile_h=64)
    wr.push(img[:150])
    with pytest.raises(mic.MicError) as e:
        wr.push(img[:51])                                   # past height: consumes nothing
    assert e.value.code == mic.MIC_ERR_ARGS
    with pytest.raises(mic.MicError) as e:
        wr.finish()
    assert e.value.code == mic.MIC_ERR_ARGS
    wr.push(img[150:])
    assert wr.finish() == len(want) and sink.getvalue() == want
    wr.close()

    # a sink that fails on its 2nd write: MIC_ERR_IO, sticky
    calls = []

    def bad(off, data):
        calls.append(off)
        if len(calls) == 2:
            raise OSError("disk full")
    wr = mic.WsiWriter(bad, w, h, tile_w=64, tile_h=64, band_tile_rows=1)
    with pytest.raises(OSError):
        for y in range(0, h, 64):
            wr.push(img[y: y + 64])
    with pytest.raises(mic.MicError) as e:
        wr.push(img[:1])
    assert e.value.code == mic.MIC_ERR_IO
    with pytest.raises(mic.MicError) as e:
        wr.finish()
    assert e.value.code == mic.MIC_ERR_IO
    wr.close()

    # a sink that returns non-zero through the C ABI's convention
    wr = mic.WsiWriter(lambda off, data: 5, w, h, tile_w=64, tile_h=64, band_tile_rows=1)
    with pytest.raises(mic.MicError) as e:
        wr.push(img)
    assert e.value.code == mic.MIC_ERR_IO
    wr.close()

    with pytest.raises(mic.MicError) as e:
        mic.WsiWriter(io.BytesIO(), w, h, channels=3, bits_per_sample=16)
    assert e.value.code == mic.MIC_ERR_UNSUPPORTED


def test_writers_interleave_with_other_calls(mic, mico, synth, gpu_ready):
    a = _slide(synth, "rgb", 1201, 777, seed=4)
    b = _slide(synth, "grey16", 777, 999, seed=6)
    want_a = _oracle(mico, "rgb", a, 128, 96, 0)
    want_b = _oracle(mico, "grey16", b, 100, 100, 4)
    sa, sb = io.BytesIO(), io.BytesIO()
    wa = mic.WsiWriter(sa, 1201, 777, tile_w=128, tile_h=96, band_tile_rows=1)
    wb = mic.WsiWriter(sb, 777, 999, channels=1, bits_per_sample=16, tile_w=100, tile_h=100, levels=4, band_tile_rows=2)
    ya = yb = 0
    while ya < 777 or yb < 999:
        if ya < 777:
            wa.push(a[ya: ya + 100]); ya = min(777, ya + 100)
        if yb < 999:
            wb.push(b[yb: yb + 130]); yb = min(999, yb + 130)
        assert mic.compress_wsi(a, 1201, 777, tile_w=128, tile_h=96) == want_a
        assert np.array_equal(mic.decompress_wsi_region(want_a, 0, 100, 50, 300, 200), a[50:250, 100:400])
    wa.finish(); wb.finish()
    wa.close(); wb.close()
    assert sa.getvalue() == want_a and sb.getvalue() == want_b


def test_stream_under_two_listed_devices(mic, synth, gpu_ready):
    img = _slide(synth, "rgb", 999, 1500, seed=8)
    want = mic.compress_wsi(img, 999, 1500, tile_w=160, tile_h=97)
    mic.set_devices([0, 0])
    try:
        assert _stream(mic, img, "rgb", 999, 1500, 160, 97, 0, 0, [500]) == want
    finally:
        mic.set_devices([0])


class _Counting:
    def __init__(self, data):
        self.data = data
        self.read = 0
        self.fail = False

    def __call__(self, off, n):
        if self.fail:
            raise OSError("gone")
        self.read += n
        return self.data[off: off + n]


@pytest.mark.parametrize("fmt,w,h,tw,th,lv", [("rgb", 2050, 1999, 256, 256, 0), ("grey16", 777, 1999, 100, 100, 4),
                                               ("rgb", 999, 1500, 160, 97, 0)])
def test_reader_matches_flat_decodes(mic, synth, gpu_ready, fmt, w, h, tw, th, lv):
    img = _slide(synth, fmt, w, h, seed=12)
    data = mic.compress_wsi(img, w, h, tile_w=tw, tile_h=th, levels=lv, **_fmt_args(fmt))
    hdr = mic.read_wsi_header(data)
    src = _Counting(data)
    try:
        for devs in ([0], [0, 0]):
            mic.set_devices(devs)
            with mic.WsiReader(src, len(data)) as r:
                for lvl, L in enumerate(hdr["levels"]):
                    for tx, ty in {(0, 0), (L["tiles_x"] - 1, L["tiles_y"] - 1), (L["tiles_x"] // 2, 0)}:
                        assert np.array_equal(r.tile(lvl, tx, ty), mic.decompress_wsi_tile(data, lvl, tx, ty)), (lvl, tx, ty)
                    for x, y, rw, rh in ((0, 0, L["width"], L["height"]), (3, th - 5, 2 * tw + 9, 2 * th + 10),
                                         (L["width"] // 2, L["height"] // 2, 10 * L["width"], 10 * L["height"])):
                        if x >= L["width"] or y >= L["height"]:
                            continue
                        assert np.array_equal(r.region(lvl, x, y, rw, rh), mic.decompress_wsi_region(data, lvl, x, y, rw, rh)), \
                            (devs, lvl, x, y)
    finally:
        mic.set_devices([0])
    # a region reads the index and the covered tiles' blobs, nothing more
    nl, total = len(hdr["levels"]), hdr["total_tiles"]
    head = 48 + 20 * nl + 16 * total
    src = _Counting(data)
    r = mic.WsiReader(src, len(data))
    assert src.read == head
    x, y, rw, rh = tw + 3, th + 7, tw + 20, th + 1
    r.region(0, x, y, rw, rh)
    tx_n = hdr["levels"][0]["tiles_x"]
    blob = 0
    for ty in range(y // th, (y + rh - 1) // th + 1):
        for tx in range(x // tw, (x + rw - 1) // tw + 1):
            t = ty * tx_n + tx
            blob += int.from_bytes(data[56 + 20 * nl + 16 * t: 64 + 20 * nl + 16 * t], "little")
    assert src.read - head <= blob
    src.fail = True
    with pytest.raises(OSError):
        r.tile(0, 0, 0)
    r.close()


def test_reader_status_codes(mic, synth, gpu_ready):
    w, h = 700, 300
    img = _slide(synth, "rgb", w, h, seed=3)
    data = bytearray(mic.compress_wsi(img, w, h))
    nl = int.from_bytes(data[28:30], "little")
    total = int.from_bytes(data[32:40], "little")
    # the last tile's blob pointed past the end of the file: only the decode that needs it fails
    e = 48 + 20 * nl + 16 * (total - 1)
    data[e: e + 8] = (len(data)).to_bytes(8, "little")
    r = mic.WsiReader(bytes(data))
    assert r.tile(0, 0, 0).shape == (256, 256, 3)
    with pytest.raises(mic.MicError) as ex:
        r.tile(nl - 1, 0, 0)
    assert ex.value.code == mic.MIC_ERR_CORRUPT
    r.close()

    lib = mic.lib()
    cb = mic._READ_FN(lambda user, off, ptr, n: 1)
    import ctypes as C
    h_ = C.c_void_p()
    assert lib.mic_hip_wsi_reader_open(cb, None, len(data), C.byref(h_)) == mic.MIC_ERR_IO
