"""The MIC3 streaming reader's open / info and the writer's argument checks need no device (csrc/mic_api_ext.hip:
mic_hip_wsi_reader_open validates the header, level table and tile index it pulls through the callback as parse_mic3 does)."""
import ctypes as C

import numpy as np
import pytest


def _file(mico, synth, w=1201, h=777, tw=128, th=96, levels=0):
    grain = np.random.default_rng(5).integers(-6, 7, (h, w, 3))     # (smooth small tiles are what the reference's normaliser gives up on)
    img = np.clip(synth.wsi_like(w, h, seed=5).astype(np.int32) + grain, 0, 255).astype(np.uint8)
    rc, data = mico.wsi_compress(img, tw, th, levels)
    assert rc == 0
    return data


class _Counting:
    def __init__(self, data):
        self.data, self.read, self.calls = data, 0, 0

    def __call__(self, off, n):
        self.read += n
        self.calls += 1
        return self.data[off: off + n]


def test_open_and_info_give_the_header(mic, mico, synth):
    data = _file(mico, synth)
    hdr = mic.read_wsi_header(data)
    src = _Counting(data)
    with mic.WsiReader(src, len(data)) as r:
        assert r.info == dict(width=1201, height=777, tile_width=128, tile_height=96, levels=len(hdr["levels"]),
                              channels=3, bits_per_sample=8)
    nl, total = len(hdr["levels"]), hdr["total_tiles"]
    assert src.read == 48 + 20 * nl + 16 * total
    with mic.WsiReader(data) as r:                           # bytes
        assert r.info["levels"] == nl


def test_grey_file_info(mic, mico, synth):
    from test_oracle_wavelet_wsi import _grey_slide
    img = _grey_slide(synth, 200, 150, 16, seed=2)
    rc, data = mico.wsi_compress_grey(img, 64, 64, 2)
    assert rc == 0
    r = mic.WsiReader(data)
    assert r.info == dict(width=200, height=150, tile_width=64, tile_height=64, levels=2, channels=1, bits_per_sample=16)
    r.close()


def test_open_rejects_corrupt_headers(mic, mico, synth):
    data = _file(mico, synth)
    nl = int.from_bytes(data[28:30], "little")
    total = int.from_bytes(data[32:40], "little")
    head = 48 + 20 * nl + 16 * total
    cases = {
        "truncated": (data, head - 1),
        "short": (data, 40),
        "magic": (b"MIC4" + data[4:], len(data)),
        "tiles_x": (data[:48 + 8] + (99).to_bytes(4, "little") + data[48 + 12:], len(data)),   # level 0's tile count is not ceil(w / tw)
        "first": (data[:48 + 20 * (nl - 1) + 16] + (total).to_bytes(4, "little") + data[48 + 20 * (nl - 1) + 20:], len(data)),
    }
    for name, (blob, n) in cases.items():
        with pytest.raises(mic.MicError) as e:
            mic.WsiReader(blob, n)
        assert e.value.code == mic.MIC_ERR_CORRUPT, name
        assert mic.lib().mic_hip_wsi_info(np.frombuffer(blob, np.uint8).ctypes.data, n, None, None, None, None, None, None) \
            == mic.MIC_ERR_CORRUPT, name


def test_open_reports_a_failing_callback(mic, mico, synth):
    data = _file(mico, synth)

    def gone(off, n):
        raise OSError("unreadable")
    with pytest.raises(OSError):
        mic.WsiReader(gone, len(data))
    h = C.c_void_p()
    cb = mic._READ_FN(lambda user, off, ptr, n: -1)
    assert mic.lib().mic_hip_wsi_reader_open(cb, None, len(data), C.byref(h)) == mic.MIC_ERR_IO
    assert not h.value


def test_writer_arguments_are_checked_without_a_device(mic):
    h = C.c_void_p()
    cb = mic._WRITE_FN(lambda user, off, ptr, n: 0)
    L = mic.lib()
    for args in ((0, 10, 3, 8, 0, 0, 0, 0), (10, -1, 3, 8, 0, 0, 0, 0), (10, 10, 3, 8, -1, 0, 0, 0), (10, 10, 3, 8, 0, 0, 0, -2)):
        assert L.mic_hip_wsi_writer_open(*args, cb, None, C.byref(h)) == mic.MIC_ERR_ARGS, args
    assert L.mic_hip_wsi_writer_open(10, 10, 3, 8, 0, 0, 0, 0, C.cast(None, mic._WRITE_FN), None, C.byref(h)) == mic.MIC_ERR_ARGS
    for ch, bps in ((3, 16), (2, 8), (1, 12), (4, 8)):
        assert L.mic_hip_wsi_writer_open(10, 10, ch, bps, 0, 0, 0, 0, cb, None, C.byref(h)) == mic.MIC_ERR_UNSUPPORTED, (ch, bps)
    assert L.mic_hip_wsi_writer_open(10, 10, 3, 8, 1 << 14, 1 << 14, 0, 0, cb, None, C.byref(h)) == mic.MIC_ERR_UNSUPPORTED
    assert L.mic_hip_wsi_writer_open(10, 10, 1, 8, 0, 0, 33, 0, cb, None, C.byref(h)) == mic.MIC_ERR_UNSUPPORTED
    with pytest.raises(mic.MicError) as e:
        mic.WsiWriter(lambda off, data: None, 100, 100, channels=3, bits_per_sample=16)
    assert e.value.code == mic.MIC_ERR_UNSUPPORTED
