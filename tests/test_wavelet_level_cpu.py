"""WaveletV2 at reduced resolution, the host-only part: mic_hip_wavelet_v2_level_info (csrc/mic_wavelet.hip) gives the size of the
image at level r -- nr[0] = rows, nr[l + 1] = (nr[l] + 1) // 2, cols alike -- for 0 <= r <= the header's level count, and the error
codes of the level entry points.  Needs no device."""
import numpy as np
import pytest

import wavelet_ref as W

from test_gpu_wavelet_seams import TILING


def _applied(rows, cols, levels):
    """the level count the encoder writes (waveletfsecompressu16.go:321-330)"""
    r, c, a = rows, cols, 0
    while a < min(max(levels, 1), 8) and r >= 2 and c >= 2:
        r, c, a = (r + 1) // 2, (c + 1) // 2, a + 1
    return a


def _dims(rows, cols, levels):
    nr, nc = [rows], [cols]
    for _ in range(levels):
        nr.append((nr[-1] + 1) // 2)
        nc.append((nc[-1] + 1) // 2)
    return nr, nc


def _file(rows, cols, levels, tail=b"\xff\x04"):
    return W.header(rows, cols, 4095, levels) + tail


@pytest.mark.parametrize("rows,cols,levels,depth", TILING)
def test_level_info_is_the_band_size_at_every_level(mic, rows, cols, levels, depth):
    applied = _applied(rows, cols, levels)
    f = _file(rows, cols, applied)
    nr, nc = _dims(rows, cols, applied)
    for r in range(applied + 1):
        assert mic.wavelet_v2_level_info(f, r) == (nr[r], nc[r]), (rows, cols, r)
        _, got = W.forward(np.zeros((rows, cols), np.uint16), r)              # (the stop rule agrees)
        assert r == 0 or got == r
    for bad in (-1, applied + 1, 9):
        with pytest.raises(mic.MicError) as e:
            mic.wavelet_v2_level_info(f, bad)
        assert e.value.code == mic.MIC_ERR_ARGS, (rows, cols, bad)


def test_a_short_header_is_corrupt(mic):
    for n in (0, 1, 10):
        with pytest.raises(mic.MicError) as e:
            mic.wavelet_v2_level_info(bytes(n) + b"", 0)
        assert e.value.code == mic.MIC_ERR_CORRUPT, n


def test_headers_that_describe_no_image_are_corrupt(mic):
    for rows, cols, levels in ((0, 5, 1), (5, 0, 1), (64, 64, 9)):
        with pytest.raises(mic.MicError) as e:
            mic.wavelet_v2_level_info(_file(rows, cols, levels), 0)
        assert e.value.code == mic.MIC_ERR_CORRUPT, (rows, cols, levels)


def test_a_header_with_no_levels_admits_only_level_zero(mic):
    f = _file(700, 1, 0)
    assert mic.wavelet_v2_level_info(f, 0) == (700, 1)
    with pytest.raises(mic.MicError) as e:
        mic.wavelet_v2_level_info(f, 1)
    assert e.value.code == mic.MIC_ERR_ARGS


def test_the_entry_points_check_their_arguments_before_the_device(mic):
    """out-of-range levels and short headers are refused by the host before any launch"""
    L = mic.lib()
    f = np.frombuffer(_file(64, 48, 3), dtype=np.uint8)
    out = np.zeros(64 * 48, dtype=np.uint16)
    for lvl in (-1, 4):
        assert L.mic_hip_wavelet_v2_decompress_level(f.ctypes.data, f.size, lvl, out.ctypes.data, out.size) == mic.MIC_ERR_ARGS
    assert L.mic_hip_wavelet_v2_decompress_level(f.ctypes.data, 10, 0, out.ctypes.data, out.size) == mic.MIC_ERR_CORRUPT
    assert L.mic_hip_wavelet_v2_decompress_level(f.ctypes.data, f.size, 0, None, out.size) == mic.MIC_ERR_ARGS
