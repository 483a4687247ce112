"""mic_hip_wsi_band_plan (csrc/mic_api_ext.hip): the bands of tile rows mic_hip_wsi_compress_ex cuts a slide into, one per device of
mic_hip_set_devices.  It must be parallel.wsi_band_plan -- the plan dist_compress_wsi runs over torch.distributed ranks -- so that
the library and the multi-process path cut a slide the same way.  Pure host logic: no GPU."""
import ctypes as C
import importlib

import pytest

HEIGHTS = [1, 2, 3, 63, 64, 65, 99, 100, 101, 255, 256, 257, 511, 512, 513, 767, 1000, 1023, 1024, 1025, 2047, 2048, 3000, 4095,
           4096, 4097, 8191, 8192, 10007, 16384, 20000, 32767, 32768, 32769, 50000, 65535, 65536, 69999, 70000]
TILE_H = [64, 100, 255, 256]
LEVELS = [0, 1, 2, 4, 7, 12]
WIDTHS = [1, 333, 40000]


@pytest.fixture(scope="module")
def par(mic):
    return importlib.import_module("medical_image_codec_amd.parallel")


def test_plan_equals_the_python_plan(mic, par):
    n = 0
    for width in WIDTHS:
        for height in HEIGHTS:
            for th in TILE_H:
                for req in LEVELS:
                    L = len(par.wsi_levels(width, height, 256, th, req))
                    for shards in range(1, 10):
                        k, first = mic.wsi_band_plan(width, height, 256, th, req, shards)
                        wk, bands = par.wsi_band_plan(height, th, L, shards)
                        assert k == wk, (width, height, th, req, shards)
                        assert [(a, b) for a, b in zip(first, first[1:])] == bands, (width, height, th, req, shards)
                        n += 1
    assert n == len(WIDTHS) * len(HEIGHTS) * len(TILE_H) * len(LEVELS) * 9


def test_bands_tile_the_slide_in_whole_blocks(mic, par):
    for height in HEIGHTS:
        for th in TILE_H:
            for req in (0, 3):
                L = len(par.wsi_levels(5000, height, 256, th, req))
                for shards in range(1, 10):
                    k, first = mic.wsi_band_plan(5000, height, 256, th, req, shards)
                    assert 0 <= k <= L - 1
                    assert len(first) == shards + 1 and first[0] == 0 and first[-1] == height
                    assert all(a <= b for a, b in zip(first, first[1:]))
                    # every band but the last holds whole tiles of levels 0..K: a multiple of tile_h << K rows
                    assert all((b - a) % (th << k) == 0 for a, b in zip(first[:-1], first[1:-1]))
                    # K is the top level that still leaves every shard a block of its own (or level 0)
                    nb = -(-height // (th << k))
                    assert k == 0 or nb >= shards
                    if k < L - 1:
                        assert -(-height // (th << (k + 1))) < shards


def test_defaults_match_explicit_arguments(mic):
    assert mic.wsi_band_plan(30000, 30000, 0, 0, 0, 8) == mic.wsi_band_plan(30000, 30000, 256, 256, 0, 8)
    assert mic.wsi_band_plan(30000, 30000, 0, 0, -3, 5) == mic.wsi_band_plan(30000, 30000, 256, 256, 0, 5)


def test_bad_arguments(mic):
    for args in ((0, 100, 256, 256, 0, 2), (100, 0, 256, 256, 0, 2), (-1, 100, 256, 256, 0, 2), (100, 100, -1, 256, 0, 2),
                 (100, 100, 256, -5, 0, 2), (100, 100, 256, 256, 0, 0), (100, 100, 256, 256, 0, -1), (100, 100, 256, 256, 33, 2)):
        with pytest.raises(mic.MicError) as e:
            mic.wsi_band_plan(*args)
        assert e.value.code == mic.MIC_ERR_ARGS, args
    first = (C.c_int * 3)()
    assert mic.lib().mic_hip_wsi_band_plan(100, 100, 256, 256, 0, 2, None, first) == mic.MIC_ERR_ARGS
    kk = C.c_int()
    assert mic.lib().mic_hip_wsi_band_plan(100, 100, 256, 256, 0, 2, C.byref(kk), None) == mic.MIC_ERR_ARGS
