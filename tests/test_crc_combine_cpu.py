"""CPU tests of mic_hip_crc32_combine (no device): the fold the PICS doors join their strips' CRC-32s with, against zlib.crc32."""
import zlib

import numpy as np
import pytest


def _bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("len_a", [0, 1, 7])
@pytest.mark.parametrize("len_b", [0, 1, 2, 3, 4, 5, 63, 64, 65, 4095, 4096, 1048577])
def test_combine_equals_zlib_of_the_concatenation(mic, len_a, len_b):
    a, b = _bytes(len_a, 1 + len_a), _bytes(len_b, 100 + len_b)
    assert mic.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b)


def test_combine_is_associative_at_lengths_that_cannot_be_hashed(mic):
    ca, cb, cc = zlib.crc32(b"first part"), zlib.crc32(b"second"), zlib.crc32(b"the third part")
    lens = [0, 1, 5, 4096, (1 << 32) - 1, 1 << 32, (1 << 40) + 3]
    for l1 in lens:
        for l2 in lens:
            left = mic.crc32_combine(mic.crc32_combine(ca, cb, l1), cc, l2)
            right = mic.crc32_combine(ca, mic.crc32_combine(cb, cc, l2), l1 + l2)
            assert left == right, (l1, l2)
    # ... and agrees with zlib where zlib can say: a long run of zero bytes, hashed piecewise
    zeros = bytes(1 << 20)
    four = 0
    for _ in range(4):
        four = zlib.crc32(zeros, four)
    assert mic.crc32_combine(ca, four, 4 << 20) == zlib.crc32(zeros, zlib.crc32(zeros, zlib.crc32(zeros, zlib.crc32(zeros, ca))))


@pytest.mark.parametrize("strips", [1, 3, 8])
def test_strip_fold_of_an_image_cut_as_pics_cuts_it(mic, synth, strips):
    w, h = 173, 211
    img = synth.xr_like(cols=w, rows=h, depth=12, seed=5)
    strip_h = (h + strips - 1) // strips                       # parallelstrips.go:70-72
    actual = (h + strip_h - 1) // strip_h
    crc = None
    for k in range(actual):
        part = img[k * strip_h:min(h, (k + 1) * strip_h)].astype("<u2").tobytes()
        crc = zlib.crc32(part) if crc is None else mic.crc32_combine(crc, zlib.crc32(part), len(part))
    assert crc == zlib.crc32(img.astype("<u2").tobytes())
