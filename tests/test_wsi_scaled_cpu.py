"""CPU tests of the scaled MIC3 patch readers: the judgement of a scale and the source extent (mic_hip_wsi_scaled_extent, which needs no
device), and the host reference itself (scaled_ref.py) against the pyramid rule and its own weights."""
import math

import numpy as np
import pytest

import scaled_ref as SR

# the scales of tests/test_gpu_wsi_scaled.py
SCALES = [(2, 1), (3, 2), (7, 3), (16, 1), (1024, 1023), (1024, 64), (13, 6)]
SIZES = [(24, 20), (71, 37), (4, 4), (2, 3), (256, 256), (1, 1)]


def test_scaled_extent_is_the_ceiling(mic):
    for num, den in SCALES + [(1, 1), (6, 6), (2048, 2048), (6, 4), (32, 2)]:
        for pw, ph in SIZES:
            want = (math.ceil(pw * num / den), math.ceil(ph * num / den))
            assert want == SR.extent(pw, ph, num, den)
            assert mic.wsi_scaled_extent(pw, ph, (num, den)) == want, (num, den, pw, ph)


@pytest.mark.parametrize("scale", [(0, 1), (1, 0), (0, 0), (-2, 1), (2, -1), (-2, -1), (1, 2), (1023, 1024), (17, 1), (33, 2), (1025, 1024),
                                   (2048, 2047), (2050, 2048), (1031, 65)])
def test_refused_scales(mic, scale):
    assert not SR.accepted(*scale)
    with pytest.raises(mic.MicError) as e:
        mic.wsi_scaled_extent(24, 20, scale)
    assert e.value.code == mic.MIC_ERR_ARGS


def test_accepted_scales_and_bad_sizes(mic):
    assert mic.wsi_scaled_extent(24, 20, (2048, 2048)) == (24, 20)               # 1 / 1 behind the reduction
    assert mic.wsi_scaled_extent(24, 20, (2048, 128)) == (384, 320)             # 16 / 1
    for scale in SCALES:
        assert SR.accepted(*scale)
    for pw, ph in [(0, 4), (4, 0), (-1, 4)]:
        with pytest.raises(mic.MicError) as e:
            mic.wsi_scaled_extent(pw, ph, (2, 1))
        assert e.value.code == mic.MIC_ERR_ARGS


def test_reference_is_the_pyramid_rule_at_2_1():
    rng = np.random.default_rng(3)
    for img in (rng.integers(0, 65536, (37, 52)).astype(np.uint16), rng.integers(0, 256, (20, 31, 3)).astype(np.uint8)):
        h, w = img.shape[0] // 2, img.shape[1] // 2
        got, outside = SR.resample(img, [(0, 0)], w, h, 2, 1)
        assert np.array_equal(got[0], SR.pyramid_2x(img)) and not outside.any()
        got, _ = SR.resample(img, [(4, 2)], 5, 3, 4, 2)                          # (reduced; an even origin inside)
        assert np.array_equal(got[0], SR.pyramid_2x(img)[1:4, 2:7])


def test_weights_sum_to_num():
    for num, den in SCALES:
        num, den = SR.reduce(num, den)
        for count in (1, 2, 3, 4, 20, 24, 37, 71):
            w = SR.weights(count, num, den)
            assert (w.sum(axis=1) == num).all() and w.max() <= den and w.min() >= 0, (num, den, count)
            assert (w.sum(axis=0)[: count * num // den] == den).all()             # every source pixel wholly under the patch is used up


def test_reference_pads_and_zero_extends():
    img = np.full((10, 10), 1000, dtype=np.uint16)
    got, outside = SR.resample(img, [(-3, 0), (10, 0), (7, 7)], 2, 2, 3, 1)
    assert outside[0].tolist() == [[True, False], [True, False]] and outside[1].all()
    assert got[0, 0, 1] == 1000 and got[2].tolist() == [[1000, 0], [0, 0]] and not outside[2, 0, 0] and outside[2, 1, 1]
    got, outside = SR.resample(img, [(9, 9)], 1, 1, 2, 1)                        # one of four pixels inside: no renormalisation
    assert got[0, 0, 0] == 250 and not outside.any()
