"""mic_hip_wavelet_v2_batch_plan (no device) against the cut rule restated in tests/wavelet_mixed_frames.py, on lists chosen to hit its
seams; and the oracle's word on the frame lists tests/test_gpu_wavelet_mixed.py sends through one batch call."""
import numpy as np
import pytest

import wavelet_mixed_frames as F

HUGE, SMALL = (2140, 1760), (64, 64)
PER_HUGE = F.per_frame(HUGE[0] * HUGE[1])


def _check(mic, rc, budget):
    want = F.plan(rc, budget)
    got = mic.wavelet_v2_batch_plan(rc, budget)
    assert got.dtype == np.uint32 and got.tolist() == want, (budget, got.tolist()[:8], want[:8])
    return want


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_huge_frame_among_many_small_ones(mic, where):
    rc = [SMALL] * 40
    rc.insert({"first": 0, "middle": 20, "last": 40}[where], HUGE)
    budget = 3 * PER_HUGE + 5                                  # three frames of the huge one's size; 40 small ones fit on their own
    assert budget // F.per_frame(64 * 64) >= 41
    cuts = _check(mic, rc, budget)
    # the huge frame sets the capacity of its sub-batch from the moment it joins: in front it takes two small ones along, behind
    # more than three small ones it starts a sub-batch of its own
    assert cuts == {"first": [0, 3, 41], "middle": [0, 20, 23, 41], "last": [0, 40, 41]}[where]


@pytest.mark.parametrize("k", [1, 2, 5])
def test_a_budget_that_holds_exactly_k_frames_of_the_largest(mic, k):
    rc = [HUGE] * (2 * k + 3)
    assert _check(mic, rc, k * PER_HUGE)[1] == k
    assert _check(mic, rc, (k + 1) * PER_HUGE)[1] == k + 1
    assert _check(mic, rc, (k + 1) * PER_HUGE - 1)[1] == k


def test_a_single_frame_over_the_budget_joins_alone(mic):
    rc = [SMALL, HUGE, SMALL, HUGE, HUGE]
    assert _check(mic, rc, PER_HUGE // 2) == [0, 1, 2, 3, 4, 5]
    assert _check(mic, [HUGE], 1) == [0, 1]


def test_65536_tiny_frames_and_the_pixel_target(mic):
    assert _check(mic, [(1, 1)] * 65536, 1 << 50) == [0, 65535, 65536]
    assert _check(mic, [(1 << 13, 1 << 14)] * 9, 1 << 60) == [0, 8, 9]      # 8 x 2^27 pixels reach the target of 2^30
    assert _check(mic, [], 1 << 30) == [0]


def test_capacity_and_argument_errors(mic):
    rc = [HUGE] * 7
    with pytest.raises(mic.MicError) as e:
        mic.wavelet_v2_batch_plan(rc, PER_HUGE, cap=3)
    assert e.value.code == mic.MIC_ERR_CAPACITY and e.value.ncuts == 8
    assert mic.wavelet_v2_batch_plan(rc, PER_HUGE, cap=8).tolist() == list(range(8))
    for bad in ((0, 5), (5, 0), (-1, 5), (5, -3)):
        with pytest.raises(mic.MicError) as e:
            mic.wavelet_v2_batch_plan([SMALL, bad, SMALL], PER_HUGE)
        assert e.value.code == mic.MIC_ERR_ARGS, bad


def test_the_gpu_lists_compress_in_the_oracle_except_the_3_x_3_frame(mico):
    jobs = F.tiling_jobs() + F.scan_jobs() + F.wide_jobs() + F.level_images() + [(F.escape_frame(), 65535, 2)]
    for img, mv, lv in jobs:
        rc, f = mico.wavelet_v2_compress(img, mv, lv)
        assert (rc != 0) == (img.shape == (3, 3)), (img.shape, rc)
        if rc == 0:
            rc2, back = mico.wavelet_v2_decompress(f)
            assert rc2 == 0 and np.array_equal(back, img), img.shape
