"""mic_hip_shard_plan (csrc/mic_host_io.hip): the contiguous, pixel-balanced cut of a batch's jobs over the devices of
mic_hip_set_devices -- the static assignment of the reference's fan-outs (parallelstrips.go:77-93).  Pure host logic: no GPU."""
import numpy as np


def _check(first, n, shards):
    assert len(first) == shards + 1 and first[0] == 0 and first[-1] == n
    assert all(a <= b for a, b in zip(first, first[1:]))


def test_equal_weights_cut_evenly(mic):
    for n, shards in ((8, 2), (64, 8), (10, 3), (7, 7), (5, 8), (0, 4), (1, 1)):
        first = mic.shard_plan([1000] * n, shards)
        _check(first, n, shards)
        sizes = [b - a for a, b in zip(first, first[1:])]
        assert max(sizes) - min(sizes) <= 1 or n < shards


def test_weighted_cut_is_balanced_to_within_one_item(mic):
    rng = np.random.default_rng(1)
    for _ in range(200):
        n = int(rng.integers(1, 400)); shards = int(rng.integers(1, 9))
        w = rng.integers(1, 6_000_000, n)
        first = mic.shard_plan(w, shards)
        _check(first, n, shards)
        total = int(w.sum())
        for k in range(shards):
            got = int(w[first[k]: first[k + 1]].sum())
            assert got <= total / shards + int(w.max()) + 1      # never more than its share plus one item
        # the prefix up to boundary k reaches k / shards of the total, and would not without its last item
        for k in range(1, shards):
            pre = int(w[: first[k]].sum())
            assert pre >= (total * k) // shards or first[k] == n
            if first[k] > 0 and first[k] > first[k - 1]:
                assert pre - int(w[first[k] - 1]) < (total * k) // shards + 1


def test_zero_weights_and_bad_arguments(mic):
    first = mic.shard_plan([0, 0, 0, 0], 2)
    _check(first, 4, 2)
    assert first[1] == 2                                         # (an item of no weight counts as one pixel)
    import pytest
    with pytest.raises(mic.MicError):
        mic.shard_plan([1, 2], 0)


def test_groups_cut_by_frame_count_do_not_survive_a_second_plan(mic):
    """mic_hip_mic2_compress / _decompress cut n frames into the groups [n k / shards, n (k + 1) / shards): 26 frames on three
    devices are 8, 9 and 9.  Planned again by weight, the goals are 26 npx k / 3 = 8.67 npx and 17.33 npx: the first group's 8 npx
    is below the first, so shard 0 takes the second group too; 17 npx is below the second, so shard 1 takes the third -- two shards
    of 17 and 9 frames and an idle third device, where the groups were made for three.  17 frames on two devices (8 and 9, goal
    8.5 npx) end on one.  So MIC2 hands its own cut to the fan-out (micapi::over_devices, the explicit form) and does not go
    through this plan; tests/test_gpu_multi_device.py checks the shards that run."""
    npx = 160 * 120
    assert mic.shard_plan([8 * npx, 9 * npx, 9 * npx], 3) == [0, 2, 3, 3]
    assert mic.shard_plan([8 * npx, 9 * npx], 2) == [0, 2, 2]
    assert mic.shard_plan([npx] * 26, 3) == [0, 9, 18, 26]                   # (frames planned one by one: no such collapse)
