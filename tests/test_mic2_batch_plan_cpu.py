"""CPU tests of mic_hip_mic2_batch_plan, the cut rule of the MIC2 whole-volume batches as a host function, against the rule restated
in mic2_multi_volumes.cuts_of."""
import numpy as np
import pytest

import mic2_multi_volumes as M

MB = 1 << 20
# (w, h, n): 150 x 70 and 160 x 96 hold three and two units in 7 MiB, the small ones three (test_gpu_mic2_multi_crops.py)
MIXED = [(150, 70, 10), (7, 35, 1), (33, 9, 3), (160, 96, 6), (150, 70, 11), (150, 70, 1), (150, 70, 2), (160, 96, 6)]


def _px(whn):
    return [w * h for w, h, n in whn for _ in range(n)]


@pytest.mark.parametrize("budget", [1, 3 * MB, 7 * MB, 12 * MB, 64 * MB, 1 << 40])
@pytest.mark.parametrize("whn", [MIXED, MIXED[::-1], [(512, 512, 5)], [(1, 1, 1)] * 9, [(33, 9, 3), (1024, 1024, 2), (7, 35, 4)]])
def test_cuts_equal_the_restated_rule(mic, whn, budget):
    cuts, nunits = mic.mic2_batch_plan(whn, budget)
    px = _px(whn)
    assert nunits == len(px)
    assert cuts.tolist() == M.cuts_of(px, budget)
    assert cuts[0] == 0 and cuts[-1] == len(px) and (np.diff(cuts.astype(np.int64)) >= 1).all()


def test_a_unit_larger_than_the_budget_still_gets_a_sub_batch(mic):
    whn = [(33, 9, 2), (2048, 2048, 3), (33, 9, 2)]
    assert M.unit_ws_bytes(2048 * 2048) > 7 * MB
    cuts, nunits = mic.mic2_batch_plan(whn, 7 * MB)
    assert nunits == 7 and cuts.tolist() == M.cuts_of(_px(whn), 7 * MB)
    assert [2, 3] in [[a, b] for a, b in zip(cuts.tolist(), cuts.tolist()[1:])]          # each large frame alone
    assert all(b - a == 1 for a, b in zip(cuts.tolist(), cuts.tolist()[1:]) if 2 <= a < 5)


def test_where_the_cuts_of_the_mixed_list_fall(mic):
    """at 7 MiB: inside a volume, right behind a frame 0, and between volumes"""
    cuts, _ = mic.mic2_batch_plan(MIXED, 7 * MB)
    first = np.cumsum([0] + [n for _, _, n in MIXED]).tolist()                            # first unit of each volume
    inner = cuts.tolist()[1:-1]
    assert any(c in first for c in inner)                                                  # between volumes
    assert any(c - 1 in first and c not in first for c in inner)                           # right behind a frame 0
    assert any(c not in first and c - 1 not in first for c in inner)                       # inside a volume
    assert cuts.tolist()[:5] == [0, 3, 6, 9, 12] and 12 == first[2] + 1                    # [f9, the 7 x 35 frame, frame 0 of 33 x 9 x 3]


def test_cap_too_small_and_no_volumes(mic):
    with pytest.raises(mic.MicError) as e:
        mic.mic2_batch_plan(MIXED, 7 * MB, cap=3)
    want = M.cuts_of(_px(MIXED), 7 * MB)
    assert e.value.code == mic.MIC_ERR_CAPACITY and e.value.ncuts == len(want) and e.value.nunits == len(_px(MIXED))
    cuts, nunits = mic.mic2_batch_plan(MIXED, 7 * MB, cap=len(want))
    assert cuts.tolist() == want
    cuts, nunits = mic.mic2_batch_plan([], 7 * MB)
    assert cuts.tolist() == [0] and nunits == 0


def test_bad_dimensions_and_the_default_budget(mic):
    for bad in [(0, 5, 1), (5, -1, 1), (5, 5, 0)]:
        with pytest.raises(mic.MicError) as e:
            mic.mic2_batch_plan([(4, 4, 1), bad], 7 * MB)
        assert e.value.code == mic.MIC_ERR_ARGS
    cuts, nunits = mic.mic2_batch_plan(MIXED, 0)                                           # the default ceiling is at least 1 GiB: one chain
    assert cuts.tolist() == [0, nunits] and nunits == len(_px(MIXED))
