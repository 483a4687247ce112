"""The frame cache of the MIC2 crop readers without a device: the host model (mic2_frame_cache_model.py) pinned by hand-worked
traces, the cache object's constructor and slot size, and mic_hip_tile_cache_plan -- the policy's own code -- against the model's
outcomes on the same traces."""
import numpy as np
import pytest

import mic2_frame_cache_model as FM
from mic2_frame_cache_model import HIT, MISS, BYPASS

T20 = [(20, True)]


def _r0(d):
    """the entries of reader 0 of a model result, by frame"""
    return {f: v for (r, f), v in d.items() if r == 0}


def test_anchor_that_no_crop_named():
    res, cnt = FM.predict(4, T20, [[(0, [3, 9])], [(0, [11, 12])]])
    assert _r0(res[0]["outcomes"]) == {3: MISS, 9: MISS}
    assert _r0(res[0]["anchors"]) == {3: None, 9: 3}                     # (3 is an earlier miss of the same call)
    assert res[0]["decoded"] == {(0, g) for g in range(10)}
    assert _r0(res[1]["anchors"]) == {11: 9, 12: 11}                     # frame 9: resident, named by nobody in this call
    assert res[1]["decoded"] == {(0, 10), (0, 11), (0, 12)}
    assert res[1]["resident"] == {FM.key(0, f) for f in (3, 9, 11, 12)}
    assert cnt == dict(hits=0, misses=4, bypassed=0, evictions=0, calls=2)


def test_anchor_evicted_by_the_same_calls_misses():
    res, cnt = FM.predict(2, T20, [[(0, [3, 9])], [(0, [11, 12])]])
    assert _r0(res[1]["outcomes"]) == {11: MISS, 12: MISS}
    assert _r0(res[1]["anchors"]) == {11: None, 12: 11}                  # frame 9 went to make room: not an anchor
    assert res[1]["decoded"] == {(0, g) for g in range(13)}
    assert res[1]["resident"] == {FM.key(0, 11), FM.key(0, 12)}
    assert cnt == dict(hits=0, misses=4, bypassed=0, evictions=2, calls=2)


def test_no_slot_one_slot_and_exactly_the_calls_size():
    res, cnt = FM.predict(0, T20, [[(0, [3, 9])], [(0, [3, 9])]])
    for r in res:
        assert _r0(r["outcomes"]) == {3: BYPASS, 9: BYPASS} and _r0(r["anchors"]) == {3: None, 9: None}
        assert r["decoded"] == {(0, g) for g in range(10)} and r["resident"] == set()
    assert cnt == dict(hits=0, misses=0, bypassed=4, evictions=0, calls=2)
    res, cnt = FM.predict(1, T20, [[(0, [3, 9])], [(0, [9])], [(0, [9, 10])]])
    assert _r0(res[0]["outcomes"]) == {3: MISS, 9: BYPASS} and _r0(res[0]["anchors"]) == {3: None, 9: 3}
    assert res[0]["decoded"] == {(0, g) for g in range(10)} and res[0]["resident"] == {FM.key(0, 3)}
    assert _r0(res[1]["outcomes"]) == {9: MISS} and _r0(res[1]["anchors"]) == {9: None}   # its own miss evicted frame 3
    assert res[1]["decoded"] == {(0, g) for g in range(10)}
    assert _r0(res[2]["outcomes"]) == {9: HIT, 10: BYPASS} and _r0(res[2]["anchors"]) == {10: 9}
    assert res[2]["decoded"] == {(0, 10)}
    assert cnt == dict(hits=1, misses=2, bypassed=2, evictions=1, calls=3)
    res, cnt = FM.predict(2, T20, [[(0, [3, 9])], [(0, [3, 9])]])
    assert _r0(res[1]["outcomes"]) == {3: HIT, 9: HIT} and res[1]["decoded"] == set() and res[1]["anchors"] == {}
    assert cnt == dict(hits=2, misses=2, bypassed=0, evictions=0, calls=2)


def test_failed_residual_in_the_middle_of_a_run():
    res, cnt = FM.predict(4, T20, [[(0, [3, 6, 9])], [(0, [6])]], bad={0: [(0, 5)]})
    assert res[0]["decoded"] == {(0, g) for g in range(10)}
    assert _r0(res[0]["failed"]) == {6: 5, 9: 5}
    assert res[0]["resident"] == {FM.key(0, 3)}
    assert _r0(res[1]["anchors"]) == {6: 3} and res[1]["decoded"] == {(0, 4), (0, 5), (0, 6)}
    assert cnt == dict(hits=0, misses=2, bypassed=2, evictions=0, calls=2)
    # two runs in one call: the second one has an anchor of its own and stands
    m = FM.FrameCacheModel(4, T20)
    m.call([(0, [12])])
    r = m.call([(0, [3, 14])], bad=[(0, 2)])
    assert r["decoded"] == {(0, g) for g in (0, 1, 2, 3, 13, 14)} and _r0(r["failed"]) == {3: 2}
    assert r["resident"] == {FM.key(0, 12), FM.key(0, 14)}
    # an independent file loses the frame alone
    res, cnt = FM.predict(4, [(20, False)], [[(0, [3, 6, 9])]], bad={0: [(0, 6)]})
    assert res[0]["decoded"] == {(0, 3), (0, 6), (0, 9)} and _r0(res[0]["failed"]) == {6: 6} and res[0]["anchors"] == {}
    assert res[0]["resident"] == {FM.key(0, 3), FM.key(0, 9)}
    assert cnt == dict(hits=0, misses=2, bypassed=1, evictions=0, calls=1)


def test_two_readers_share_the_slots():
    files = [(20, False), (20, True)]
    res, cnt = FM.predict(3, files, [[(0, [1, 2]), (1, [5])], [(1, [7]), ], [(0, [2]), (1, [4, 8])]])
    assert res[0]["outcomes"] == {(0, 1): MISS, (0, 2): MISS, (1, 5): MISS} and res[0]["anchors"] == {(1, 5): None}
    assert res[1]["outcomes"] == {(1, 7): MISS} and res[1]["anchors"] == {(1, 7): 5}       # evicts reader 0's frame 1 (slot 0)
    assert res[1]["resident"] == {FM.key(1, 7), FM.key(0, 2), FM.key(1, 5)}
    # call 3: frame 2 hits; two misses evict the oldest entries that are left -- reader 1's frame 5, then its frame 7
    assert res[2]["outcomes"] == {(0, 2): HIT, (1, 4): MISS, (1, 8): MISS}
    assert res[2]["anchors"] == {(1, 4): None, (1, 8): 4}
    assert res[2]["decoded"] == {(1, g) for g in range(9)}
    assert cnt == dict(hits=1, misses=6, bypassed=0, evictions=3, calls=3)


TRACES = [(4, [[(0, [3, 9])], [(0, [11, 12])]]), (2, [[(0, [3, 9])], [(0, [11, 12])]]), (0, [[(0, [3, 9])], [(0, [3, 9])]]),
          (1, [[(0, [3, 9])], [(0, [9])], [(0, [9, 10])]]), (2, [[(0, [3, 9])], [(0, [3, 9])]]),
          (3, [[(0, [1, 2]), (1, [5])], [(1, [7])], [(0, [2]), (1, [4, 8])]])]


@pytest.mark.parametrize("nslots,calls", TRACES)
def test_the_librarys_policy_agrees_with_the_model(mic, nslots, calls):
    files = [(20, True), (20, True)]
    res, cnt = FM.predict(nslots, files, calls)
    outs, evictions = mic.tile_cache_plan(nslots, [FM.keys_of(c) for c in calls])
    for k, c in enumerate(calls):
        want = [res[k]["outcomes"][(key >> 32, key & 0xFFFFFFFF)] for key in FM.keys_of(c)]
        assert outs[k].tolist() == want, (nslots, k)
    assert evictions == cnt["evictions"]


def test_frame_cache_slot_bytes_and_create_need_no_device(mic):
    assert mic.frame_cache_slot_bytes(37, 19) == 1536                    # 1406 bytes of samples, padded to 256
    assert mic.frame_cache_slot_bytes(64, 33) == 4352
    assert mic.frame_cache_slot_bytes(8, 1) == 256 and mic.frame_cache_slot_bytes(128, 1) == 256 and mic.frame_cache_slot_bytes(129, 1) == 512
    assert mic.frame_cache_slot_bytes(1 << 14, 1 << 14) == 1 << 29       # 2^28 pixels: the crop doors' limit
    for w, h in ((0, 5), (5, 0), (-1, 5), (5, -3)):
        with pytest.raises(mic.MicError) as e:
            mic.frame_cache_slot_bytes(w, h)
        assert e.value.code == mic.MIC_ERR_ARGS
        with pytest.raises(mic.MicError) as e:
            mic.FrameCache(w, h, 4)
        assert e.value.code == mic.MIC_ERR_ARGS
    for call in (lambda: mic.frame_cache_slot_bytes((1 << 14) + 1, 1 << 14), lambda: mic.FrameCache((1 << 14) + 1, 1 << 14, 1),
                 lambda: mic.FrameCache(64, 33, 0xFFFFFFFF)):
        with pytest.raises(mic.MicError) as e:
            call()
        assert e.value.code == mic.MIC_ERR_UNSUPPORTED
    for slots in (0, 1, 7):
        with mic.FrameCache(64, 33, slots) as c:
            st = c.stats()
            assert st == dict(slots=slots, resident=0, hits=0, misses=0, bypassed=0, evictions=0, calls=0, device_bytes=0)
            c.clear()
    c = mic.FrameCache(1 << 14, 1 << 14, 1 << 20)                        # 2^49 bytes: still no allocation
    assert c.stats()["device_bytes"] == 0
    c.close()
    c.close()


def test_a_reader_takes_only_a_cache_of_its_frame_size(mic):
    import mic2_multi_volumes as M
    data = M.hand_file(64, 33, 5, True)
    rd = mic.Mic2Reader(data)
    assert not rd.cache_probe([0, 1, 4]).any()                           # no cache: nothing is resident
    for w, h in ((64, 32), (63, 33), (33, 64)):
        with mic.FrameCache(w, h, 2) as c:
            with pytest.raises(mic.MicError) as e:
                rd.set_cache(c)
            assert e.value.code == mic.MIC_ERR_ARGS
    with mic.TileCache(64, 33, 1, 8, 2) as c:                            # a tile cache of 8-bit samples
        with pytest.raises(mic.MicError) as e:
            rd.set_cache(c)
        assert e.value.code == mic.MIC_ERR_ARGS
    c = mic.FrameCache(64, 33, 2)
    rd.set_cache(c)
    rd.set_cache(c)                                                      # the cache it has: nothing happens
    assert not rd.cache_probe(np.arange(5)).any()
    with pytest.raises(mic.MicError) as e:
        c.close()                                                        # attached
    assert e.value.code == mic.MIC_ERR_ARGS
    rd.set_cache(None)
    rd.set_cache(c)
    rd.close()                                                           # close detaches
    c.close()
