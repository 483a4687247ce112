"""The MIC3 tile cache without a device (include/mic_hip.h: mic_hip_tile_cache_*): the replacement policy over traces
(mic_hip_tile_cache_plan, the code the device path runs) against an LRU model written from the policy's text
(tests/tile_cache_model.py), the slot size, and
the lifecycle of cache, reader and session attachments.  Nothing here launches anything: the cache allocates its arena at the first
patch call that uses it."""
import struct

import numpy as np
import pytest

from tile_cache_model import lru_model


# ---- the policy against the model written from its text (tile_cache_model.py) -----------------------------------------------------
def _check(mic, nslots, calls):
    got, ev = mic.tile_cache_plan(nslots, calls)
    want, wev, _ = lru_model(nslots, calls)
    assert [g.tolist() for g in got] == want, (nslots, calls)
    assert ev == wev
    return want


def _random_trace(seed, ncalls=12, universe=24, longest=9):
    rng = np.random.default_rng(seed)
    return [sorted(rng.choice(universe, size=int(rng.integers(1, longest + 1)), replace=False).tolist()) for _ in range(ncalls)]


@pytest.mark.parametrize("seed", range(6))
def test_plan_follows_the_lru_model_on_random_traces(mic, seed):
    calls = _random_trace(seed)
    union = len(set().union(*calls))
    for nslots in (0, 1, 2, union - 1, union, union + 1):
        _check(mic, nslots, calls)


def test_a_call_longer_than_the_cache_bypasses_its_tail(mic):
    out = _check(mic, 3, [[1, 2, 3, 4, 5], [1, 2, 3, 4, 5], [4, 5]])
    assert out[0] == [1, 1, 1, 2, 2] and out[1] == [0, 0, 0, 2, 2]
    assert out[2] == [1, 1]                            # (evicts two entries of the call before: stamps below this call's)
    assert _check(mic, 0, [[7, 8], [7]]) == [[2, 2], [2]]


def test_a_hit_is_stamped_before_any_miss_picks_a_victim(mic):
    # two slots hold 1 (older) and 2; the call [1, 3] hits 1 first, so 3 must evict 2, although 1 had the smaller stamp
    out = _check(mic, 2, [[1], [2], [1, 3], [1, 2, 3]])
    assert out[2] == [0, 1] and out[3] == [0, 2, 0]    # 1 and 3 stayed; 2 finds both slots stamped by its own call: bypassed
    out = _check(mic, 2, [[1], [2], [1, 3], [2]])
    assert out[3] == [1]


def test_equal_stamps_fall_to_the_lowest_slot(mic):
    # call 1 fills slots 0..3 with one stamp; the misses of call 2 take slots 0 and 1, so 10 and 11 go and 12, 13 stay
    out = _check(mic, 4, [[10, 11, 12, 13], [20, 21], [12, 13], [10, 11]])
    assert out[2] == [0, 0] and out[3] == [1, 1]
    # freed slots are taken lowest first as well: with slots {0: 20, 1: 21, 2: 12, 3: 13} all but 12 / 13 equally old
    _check(mic, 4, [[10, 11, 12, 13], [20, 21], [12, 13], [30], [20], [21]])


def test_plan_refuses_a_trace_that_is_no_plan(mic):
    with pytest.raises(mic.MicError) as e:
        mic.tile_cache_plan(4, [[3, 2]])
    assert e.value.code == mic.MIC_ERR_ARGS
    with pytest.raises(mic.MicError):
        mic.tile_cache_plan(4, [[2, 2]])
    assert mic.tile_cache_plan(4, []) == ([], 0)


# ---- the slot ------------------------------------------------------------------------------------------------------------------------
def test_slot_bytes_of_the_three_formats_and_refusals(mic):
    assert mic.tile_cache_slot_bytes(256, 256, 3, 8) == 256 * 256 * 3
    assert mic.tile_cache_slot_bytes(64, 64, 1, 8) == 4096
    assert mic.tile_cache_slot_bytes(64, 64, 1, 16) == 8192
    assert mic.tile_cache_slot_bytes(0, 0, 3, 8) == 256 * 256 * 3                  # 0 = 256, as the encoder's defaults
    assert mic.tile_cache_slot_bytes(5, 7, 3, 8) == 256                           # 105 bytes, padded to 256
    assert mic.tile_cache_slot_bytes(9, 9, 1, 16) == 256 and mic.tile_cache_slot_bytes(13, 10, 1, 16) == 512
    for bad, code in (((64, 64, 3, 16), mic.MIC_ERR_UNSUPPORTED), ((64, 64, 2, 8), mic.MIC_ERR_UNSUPPORTED),
                      ((64, 64, 1, 12), mic.MIC_ERR_UNSUPPORTED), ((-1, 64, 3, 8), mic.MIC_ERR_ARGS),
                      ((1 << 14, 1 << 13, 3, 8), mic.MIC_ERR_UNSUPPORTED)):
        with pytest.raises(mic.MicError) as e:
            mic.tile_cache_slot_bytes(*bad)
        assert e.value.code == code, bad
        with pytest.raises(mic.MicError) as e:
            mic.TileCache(*bad, slots=4)
        assert e.value.code == code, bad
    assert mic.lib().mic_hip_tile_cache_slot_bytes(64, 64, 3, 8, None) == mic.MIC_ERR_ARGS


# ---- lifecycle ---------------------------------------------------------------------------------------------------------------------
def _mic3(tile, channels, bps):
    """a one-tile MIC3 file (wsiformat.go:99-165) of constant-zero planes: enough for a reader to open"""
    blob = (struct.pack("<III", 1, 1, 1) + bytes(3)) if channels == 3 else bytes(1)
    head = b"MIC3" + struct.pack("<IIIII", 1, tile, tile, tile, tile) + struct.pack("<HBBH", channels, bps, 0x01 | (0x02 if channels == 3 else 0), 1)
    head += bytes(2) + struct.pack("<Q", 1) + bytes(8)
    assert len(head) == 48
    return head + struct.pack("<IIIII", tile, tile, 1, 1, 0) + struct.pack("<QQ", 0, len(blob)) + blob


def test_fresh_cache_stats_are_zero(mic):
    with mic.TileCache(64, 64, 3, 8, slots=5) as c:
        assert c.stats() == dict(slots=5, resident=0, hits=0, misses=0, bypassed=0, evictions=0, calls=0, device_bytes=0)
        c.clear()
        assert c.stats()["resident"] == 0
    with mic.TileCache(64, 64, 1, 16, slots=0) as c:                               # a valid cache that keeps nothing
        assert c.stats()["slots"] == 0


def test_null_rules(mic):
    L = mic.lib()
    assert L.mic_hip_tile_cache_destroy(None) == mic.MIC_OK and L.mic_hip_tile_cache_clear(None) == mic.MIC_OK
    assert L.mic_hip_tile_cache_get_stats(None, None) == mic.MIC_ERR_ARGS
    assert L.mic_hip_tile_cache_create(64, 64, 3, 8, 1, None) == mic.MIC_ERR_ARGS
    assert L.mic_hip_wsi_reader_set_cache(None, None) == mic.MIC_ERR_ARGS
    assert L.mic_hip_wsi_reader_cache_probe(None, None, 0, None) == mic.MIC_ERR_ARGS
    assert L.mic_hip_session_set_tile_cache(None, None) == mic.MIC_ERR_ARGS
    assert L.mic_hip_session_tile_cache_probe(None, None, 0, None) == mic.MIC_ERR_ARGS
    assert L.mic_hip_tile_cache_plan(1, None, None, 1, None, None) == mic.MIC_ERR_ARGS
    with mic.TileCache(64, 64) as c:
        assert L.mic_hip_tile_cache_get_stats(c._h, None) == mic.MIC_ERR_ARGS


def test_attach_checks_the_format_and_destroy_waits_for_detach(mic):
    c = mic.TileCache(64, 64, 3, 8, slots=4)
    for tile, ch, bps in ((32, 3, 8), (64, 1, 8), (64, 1, 16)):
        with mic.WsiReader(_mic3(tile, ch, bps)) as rd:
            with pytest.raises(mic.MicError) as e:
                rd.set_cache(c)
            assert e.value.code == mic.MIC_ERR_ARGS
    a, b = mic.WsiReader(_mic3(64, 3, 8)), mic.WsiReader(_mic3(64, 3, 8))
    a.set_cache(c)
    a.set_cache(c)                                                                  # the cache it already has: nothing happens
    b.set_cache(c)
    assert not a.cache_probe([0, 1]).any()
    assert mic.lib().mic_hip_tile_cache_destroy(c._h) == mic.MIC_ERR_ARGS           # two owners attached: nothing is freed
    assert c.stats()["slots"] == 4
    a.set_cache(None)                                                               # detach ...
    assert mic.lib().mic_hip_tile_cache_destroy(c._h) == mic.MIC_ERR_ARGS
    b.close()                                                                       # ... and a reader's close detaches too
    c.close()
    assert not a.cache_probe([0]).any()                                             # (a reader without a cache: nothing is resident)
    a.close()
