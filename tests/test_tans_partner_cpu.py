"""The deadline of the partner protocol of the eight-part split decode (tests/tans_partner_model.py), on the oracle's own streams:
with the partner serving chunk c no later than the start of chunk c + 2, every dword a chunk reads is in the ring, no fill replaces
a block that a chunk still to come reads, and neither stage half nor mailbox half c & 1 is written again before chunk c is served
-- at each of the four byte offsets a bitstream can have against the dword grid.  One chunk later than that, it fails.  No GPU.

The streams: the eight-part tests' 9.57-bit strip, the fastest consumer found (noise 800: 11.66 bits per token, 5.8 of the 6.5 dwords
a chunk can take), and a strip whose noise falls towards its bottom, so the rate changes along the stream."""
import functools

import numpy as np
import pytest

import tans_partner_model as PM
import tans_split_model as M
import tans_split8_model as M8

W = 8192
MIN_TEST, MIN4_TEST, MIN8_TEST = 4096, 49152, 65536                # the eight-part GPU tests' thresholds


def _strip(synth, seed, rows, noise=None):
    img = synth.xr_like(cols=2577, rows=256, depth=12, seed=seed, noise=synth.XR_NOISE_PUBLISHED_RATIO if noise is None else noise)
    return np.ascontiguousarray(img[64:64 + rows])


def _falling(synth, seed, rows, top_rows, top=400.0, low=4.0):
    return np.ascontiguousarray(np.vstack([_strip(synth, seed, rows, top)[:top_rows], _strip(synth, seed, rows, low)[top_rows:]]))


@functools.lru_cache(maxsize=None)
def _stream(mico, synth, name):
    img = {"published": lambda: _strip(synth, 5, 48), "fast": lambda: _strip(synth, 5, 48, 800.0), "falling": lambda: _falling(synth, 5, 64, 51)}[name]()
    s = M.Stream(mico, mico.delta_rle_compress(img, 4095))
    return s, M.Parts(s, W, n=8)


@pytest.mark.parametrize("name", ["published", "fast", "falling"])
def test_the_partner_meets_its_deadline(mico, synth, name):
    s, P = _stream(mico, synth, name)
    assert s.table_log == 13 and not s.zero_bits
    assert M8.route(s, min_tokens=MIN_TEST, min_tokens4=MIN4_TEST, min_tokens8=MIN8_TEST) == M8.EIGHT_PARTS
    assert M8.split8(s, W, parts=P)[0] == M.DONE
    rate = s.bits / s.count
    if name == "published":
        assert s.count == 120136 and abs(rate - 9.57) < 0.01, (s.count, rate)
    if name == "fast":
        assert s.count == 121235 and rate >= 11.5, (s.count, rate)
    if name == "falling":                                                   # the first part's rate against the last one's
        bounds = [0, *M8.split8(s, W, parts=P)[1], s.count]
        live = [b - a for a, b in zip(bounds, bounds[1:])]
        assert max(live) > 1.5 * min(live), live                            # (the parts cover equal bits: tokens per part differ with the rate)
    for sb in range(4):
        n, fills, most = PM.check(s, W, sb=sb, parts=P)
        assert n == PM.chunks_run(s, W, P) and n >= (s.count + 7 * W) // 8 // PM.CHUNK
        assert most <= 6.5 and all(f > 0 for f in fills), (most, fills)
        if name == "fast" and sb == 0:
            assert most > 5.5, most                                         # close to the ceiling: the case the ring has no dword to spare for


def test_a_partner_one_chunk_later_is_too_late(mico, synth):
    """the same model with the fill (and the stage) served one chunk behind the rule: a chunk reads a block that is not there yet,
    or writes a stage half that still holds the chunk two back"""
    s, P = _stream(mico, synth, "fast")
    with pytest.raises(AssertionError, match="late schedule, lag 1"):
        PM.check(s, W, sb=0, lag=1, parts=P)
    # and the ring alone, every chunk with a stage and a mailbox of its own: a chunk reads a block that is not there yet
    for name in ("fast", "published"):
        s, P = _stream(mico, synth, name)
        with pytest.raises(AssertionError, match="late schedule, lag 1: chunk [0-9]+ reads block"):
            PM.check(s, W, sb=0, lag=1, parts=P, ring_only=True)
        PM.check(s, W, sb=0, lag=0, parts=P, ring_only=True)
