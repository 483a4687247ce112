"""The CPU model of the eight-part split decode (tests/tans_split8_model.py) against the oracle's own streams: the states read out of
part 0's tok and the seven scratch regions -- which hold a part's steps from W on only -- are the plain decode's; a region of
exactly a part's live steps is enough and one a chunk shorter is not, at a middle boundary and at the stream's end; and a seventh of
a tier-1 slab holds every part of a full 256-row strip at the default overlap.  No GPU."""
import functools

import numpy as np

import tans_split_model as M
import tans_split8_model as M8

W = 8192


def _strip(synth, seed, rows, noise=None):
    img = synth.xr_like(cols=2577, rows=256, depth=12, seed=seed, noise=synth.XR_NOISE_PUBLISHED_RATIO if noise is None else noise)
    return np.ascontiguousarray(img[64:64 + rows])


@functools.lru_cache(maxsize=None)
def _stream(mico, synth, seed=5, rows=48):
    return M.Stream(mico, mico.delta_rle_compress(_strip(synth, seed, rows), 4095))


def _live(s, I, w):
    """the steps behind W that parts 1 .. 7 must hold in their regions: e_p - W, and j_end - W for the last"""
    bounds = [*I, s.count]
    return [b - a for a, b in zip(bounds, bounds[1:])]


def test_joined_parts_equal_the_plain_decode(mico, synth):
    s = _stream(mico, synth)
    assert s.table_log == 13 and not s.zero_bits and s.count >= 8 * W
    states, I = M8.joined(s, W)
    assert len(I) == 7 and 0 < I[0] and all(a < b for a, b in zip(I, I[1:])) and I[6] < s.count
    want, left = s.decode()
    assert left >= 0 and len(states) == s.count
    assert np.array_equal(s.tab_sym[np.asarray(states, np.int64)], want) and np.array_equal(want, s.tok)
    # every part keeps about an eighth of what lies behind the overlaps: (T + 7 W) / 8 steps, W of them dead for parts 1 .. 7
    eighth = (s.count + 7 * W) // 8
    assert abs(I[0] - eighth) < s.count // 20 and all(abs(k + W - eighth) < s.count // 20 for k in _live(s, I, W))


def test_a_region_of_a_parts_live_steps_is_enough_and_a_chunk_less_is_not(mico, synth):
    """R is one value for all seven regions, so the part that decides is the first one that needs the last chunk of an R rounded up
    from the most live steps of any part: that R joins the unit, one chunk less hands it back at that part's lower end -- boundary p + 1 for a middle part p, 8 (the
    stream's end) for part 7.  The last part is the long one where the noise falls towards the strip's bottom (many tokens for the
    stream's last eighth of the bits)"""
    seen = set()
    hi, lo = _strip(synth, 5, 64, 400.0), _strip(synth, 5, 64, 8.0)
    falling = np.ascontiguousarray(np.vstack([hi[:51], lo[51:]]))
    for s in (_stream(mico, synth, 5, 48), M.Stream(mico, mico.delta_rle_compress(falling, 4095))):
        P = M.Parts(s, W, n=8)
        outcome, I, fail = M8.split8(s, W, parts=P)
        assert (outcome, fail) == (M.DONE, 0), (s.count, outcome, fail)
        live = _live(s, I, W)
        r_ok = (max(live) + 15) & ~15
        p = 1 + min(q for q, x in enumerate(live) if x > r_ok - 16)          # the first part whose live steps need R's last chunk
        assert M8.split8(s, W, R=r_ok, parts=P) == (M.DONE, I, 0)
        o, II, f = M8.split8(s, W, R=r_ok - 16, parts=P)
        assert (o, f) == (M.NO_ROOM, p + 1) and II[:p] == I[:p], (s.count, p, o, f)
        # the layout with the dead steps stored needs W more
        assert M.split_parts(s, W, R=r_ok, parts=P, n=8)[0] == M.NO_ROOM and M.split_parts(s, W, R=r_ok + W, parts=P, n=8)[0] == M.DONE
        seen.add("end" if p == 7 else "middle")
    assert seen == {"end", "middle"}, seen


def test_routing_at_the_eight_part_threshold(mico, synth):
    s = _stream(mico, synth)
    assert s.gate(min_tokens=4096)
    assert M8.route(s, min_tokens=4096, min_tokens4=4096, min_tokens8=s.count) == M8.EIGHT_PARTS
    assert M8.route(s, min_tokens=4096, min_tokens4=4096, min_tokens8=s.count + 1) == M.FOUR_PARTS
    assert M8.route(s, min_tokens=4096, min_tokens4=s.count + 1, min_tokens8=4096) == M.TWO_PARTS    # max(min_tokens8, min_tokens4) decides
    assert M8.route(s, min_tokens=s.count + 1, min_tokens4=4096, min_tokens8=4096) == M.UNSPLIT
    assert M8.route(s, min_tokens=4096, min_tokens4=4096, min_tokens8=4096, min_bits16=16 * 11) == M.UNSPLIT
    assert M8.route(s) == M.UNSPLIT and M8.MIN_TOKENS8 == 3 * M.MIN_TOKENS


def test_the_tier_one_region_holds_a_full_strip(mico, synth):
    """a headline strip from the frame's middle (2577 x 256, about 640 k tokens) at the default overlap: all seven joins, part 0 inside tok, every later part's
    live steps inside a seventh of the slab -- where the four-part layout's W dead steps in front would not fit"""
    img = np.ascontiguousarray(synth.xr_like(cols=2577, rows=2048, depth=12, seed=1, noise=synth.XR_NOISE_PUBLISHED_RATIO)[1024:1280])
    s = M.Stream(mico, mico.delta_rle_compress(img, 4095))
    R = M8.region(img.size)
    assert R == 746272 // 7 & ~15 == 106608 and M8.route(s) == M8.EIGHT_PARTS
    P = M.Parts(s, M.OVERLAP, n=8)
    o, I, f = M8.split8(s, M.OVERLAP, R=R, parts=P)
    assert (o, f) == (M.DONE, 0), (o, I, f)
    live = _live(s, I, M.OVERLAP)
    assert s.count > 600000 and I[0] <= 746272 and max(live) <= R < max(live) + M.OVERLAP, (s.count, I, live)
    assert M.split_parts(s, M.OVERLAP, R=R, parts=P, n=8)[0] == M.NO_ROOM   # the layout with the dead steps stored
