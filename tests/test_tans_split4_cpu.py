"""The CPU model of the four-part split decode (tests/tans_split_model.py) against the oracle's own streams: the states read out
of part 0's tok and the three scratch regions are the plain decode's, units are routed by length between the two split
instances, and no part's output can leave its region.  No GPU."""
import functools

import numpy as np

import tans_split_model as M

M4 = M                                             # (one model for both part counts; four parts are its default)

W = 8192


def _strip(synth, seed, rows):
    img = synth.xr_like(cols=2577, rows=256, depth=12, seed=seed, noise=synth.XR_NOISE_PUBLISHED_RATIO)
    return np.ascontiguousarray(img[64:64 + rows])


@functools.lru_cache(maxsize=None)
def _stream(mico, synth, seed=5, rows=48):
    return M.Stream(mico, mico.delta_rle_compress(_strip(synth, seed, rows), 4095))


def test_joined_parts_equal_the_plain_decode(mico, synth):
    s = _stream(mico, synth)
    assert s.table_log == 13 and not s.zero_bits and s.count >= 4 * W
    states, I = M4.joined(s, W)
    assert 0 < I[0] < I[1] < I[2] < s.count
    want, left = s.decode()
    assert left >= 0 and len(states) == s.count
    assert np.array_equal(s.tab_sym[np.asarray(states, np.int64)], want) and np.array_equal(want, s.tok)
    # every part decodes about a quarter of the stream plus three quarters of the overlap
    quarter = (s.count + 3 * W) // 4
    ends = [I[0], I[1] - I[0] + W, I[2] - I[1] + W, s.count - I[2] + W]
    assert all(abs(e - quarter) < s.count // 20 for e in ends), (ends, quarter)


def test_starts_fall_and_stay_inside_the_stream(mico, synth):
    s = _stream(mico, synth)
    for w in (64, 4096, W, 32768, s.count, 4 * s.count):
        p = M4.starts(s, w)
        assert p[0] == s.bits and all(a >= b for a, b in zip(p, p[1:])) and p[3] >= 0, (w, p)


def test_routing_at_the_four_part_threshold(mico, synth):
    s = _stream(mico, synth)
    assert s.gate(min_tokens=4096)
    assert M4.route(s, min_tokens=4096, min_tokens4=s.count) == M4.FOUR_PARTS        # count == min_tokens4
    assert M4.route(s, min_tokens=4096, min_tokens4=s.count + 1) == M4.TWO_PARTS     # count == min_tokens4 - 1
    assert M4.route(s, min_tokens=s.count + 1, min_tokens4=4096) == M4.UNSPLIT       # the four-part list lies behind the two-part gate
    assert M4.route(s) == M4.UNSPLIT and M4.MIN_TOKENS4 == 2 * M.MIN_TOKENS
    assert M4.route(s, min_tokens=4096, min_tokens4=4096, min_bits16=16 * 11) == M4.UNSPLIT   # ... and behind its rate gate


def test_no_part_can_overrun_its_region(mico, synth):
    s = _stream(mico, synth)
    P = M4.Parts(s, W)
    outcome, I, fail = M4.split4(s, W, parts=P)
    assert (outcome, fail) == (M.DONE, 0)
    ends = [I[1] - I[0] + W, I[2] - I[1] + W, s.count - I[2] + W]            # the last step of parts 1 .. 3
    for p, e in enumerate(ends):
        # a region that is one chunk short of a part's last step hands the unit back, at that part's lower boundary
        r_ok, r_short = (max(ends) + 31) & ~31, (e - 1) & ~31
        assert M4.split4(s, W, R=r_ok, parts=P)[0] == M.DONE
        o, _, f = M4.split4(s, W, R=r_short, parts=P)
        assert o == M.NO_ROOM and f <= p + 2, (p, e, o, f)
        first_short = min(q for q, x in enumerate(ends) if x > r_short)
        assert f == first_short + 2, (p, f, first_short)
    # the session's own regions hold the parts of such a strip with room to spare
    assert max(ends) <= M4.region(2577 * 48)


def test_an_overlap_too_small_to_meet_in_falls_back(mico, synth):
    s = _stream(mico, synth)
    o, I, f = M4.split4(s, 64)
    assert o == M.NOT_MET and 1 <= f <= 3 and all(v == 0 for v in I[f - 1:]), (o, I, f)
    assert M4.split4(s, s.count + 4096) == (M.NOT_MET, (0, 0, 0), 1)         # no hand-over inside the stream's chunks
