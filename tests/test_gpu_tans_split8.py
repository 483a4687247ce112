"""The eight-part instance of the two-state tANS chain (k_dec_tans_ls_parts<8>, csrc/mic_decode_ls.hip) at its seams, on small units.

The units are strips of the headline's frame (2577 columns, 32 .. 72 rows of 12-bit xr_like at the published noise: 80 - 180 k
tokens), coded by the oracle; the session's eight-part threshold is lowered to 65536 tokens, the two-part gate to 4096 and the
overlap set to 8192 through the debug setters, so that such units take the eight-part instance.  The eight-part list takes units of
at least max(min_tokens8, min_tokens4) tokens, so the four-part threshold comes down as well, to 49152.  One case needs a unit
that is shorter than its overlap of 65536 on the eight-part list and lowers min_tokens8 to 32768 for it.  What the kernel must
make of each unit -- joined, or handed back to the four-part instance and what that one makes of it -- is worked out on the CPU by tests/tans_split8_model.py; the library is asked for its record
(MicUnit.split and split_hi through mic_hip_debug_split8, the four-part view through mic_hip_debug_split4) and for the pixels, which
must be the source's bit for bit.

The shapes a case is there for are asserted on the CPU side, in front of the GPU run."""
import ctypes as C
import functools

import numpy as np
import pytest

import tans_split_model as M
import tans_split8_model as M8
import test_gpu_tans_split as S2
import test_gpu_tans_split4 as S4

pytestmark = pytest.mark.gpu

W_TEST = 8192
MIN8_TEST = 65536
MIN4_TEST = 49152                                  # (strips of fewer than about 32 k tokens are coded at tableLog 12: no class-0 units)
MIN_TEST = 4096
TILE = S2.TILE
Unit, _strip, _with_tokens = S2.Unit, S2._strip, S2._with_tokens

CANDIDATES = ((5, 48), (7, 56), (11, 48), (14, 50), (15, 54), (16, 62), (17, 72), (18, 48), (20, 60), (21, 44), (8, 36))
RESIDUES = ((30, 44, 0), (31, 46, 1), (32, 48, TILE - 1))   # (seed, rows, token count modulo 1536)
HANDED_BACK = ((13, 52), (9, 64), (6, 32))                 # the eight parts do not meet at boundary 7, 2 and 3


@functools.lru_cache(maxsize=None)
def _unit(mico, synth, seed, rows, residue=None, noise=None):
    img = _strip(synth, seed, rows, noise=noise)
    return Unit(mico, img if residue is None else _with_tokens(mico, img, residue))


def _lib(mic):
    L = S4._lib(mic)
    L.mic_hip_debug_split8.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mic_hip_debug_split8_config.argtypes = [C.c_void_p, C.c_uint32]
    return L


def _configure(mic, sess, min_tokens=MIN_TEST, overlap=W_TEST, min_tokens8=MIN8_TEST, min_tokens4=MIN4_TEST):
    S4._configure(mic, sess, min_tokens=min_tokens, overlap=overlap, min_tokens4=min_tokens4)
    assert _lib(mic).mic_hip_debug_split8_config(sess._h, min_tokens8) == 0


def _decode(mic, torch, sess, units, blobs=None, lead=0):
    """S4._decode, and the eight-part record per unit: (outcome, (I_1 .. I_7), W, R, failing boundary, parts)"""
    st, rec, split, rec4, imgs, align = S4._decode(mic, torch, sess, units, blobs=blobs, lead=lead)
    rec8 = []
    for i in range(len(units)):
        out = (C.c_uint32 * 12)()
        assert _lib(mic).mic_hip_debug_split8(sess._h, i, out) == 0
        rec8.append((int(out[0]), tuple(int(v) for v in out[1:8]), int(out[8]), int(out[9]), int(out[10]), int(out[11])))
    return st, rec, split, rec4, rec8, imgs, align


def _expect(u, overlap, min_tokens=MIN_TEST, min_tokens4=MIN4_TEST, min_tokens8=MIN8_TEST):
    """(the four-part view, the eight-part view) the unit's record must show: an eight-part unit that joins has zeros in the four-part
    view, one that is handed back carries the four-part instance's record and zeros in the eight-part view; parts is MicUnit.split[7]"""
    r = M8.route(u.model, min_tokens=min_tokens, min_tokens4=min_tokens4, min_tokens8=min_tokens8)
    Wr = overlap & ~63
    if r != M8.EIGHT_PARTS:
        w2, w4 = S4._expect(u, overlap, min_tokens=min_tokens, min_tokens4=min_tokens4)
        parts = {M.UNSPLIT: 0, M.TWO_PARTS: 2, M.FOUR_PARTS: 4}[r]
        return w4, (w4[0], (0,) * 7, None, 0, 0, parts)
    key = ("eight", overlap)
    if key not in u.expected:
        R8, R4 = M8.region(u.img.size), M.region(u.img.size)
        parts, o, I, fail = M8.outcome(u.model, overlap, R8, R4)
        if parts == 8:
            u.expected[key] = ((o, (0, 0, 0), Wr, 0, 0), (o, I, Wr, R8, fail, 8))
        else:
            u.expected[key] = ((o, I, Wr, R4, fail), (o, (0,) * 7, Wr, 0, 0, 4))
    return u.expected[key]


def _check(units, want, st, rec, rec4, rec8, imgs):
    for i, u in enumerate(units):
        w4, w8 = want[i]
        assert st[i] == 0, (i, st[i])
        got4 = rec4[i] if w4[2] is not None else rec4[i][:2] + (None,) + rec4[i][3:]   # (a two-part or unsplit unit: W is not part of the expectation)
        got8 = rec8[i] if w8[2] is not None else rec8[i][:2] + (None,) + rec8[i][3:]
        assert got4 == w4, (i, rec4[i], w4, u.ntok)
        assert got8 == w8, (i, rec8[i], w8, u.ntok)
        if u.model.table_log == 13 and not u.model.zero_bits:
            assert rec[i] == 1, (i, rec[i])                                 # class 0's record, whichever instance ran
        assert np.array_equal(imgs[i], u.img), (i, u.ntok, rec8[i])


def test_eight_part_units_join_where_the_model_says(mic, mico, synth, gpu_ready):
    torch = pytest.importorskip("torch")
    cand = [_unit(mico, synth, seed, rows, res) for seed, rows, res in RESIDUES] + [_unit(mico, synth, seed, rows) for seed, rows in CANDIDATES]
    want = [_expect(u, W_TEST) for u in cand]
    # the CPU side: the seams this batch is there for
    assert all(w[1][0] == M.DONE and w[1][5] == 8 for w in want), want
    assert all(w[1][3] == M8.region(u.img.size) > 0 for u, w in zip(cand, want))
    assert any(i % 8 for w in want for i in w[1][1])                          # a join inside a translate thread's eight tokens
    steps = [e for w in want for e in [w[1][1][0]] + [b - a + W_TEST for a, b in zip(w[1][1], w[1][1][1:])]]   # e_0 .. e_6
    assert {e & 1 for e in steps} == {0, 1}                                   # the lower part's lanes in step with it, and role-swapped
    assert [u.ntok % TILE for u in cand[:3]] == [0, 1, TILE - 1] and [u.ntok % 16 for u in cand[:3]] == [0, 1, 15]
    assert len({u.ntok // 16 for u in cand}) >= 10                            # lengths differ by whole chunks
    sess = mic.Session(len(cand), max(u.img.size for u in cand))
    try:
        _configure(mic, sess)
        seen, first = set(), None
        # 14 units: a full group (nine), a full wave and a last wave of two; 10 and 13: last waves of one
        for lead, units in ((0, cand), (0, cand), (1, cand[:10]), (2, cand[:13]), (3, cand[:11])):
            w = [_expect(u, W_TEST) for u in units]
            st, rec, split, rec4, rec8, imgs, align = _decode(mic, torch, sess, units, lead=lead)
            _check(units, w, st, rec, rec4, rec8, imgs)
            seen |= set(align)
            if units is cand:                                                 # two consecutive decodes: the same records, the same pixels
                if first is None:
                    first = (list(st), rec, rec4, rec8, imgs)
                else:
                    assert (list(st), rec, rec4, rec8) == first[:4] and all(np.array_equal(a, b) for a, b in zip(imgs, first[4]))
        assert seen == {0, 1, 2, 3}                                           # an eight-part unit's bitstream at each of the four byte offsets
    finally:
        sess.close()


def test_units_the_eight_part_instance_hands_back(mic, mico, synth, gpu_ready):
    """no meeting at boundary 7, 2 and 3: the units go to the end of the four-part list, behind one k_dec_classify put there, and come
    out with the four-part instance's record -- joined, or handed on to the unsplit instance -- among eight-part units that join"""
    torch = pytest.importorskip("torch")
    back = [_unit(mico, synth, seed, rows) for seed, rows in HANDED_BACK]
    good = [_unit(mico, synth, seed, rows) for seed, rows in CANDIDATES[:4]]
    four = _unit(mico, synth, 5, 24)                                          # 60 k tokens: a four-part unit by the classifier
    fails = [M8.split8(u.model, W_TEST, R=M8.region(u.img.size))[::2] for u in back]
    assert fails == [(M.NOT_MET, 7), (M.NOT_MET, 2), (M.NOT_MET, 3)], fails
    units = [good[0], back[0], good[1], four, back[1], good[2], back[2], good[3]]
    want = [_expect(u, W_TEST) for u in units]
    assert want[1][0][0] == M.DONE and want[1][0][3] > 0 and want[1][1][5] == 4, want[1]    # (13, 52): a four-part DONE record
    assert M8.route(four.model, MIN_TEST, MIN4_TEST, MIN8_TEST) == M.FOUR_PARTS and want[3][0][0] == M.DONE
    assert sorted(w[1][5] for w in want) == [4, 4, 4, 4, 8, 8, 8, 8]
    sess = mic.Session(len(units), max(u.img.size for u in units))
    try:
        _configure(mic, sess)
        for _ in range(2):
            st, rec, split, rec4, rec8, imgs, _ = _decode(mic, torch, sess, units)
            _check(units, want, st, rec, rec4, rec8, imgs)
    finally:
        sess.close()


def test_a_stream_shorter_than_the_overlap_beside_a_longer_one(mic, mico, synth, gpu_ready):
    """the per-stream chunk cap: the hand-over after W = 65536 symbols lies behind everything a 60 k-token strip has to decode, but
    inside its 100 k-token neighbour's chunks, so the wave's loop runs up to the hand-over all the same; the short unit is not met at
    boundary 1 (no hand-over of its own) and is handed back to the four-part instance, which finds the same; the long one is recorded
    as modelled -- its regions hold no overlap steps, so an overlap of most of the stream costs it no room"""
    torch = pytest.importorskip("torch")
    W = 65536
    units = [_unit(mico, synth, 5, 24), _unit(mico, synth, 9, 40)]
    cfg = dict(min_tokens8=32768)                                             # (a unit shorter than 65536 - 32 tokens on the eight-part list)
    assert W // 16 >= units[0].ntok // 16 + 2 and W // 16 < units[1].ntok // 16 + 2, [u.ntok for u in units]
    assert all(M8.route(u.model, MIN_TEST, MIN4_TEST, 32768) == M8.EIGHT_PARTS for u in units)
    assert M8.split8(units[0].model, W, R=M8.region(units[0].img.size)) == (M.NOT_MET, (0,) * 7, 1)
    want = [_expect(u, W, **cfg) for u in units]
    assert want[0][0][:2] == (M.NOT_MET, (0, 0, 0)) and want[0][0][4] == 1 and want[0][1][5] == 4, want
    sess = mic.Session(len(units), max(u.img.size for u in units))
    try:
        _configure(mic, sess, overlap=W, **cfg)
        st, rec, split, rec4, rec8, imgs, _ = _decode(mic, torch, sess, units)
        _check(units, want, st, rec, rec4, rec8, imgs)
    finally:
        sess.close()


def test_routing_between_the_three_instances(mic, mico, synth, gpu_ready):
    """one unit under min_tokens8 keeps its four-part record, one under min_tokens4 its two-part record, one is under the rate gate"""
    torch = pytest.importorskip("torch")
    eight, four, two = _unit(mico, synth, 5, 48), _unit(mico, synth, 5, 24), _unit(mico, synth, 7, 16)
    quiet = _unit(mico, synth, 3, 48, noise=3.0)
    units = [eight, four, two, quiet]
    assert [M8.route(u.model, MIN_TEST, MIN4_TEST, MIN8_TEST) for u in units] == [M8.EIGHT_PARTS, M.FOUR_PARTS, M.TWO_PARTS, M.UNSPLIT]
    assert quiet.ntok >= MIN8_TEST and MIN4_TEST <= four.ntok < MIN8_TEST and MIN_TEST <= two.ntok < MIN4_TEST
    want = [_expect(u, W_TEST) for u in units]
    assert [w[1][5] for w in want] == [8, 4, 2, 0] and want[1][0][0] == M.DONE and want[1][0][3] > 0
    want2 = [S2._expect(two, W_TEST), (M.NOT_TRIED, 0, 0)]
    assert want2[0][0] == M.DONE
    sess = mic.Session(len(units), max(u.img.size for u in units))
    try:
        _configure(mic, sess)
        st, rec, split, rec4, rec8, imgs, _ = _decode(mic, torch, sess, units)
        _check(units, want, st, rec, rec4, rec8, imgs)
        assert [split[2], split[3]] == want2, split                           # the two-part record, and none
    finally:
        sess.close()


def test_a_damaged_stream_is_judged_as_without_the_split(mic, mico, synth, gpu_ready):
    """a stream cut at its end, and one with a bit flipped in part 5's range, among whole neighbours: status and pixels are those of
    the same session's unsplit decode of the same bytes, and the oracle's status"""
    torch = pytest.importorskip("torch")
    cand = [_unit(mico, synth, seed, rows) for seed, rows in CANDIDATES[:5]]
    victim = 2
    u = cand[victim]
    nbytes = len(u.blob) - u.hdr_len
    cut = u.blob[:u.hdr_len] + u.blob[u.hdr_len + 300:]                       # the bytes read last are gone: the count runs past bit 0
    starts = M.starts(u.model, W_TEST, 8)
    at = (starts[5] + starts[6]) // 16                                        # a byte half way down part 5's own range
    assert starts[6] // 8 + 600 < at < starts[5] // 8 - 600 and at < nbytes
    flip = bytearray(u.blob)
    flip[u.hdr_len + at] ^= 0x08
    sess = mic.Session(len(cand), max(x.img.size for x in cand))
    try:
        for bad in (cut, bytes(flip)):
            rc_o, _ = mico.decompress_single_frame(bad, *u.dims)
            blobs = [bad if i == victim else x.blob for i, x in enumerate(cand)]
            _configure(mic, sess, min_tokens=1 << 30)                         # nothing is split
            st0, rec0, split0, rec40, rec80, imgs0, _ = _decode(mic, torch, sess, cand, blobs=blobs)
            assert all(s[0] == M.NOT_TRIED for s in split0) and all(r[3] == 0 and r[5] == 0 for r in rec80)
            _configure(mic, sess)
            st1, rec1, split1, rec41, rec81, imgs1, _ = _decode(mic, torch, sess, cand, blobs=blobs)
            assert split1[victim][0] != M.NOT_TRIED and rec81[victim][5] in (4, 8), rec81
            assert sum(r[0] == M.DONE and r[5] == 8 for r in rec81) >= 4, rec81
            assert list(st1) == list(st0) and st1[victim] == rc_o, (list(st0), list(st1), rc_o)
            for i, x in enumerate(cand):
                if st1[i] == 0:
                    assert np.array_equal(imgs1[i], imgs0[i]), i
                if i != victim:
                    assert st1[i] == 0 and np.array_equal(imgs1[i], x.img), i
    finally:
        sess.close()


def _falling(mico, synth, seed, rows, top_rows, top=400.0, low=4.0):
    """a strip whose noise falls towards the bottom: the stream's last bits are spent on quiet rows, many tokens for an eighth of the bits"""
    return Unit(mico, np.ascontiguousarray(np.vstack([_strip(synth, seed, rows, noise=top)[:top_rows], _strip(synth, seed, rows, noise=low)[top_rows:]])))


def test_a_last_part_longer_than_its_region_is_handed_back(mic, mico, synth, gpu_ready):
    """NO_ROOM at the stream's end, from a search on the CPU model (noise 400 over 51 rows, 4 over the 13 below: 160 k tokens): all
    seven joins are met, the last part has more than R steps behind W, the unit comes out with the four-part instance's record, and
    the unit beside it, whose last part ends 98 tokens inside its region (noise 8 below), joins as eight parts"""
    torch = pytest.importorskip("torch")
    units = [_falling(mico, synth, 5, 64, 51), _falling(mico, synth, 5, 64, 51, low=8.0), _unit(mico, synth, 5, 48)]
    R = M8.region(units[0].img.size)
    o, I, f = M8.split8(units[0].model, W_TEST, R=R)
    assert (o, f) == (M.NO_ROOM, 8) and units[0].ntok - I[6] > R and units[0].ntok < 200000, (o, I, f, R)
    assert all(M8.route(u.model, MIN_TEST, MIN4_TEST, MIN8_TEST) == M8.EIGHT_PARTS for u in units)
    want = [_expect(u, W_TEST) for u in units]
    assert want[0][1][5] == 4 and want[0][0][0] == M.DONE, want[0]            # the four-part instance joins it
    assert want[1][1][0] == M.DONE and want[1][1][5] == 8 and 0 <= R - (units[1].ntok - want[1][1][1][6]) < 128, want[1]
    sess = mic.Session(len(units), max(u.img.size for u in units))
    try:
        _configure(mic, sess)
        for _ in range(2):
            st, rec, split, rec4, rec8, imgs, _ = _decode(mic, torch, sess, units)
            _check(units, want, st, rec, rec4, rec8, imgs)
    finally:
        sess.close()
