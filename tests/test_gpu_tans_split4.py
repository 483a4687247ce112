"""The four-part instance of the two-state tANS chain (k_dec_tans_ls_parts<4>, csrc/mic_decode_ls.hip) at its seams, on small units.

The units are strips of the headline's frame (2577 columns, 44 .. 72 rows of 12-bit xr_like at the published noise: 110 - 180 k
tokens, about 9.6 bits each), coded by the oracle; the session's four-part threshold is lowered to 65536 tokens and the overlap
set to 8192 through the debug setters so that such units take the four-part instance.  What the kernel must make of each unit --
joined or handed back, where the three joins lie and which boundary failed -- is worked out on the CPU by
tests/tans_split_model.py; the library is asked for its record (MicUnit.split through mic_hip_debug_split4) and for the
pixels, which must be the source's bit for bit.

The unit that has to stay with the two-part instance is a 24-row strip (60 k tokens): with the four-part threshold at 65536 a
90 k-token unit would be a four-part unit itself.

The shapes a case is there for are asserted on the CPU side, in front of the GPU run."""
import ctypes as C
import functools

import numpy as np
import pytest

import tans_split_model as M
import test_gpu_tans_split as S2

M4 = M                                             # (one model for both part counts; four parts are its default)

pytestmark = pytest.mark.gpu

W_TEST = 8192                                      # (with 4096 three of the twelve candidates do not meet)
MIN4_TEST = 65536
MIN_TEST = 4096                                    # the two-part gate, lowered as in test_gpu_tans_split.py
TILE = S2.TILE
Unit, _strip, _with_tokens = S2.Unit, S2._strip, S2._with_tokens

CANDIDATES = ((5, 48), (7, 56), (11, 48), (13, 52), (14, 50), (15, 54), (16, 62), (17, 72), (18, 48), (20, 60), (21, 44))
NOT_MEETING = (9, 64)                              # its parts 0 and 1 do not meet inside 8192 symbols
RESIDUES = ((30, 44, 0), (31, 46, 1), (32, 48, TILE - 1))   # (seed, rows, token count modulo 1536)


@functools.lru_cache(maxsize=None)
def _units(mico, synth):
    """fifteen four-part candidates of differing lengths -- the first three end on k_dec_translate's tile edge, one token behind it
    and one in front of it (so also on the chunk's) --, a two-part-sized strip, a strip under the rate gate and one under every
    length gate"""
    u = [Unit(mico, _with_tokens(mico, _strip(synth, seed, rows), res)) for seed, rows, res in RESIDUES]
    u += [Unit(mico, _strip(synth, seed, rows)) for seed, rows in CANDIDATES[:9] + (NOT_MEETING,) + CANDIDATES[9:]]
    two = Unit(mico, _strip(synth, 5, 24))
    quiet = Unit(mico, _strip(synth, 3, 48, noise=3.0))
    short = Unit(mico, _strip(synth, 4, 1, noise=18.0))
    return u, two, quiet, short


def _lib(mic):
    L = S2._lib(mic)
    L.mic_hip_debug_split4.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mic_hip_debug_split4_config.argtypes = [C.c_void_p, C.c_uint32]
    return L


def _configure(mic, sess, min_tokens=MIN_TEST, overlap=W_TEST, min_tokens4=MIN4_TEST):
    S2._configure(mic, sess, min_tokens=min_tokens, overlap=overlap)
    assert _lib(mic).mic_hip_debug_split4_config(sess._h, min_tokens4) == 0


def _decode(mic, torch, sess, units, blobs=None, lead=0):
    """S2._decode, and the four-part record per unit: (outcome, (I_1, I_2, I_3), W, R, failing boundary)"""
    st, rec, split, imgs, align = S2._decode(mic, torch, sess, units, blobs=blobs, lead=lead)
    rec4 = []
    for i in range(len(units)):
        out = (C.c_uint32 * 8)()
        assert _lib(mic).mic_hip_debug_split4(sess._h, i, out) == 0
        rec4.append((int(out[0]), (int(out[1]), int(out[2]), int(out[3])), int(out[4]), int(out[5]), int(out[6])))
    return st, rec, split, rec4, imgs, align


def _expect(u, overlap, min_tokens=MIN_TEST, min_tokens4=MIN4_TEST):
    """what (MicUnit.split, the four-part record) must hold of the unit (worked out once per unit and overlap)"""
    r = M4.route(u.model, min_tokens=min_tokens, min_tokens4=min_tokens4)
    if r != M4.FOUR_PARTS:
        return S2._expect(u, overlap, min_tokens=min_tokens), (S2._expect(u, overlap, min_tokens=min_tokens)[0], (0, 0, 0), None, 0, 0)
    key = ("four", overlap)
    if key not in u.expected:
        R = M4.region(u.img.size)
        o, I, fail = M4.split4(u.model, overlap, R=R)
        u.expected[key] = ((o, I[0], overlap & ~63), (o, I, overlap & ~63, R, fail))
    return u.expected[key]


def _check(units, want, st, rec, split, rec4, imgs):
    for i, u in enumerate(units):
        w2, w4 = want[i]
        assert st[i] == 0, (i, st[i])
        assert split[i] == w2, (i, split[i], w2, u.ntok)
        got4 = rec4[i] if w4[2] is not None else rec4[i][:2] + (None,) + rec4[i][3:]   # (a two-part unit: W is split[2] = j_sync, checked above)
        assert got4 == w4, (i, rec4[i], w4, u.ntok)
        if u.model.table_log == 13 and not u.model.zero_bits:
            assert rec[i] == 1, (i, rec[i])                                 # class 0's record, whichever instance ran
        assert np.array_equal(imgs[i], u.img), (i, u.ntok, rec4[i])


def test_four_part_units_join_where_the_model_says(mic, mico, synth, gpu_ready):
    torch = pytest.importorskip("torch")
    cand, two, quiet, short = _units(mico, synth)
    want = [_expect(u, W_TEST) for u in cand]
    done = [w[1] for w in want if w[1][0] == M.DONE]
    # the CPU side: the seams this batch is there for
    assert len(done) >= 9 and any(w[1][0] == M.NOT_MET and w[1][4] == 1 for w in want), want
    assert all(w[1][3] == M4.region(u.img.size) and w[1][3] > 0 for u, w in zip(cand, want))
    steps = [e for _, I, w, _, _ in done for e in (I[0], I[1] - I[0] + w, I[2] - I[1] + w)]   # e_0, e_1, e_2: the upper part's step at a join
    assert {e & 1 for e in steps} == {0, 1}                                   # the lower part's lanes in step with it, and role-swapped
    assert any(i % 8 for _, I, _, _, _ in done for i in I)                    # a join inside a translate thread's eight tokens
    assert [u.ntok % TILE for u in cand[:3]] == [0, 1, TILE - 1] and [u.ntok % 32 for u in cand[:3]] == [0, 1, 31]
    assert all(w[1][0] == M.DONE for w in want[:3])
    assert len({u.ntok // 32 for u in cand}) >= 10                            # lengths differ by whole chunks
    w_two = _expect(two, W_TEST)
    assert MIN_TEST <= two.ntok < MIN4_TEST and M4.route(two.model, MIN_TEST, MIN4_TEST) == M4.TWO_PARTS and w_two[0][0] == M.DONE
    assert quiet.ntok >= MIN4_TEST and M4.route(quiet.model, MIN_TEST, MIN4_TEST) == M4.UNSPLIT and short.ntok < MIN_TEST
    sess = mic.Session(len(cand) + 3, max(u.img.size for u in cand + [quiet]))
    try:
        _configure(mic, sess)
        seen, first = set(), None
        # 15 candidates: a full group, a full wave and a last wave of three; 10, 11: of one and two; 13: a wave of one behind a full
        # wave; mixed: a two-part unit and unsplit units in between
        for lead, units in ((0, cand), (0, cand), (1, cand[:10]), (2, cand[:11]), (3, cand[:13]),
                            (3, cand[:4] + [two] + cand[4:6] + [quiet] + cand[6:9] + [short] + cand[9:])):
            w = [_expect(u, W_TEST) for u in units]
            st, rec, split, rec4, imgs, align = _decode(mic, torch, sess, units, lead=lead)
            _check(units, w, st, rec, split, rec4, imgs)
            seen |= {a for a, x in zip(align, w) if x[1][0] == M.DONE and x[1][3]}
            if units is cand:                                                 # two consecutive decodes: the same records, the same pixels
                if first is None:
                    first = (list(st), rec, split, rec4, imgs)
                else:
                    assert (list(st), rec, split, rec4) == first[:4] and all(np.array_equal(a, b) for a, b in zip(imgs, first[4]))
        assert seen == {0, 1, 2, 3}                                           # a four-part unit's bitstream at each of the four byte offsets
    finally:
        sess.close()


# (seed, rows, overlap, boundary) whose join `boundary` lies within eight tokens of a tile edge of k_dec_translate, from a search on
# the CPU model: I mod 1536 = 3, 2, 1528, 1534
EDGE_CASES = [(11, 48, 7040, 1), (11, 48, 7872, 3), (18, 48, 7936, 3), (18, 48, 11776, 2)]


@pytest.mark.parametrize("seed,rows,overlap,boundary", EDGE_CASES)
def test_a_join_next_to_a_translate_tile_edge(mic, mico, synth, gpu_ready, seed, rows, overlap, boundary):
    torch = pytest.importorskip("torch")
    u = Unit(mico, _strip(synth, seed, rows))
    want = _expect(u, overlap)
    i = want[1][1][boundary - 1]
    assert want[1][0] == M.DONE and (i % TILE >= TILE - 8 or i % TILE < 8), want
    sess = mic.Session(1, u.img.size)
    try:
        _configure(mic, sess, overlap=overlap)
        st, rec, split, rec4, imgs, _ = _decode(mic, torch, sess, [u])
        _check([u], [want], st, rec, split, rec4, imgs)
    finally:
        sess.close()


def test_an_overlap_too_small_to_meet_in_hands_the_units_back(mic, mico, synth, gpu_ready):
    torch = pytest.importorskip("torch")
    cand = _units(mico, synth)[0][3:8]
    want = [_expect(u, 64) for u in cand]
    assert all(w[1][0] == M.NOT_MET and 1 <= w[1][4] <= 3 for w in want), want  # (64 symbols: a wrong start is forgotten in about 1500)
    sess = mic.Session(len(cand), max(u.img.size for u in cand))
    try:
        _configure(mic, sess, overlap=64)
        for _ in range(2):
            st, rec, split, rec4, imgs, _ = _decode(mic, torch, sess, cand)
            _check(cand, want, st, rec, split, rec4, imgs)
    finally:
        sess.close()


def test_a_stream_shorter_than_the_overlap_beside_a_longer_one(mic, mico, synth, gpu_ready):
    """the per-stream chunk cap: the hand-over after W = 131072 symbols lies behind everything a 110 k-token strip has to decode,
    but inside its 180 k-token neighbour's chunks; the short unit is not met at boundary 1 (no hand-over of its own), the long one
    is handed over and recorded as modelled -- a part's W steps alone overrun a region of about 70 k tokens"""
    torch = pytest.importorskip("torch")
    cand = _units(mico, synth)[0]
    W, units = 131072, [cand[14], cand[10]]
    assert [u.img.shape[0] for u in units] == [44, 72]
    want = [_expect(u, W) for u in units]
    # the CPU side: Wc against each stream's own cap; both pass the gate onto the four-part list, where they are neighbours: units 0
    # and 1 of the batch are streams 0 and 1 of the first wave
    assert W // 32 >= units[0].ntok // 32 + 2 and W // 32 < units[1].ntok // 32 + 2, [u.ntok for u in units]
    assert all(M4.route(u.model, MIN_TEST, MIN4_TEST) == M4.FOUR_PARTS for u in units)
    assert want[0][1][:2] == (M.NOT_MET, (0, 0, 0)) and want[0][1][4] == 1, want
    assert want[1][1][0] != M.NOT_TRIED and want[1][1][3] == M4.region(units[1].img.size) < W, want
    sess = mic.Session(len(units), max(u.img.size for u in units))
    try:
        _configure(mic, sess, overlap=W)
        st, rec, split, rec4, imgs, _ = _decode(mic, torch, sess, units)
        _check(units, want, st, rec, split, rec4, imgs)
    finally:
        sess.close()


def test_a_damaged_stream_is_judged_as_without_the_split(mic, mico, synth, gpu_ready):
    """a stream cut at its end, and one with a bit flipped in part 2's range, among whole neighbours: status and pixels are those
    of the same session's unsplit decode of the same bytes, and the oracle's status"""
    torch = pytest.importorskip("torch")
    cand = _units(mico, synth)[0][3:8]
    victim = 2
    u = cand[victim]
    nbytes = len(u.blob) - u.hdr_len
    cut = u.blob[:u.hdr_len] + u.blob[u.hdr_len + 300:]                       # the bytes read last are gone: the count runs past bit 0
    starts = M4.starts(u.model, W_TEST)
    at = (starts[2] + starts[3]) // 16                                        # a byte half way down part 2's own range
    assert starts[3] // 8 + 600 < at < starts[2] // 8 - 600 and at < nbytes
    flip = bytearray(u.blob)
    flip[u.hdr_len + at] ^= 0x08
    sess = mic.Session(len(cand), max(x.img.size for x in cand))
    try:
        for bad in (cut, bytes(flip)):
            rc_o, _ = mico.decompress_single_frame(bad, *u.dims)
            blobs = [bad if i == victim else x.blob for i, x in enumerate(cand)]
            _configure(mic, sess, min_tokens=1 << 30)                         # nothing is split
            st0, rec0, split0, rec40, imgs0, _ = _decode(mic, torch, sess, cand, blobs=blobs)
            assert all(s[0] == M.NOT_TRIED for s in split0) and all(r[3] == 0 for r in rec40)
            _configure(mic, sess)
            st1, rec1, split1, rec41, imgs1, _ = _decode(mic, torch, sess, cand, blobs=blobs)
            assert rec41[victim][3] > 0 and split1[victim][0] != M.NOT_TRIED, rec41
            assert sum(r[0] == M.DONE and r[3] > 0 for r in rec41) >= 3, rec41
            assert list(st1) == list(st0) and st1[victim] == rc_o, (list(st0), list(st1), rc_o)
            for i, x in enumerate(cand):
                if st1[i] == 0:
                    assert np.array_equal(imgs1[i], imgs0[i]), i
                if i != victim:
                    assert st1[i] == 0 and np.array_equal(imgs1[i], x.img), i
    finally:
        sess.close()
