"""The partner waves of the eight-part instance of the two-state tANS chain (k_dec_tans_ls_parts<8>, csrc/mic_decode_ls.hip): a group is
three chain waves and three partner waves, and a partner does its chain wave's per-chunk upkeep -- ring fills and state stores --
through a mailbox in LDS (the comment above the kernel; tests/tans_partner_model.py for the deadline).

Units, thresholds and helpers are those of tests/test_gpu_tans_split8.py (strips of 2577 x 24 .. 72, 60 - 180 k tokens; W 8192; 65536 /
49152 / 4096 tokens for eight, four and two parts).  Every case checks pixels bit for bit, status 0, the eight-part record against the
CPU model as that file does, and the new read-out, MicUnit.partner through mic_hip_debug_partner: the upkeep was a partner's, it
served exactly the chunks the model says the unit's parts ran, and nothing stalled.  The shapes a case is there for are asserted on
the CPU side, in front of the GPU run."""
import ctypes as C

import numpy as np
import pytest

import tans_partner_model as PM
import tans_split_model as M
import tans_split8_model as M8
import test_gpu_tans_split8 as S8

pytestmark = pytest.mark.gpu

W_TEST, MIN_TEST, MIN4_TEST, MIN8_TEST = S8.W_TEST, S8.MIN_TEST, S8.MIN4_TEST, S8.MIN8_TEST
_unit, _configure, _decode, _expect, _check = S8._unit, S8._configure, S8._decode, S8._expect, S8._check


def _lib(mic):
    L = S8._lib(mic)
    L.mic_hip_debug_partner.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mic_hip_debug_partner_config.argtypes = [C.c_void_p, C.c_uint32]
    return L


def _partner(mic, sess, n):
    """MicUnit.partner per unit: (who did the upkeep, chunks the partner served, chunks its chain wave found it not ready for, stalled)"""
    out = []
    for i in range(n):
        buf = (C.c_uint32 * 4)()
        assert _lib(mic).mic_hip_debug_partner(sess._h, i, buf) == 0
        out.append(tuple(int(v) for v in buf))
    return out


def _chunks(u, overlap=W_TEST):
    key = ("chunks", overlap)
    if key not in u.expected:
        u.expected[key] = PM.chunks_run(u.model, overlap)
    return u.expected[key]


def _pool(mico, synth):
    return [_unit(mico, synth, seed, rows, res) for seed, rows, res in S8.RESIDUES] + [_unit(mico, synth, seed, rows) for seed, rows in S8.CANDIDATES]


def _check_partner(units, want, got, eight_part_list=None):
    """of a unit the eight-part instance ran (joined or handed back for the stream's sake): a partner's upkeep, all its chunks, no stall"""
    for i, u in enumerate(units):
        on_list = want[i][1][5] == 8 if eight_part_list is None else eight_part_list[i]
        if on_list:
            assert got[i][0] == 1 and got[i][1] == _chunks(u) and got[i][3] == 0, (i, got[i], _chunks(u))
        else:
            assert got[i] == (0, 0, 0, 0), (i, got[i])


def _run(mic, torch, sess, units, want=None, **kw):
    want = want or [_expect(u, W_TEST) for u in units]
    st, rec, split, rec4, rec8, imgs, align = _decode(mic, torch, sess, units, **kw)
    _check(units, want, st, rec, rec4, rec8, imgs)
    return (list(st), rec, rec4, rec8, _partner(mic, sess, len(units))), imgs


@pytest.mark.parametrize("n", [1, 2, 3, 4, 9, 10, 19])
def test_wave_and_group_occupancy(mic, mico, synth, gpu_ready, n):
    """one stream beside two clones; two; a full wave; a group with one working chain wave and one lane group of the second (the third
    chain wave and its partner leave at once); a full group; a second group of one; a third group of one stream"""
    torch = pytest.importorskip("torch")
    pool = _pool(mico, synth)
    units = [pool[i % len(pool)] for i in range(n)]
    want = [_expect(u, W_TEST) for u in units]
    assert all(w[1][0] == M.DONE and w[1][5] == 8 for w in want)
    assert len({_chunks(u) for u in units[:3]}) == min(n, 3)                  # neighbours of a wave end at different chunks
    sess = mic.Session(n, max(u.img.size for u in units))
    try:
        _configure(mic, sess)
        recs, _ = _run(mic, torch, sess, units, want)
        _check_partner(units, want, recs[4])
    finally:
        sess.close()


def test_unequal_neighbours_in_each_slot_of_a_wave(mic, mico, synth, gpu_ready):
    """the fastest consumer found (11.66 bits per token), the published strip (9.57) and a strip half as long again, in each of a wave's
    three stream slots: the partner serves the longest on behind the others' ends, whose stores are dropped behind their last chunk"""
    torch = pytest.importorskip("torch")
    fast, pub, tall = _unit(mico, synth, 5, 48, None, 800.0), _unit(mico, synth, 5, 48), _unit(mico, synth, 17, 72)
    assert fast.model.bits / fast.model.count >= 11.5 and abs(pub.model.bits / pub.model.count - 9.57) < 0.01
    assert _chunks(tall) > _chunks(fast) + 400 and _chunks(fast) != _chunks(pub)
    sess = mic.Session(3, tall.img.size)
    try:
        _configure(mic, sess)
        for units in ([fast, pub, tall], [pub, tall, fast], [tall, fast, pub]):
            want = [_expect(u, W_TEST) for u in units]
            assert all(w[1][0] == M.DONE and w[1][5] == 8 for w in want), want
            recs, _ = _run(mic, torch, sess, units, want)
            _check_partner(units, want, recs[4])
    finally:
        sess.close()


def test_ends_in_either_stage_half_and_timing_independence(mic, mico, synth, gpu_ready):
    """token counts 0, 1 and 15 modulo 16 and chunk counts of both parities (the last chunk's states leave from either stage half);
    the batch three times in one session and once in a fresh one, and every unit alone: the same records, the same pixels"""
    torch = pytest.importorskip("torch")
    units = _pool(mico, synth)
    want = [_expect(u, W_TEST) for u in units]
    assert [u.ntok % 16 for u in units[:3]] == [0, 1, 15]
    assert {_chunks(u) & 1 for u in units} == {0, 1}
    first = None
    for fresh in range(2):
        sess = mic.Session(len(units), max(u.img.size for u in units))
        try:
            _configure(mic, sess)
            for _ in range(1 if fresh else 3):
                recs, imgs = _run(mic, torch, sess, units, want)
                _check_partner(units, want, recs[4])
                recs = recs[:4] + ([p[:2] + p[3:] for p in recs[4]],)        # (the not-ready count is the one thing timing may move)
                if first is None:
                    first = (recs, imgs)
                else:
                    assert recs == first[0] and all(np.array_equal(a, b) for a, b in zip(imgs, first[1]))
            if fresh:
                for i, u in enumerate(units):                                 # alone: a lone stream beside clones, the same record
                    r1, im1 = _run(mic, torch, sess, [u], [want[i]])
                    assert [x[0] for x in r1[:4]] == [x[i] for x in first[0][:4]] and r1[4][0][:2] == first[0][4][i][:2]
                    assert np.array_equal(im1[0], first[1][i])
        finally:
            sess.close()


def test_a_damaged_stream_among_good_neighbours(mic, mico, synth, gpu_ready):
    """a unit the eight parts do not join, and a cut stream, each in a wave with two good streams: the neighbours' partners serve them
    whole, the handed-back unit carries the four-part record, the cut one the oracle's status"""
    torch = pytest.importorskip("torch")
    good = [_unit(mico, synth, seed, rows) for seed, rows in S8.CANDIDATES[:4]]
    back = _unit(mico, synth, *S8.HANDED_BACK[0])
    victim = _unit(mico, synth, *S8.CANDIDATES[4])
    assert M8.split8(back.model, W_TEST, R=M8.region(back.img.size))[::2] == (M.NOT_MET, 7)
    units = [good[0], back, good[1], good[2], victim, good[3]]               # waves: (good, back, good), (good, cut, good)
    want = [_expect(u, W_TEST) for u in units]
    assert [w[1][5] for w in want] == [8, 4, 8, 8, 8, 8]
    cut = victim.blob[:victim.hdr_len] + victim.blob[victim.hdr_len + 300:]
    rc_o, _ = mico.decompress_single_frame(cut, *victim.dims)
    assert rc_o != 0
    on_list = [True] * len(units)                                             # (the handed-back unit ran its chunks there first)
    sess = mic.Session(len(units), max(u.img.size for u in units))
    try:
        _configure(mic, sess)
        recs, _ = _run(mic, torch, sess, units, want)
        _check_partner(units, want, recs[4], on_list)
        blobs = [cut if u is victim else u.blob for u in units]
        st, rec, split, rec4, rec8, imgs, _ = _decode(mic, torch, sess, units, blobs=blobs)
        got = _partner(mic, sess, len(units))
        for i, u in enumerate(units):
            if u is victim:
                assert st[i] == rc_o and got[i][0] == 1 and got[i][3] == 0, (st[i], rc_o, got[i])
                continue
            _check([u], [want[i]], [st[i]], [rec[i]], [rec4[i]], [rec8[i]], [imgs[i]])
            assert got[i][0] == 1 and got[i][1] == _chunks(u) and got[i][3] == 0, (i, got[i])
    finally:
        sess.close()


def test_a_chain_wave_that_gives_up_hands_its_units_to_the_four_part_instance(mic, mico, synth, gpu_ready):
    """the wait bound at its minimum: a chain wave that finds its partner not ready gives up at the first poll.  A unit's record is then
    the eight-part DONE record, or, with the stalled mark, what the four-part model says; pixels and status are right either way;
    the call returns, and the next call, at the default bound, joins every unit as eight parts with no stall"""
    torch = pytest.importorskip("torch")
    units = _pool(mico, synth)
    want = [_expect(u, W_TEST) for u in units]
    Wr = W_TEST & ~63
    want4 = []
    for u in units:
        R4 = M.region(u.img.size)
        o, I, f = M.split_parts(u.model, W_TEST, R=R4, n=4)
        want4.append(((o, I, Wr, R4, f), (o, (0,) * 7, Wr, 0, 0, 4)))
    assert all(w[1][0] == M.DONE and w[1][5] == 8 for w in want)
    sess = mic.Session(len(units), max(u.img.size for u in units))
    try:
        _configure(mic, sess)
        assert _lib(mic).mic_hip_debug_partner_config(sess._h, 1) == 0
        st, rec, split, rec4, rec8, imgs, _ = _decode(mic, torch, sess, units)
        got = _partner(mic, sess, len(units))
        for i, u in enumerate(units):
            stalled = got[i][3] == 1
            assert got[i][0] == 1 and got[i][3] in (0, 1), (i, got[i])
            if stalled:
                assert got[i][2] >= 1 and got[i][1] <= _chunks(u), (i, got[i])
            else:
                assert got[i][1] == _chunks(u), (i, got[i])
            _check([u], [want4[i] if stalled else want[i]], [st[i]], [rec[i]], [rec4[i]], [rec8[i]], [imgs[i]])
        for k in range(0, len(units), 3):                                     # a wave gives up as one
            assert len({g[3] for g in got[k:k + 3]}) == 1, got[k:k + 3]
        assert _lib(mic).mic_hip_debug_partner_config(sess._h, 0) == 0       # the default again
        recs, _ = _run(mic, torch, sess, units, want)
        _check_partner(units, want, recs[4])
    finally:
        sess.close()
