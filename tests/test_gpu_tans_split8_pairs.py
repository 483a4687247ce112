"""The two-chunk pass of the eight-part instance of the two-state tANS chain (k_dec_tans_ls_parts<8>, csrc/mic_decode_ls.hip): the chain
wave tests for the loop's end in front of even chunks only, so it may run one chunk behind its parts' last one, and the partner keeps
its two blocks in registers named by block parity (tests/tans_pairs_model.py states both; tests/test_tans_pairs_cpu.py checks the
schedule on the CPU).

Units, thresholds, pools and helpers are those of tests/test_gpu_tans_split8_partner.py and tests/test_gpu_tans_split8.py (strips of
2577 x 24 .. 72; W 8192; 65536 / 49152 / 4096 tokens for eight, four and two parts).  Every case checks pixels bit for bit, status 0,
the eight-part record against the CPU model and MicUnit.partner: the chunks served are the model's chunks_run, whatever the pass
added.  The shapes a case is there for are asserted on the CPU side, in front of the GPU run.

The overlap: the library rounds it down to a multiple of 64 symbols (as the models do), so the hand-over chunk W / 16 is a multiple of
four and an odd one cannot be asked of it; the case below runs two overlaps whose hand-over chunks differ by a pass and two passes
(512, 516) -- the kernel tests for the hand-over in front of both chunks of a pass all the same."""
import numpy as np
import pytest

import tans_pairs_model as PP
import tans_partner_model as PM
import tans_split_model as M
import tans_split8_model as M8
import test_gpu_tans_split8 as S8
import test_gpu_tans_split8_partner as P8

pytestmark = pytest.mark.gpu

W_TEST, MIN_TEST, MIN4_TEST, MIN8_TEST = S8.W_TEST, S8.MIN_TEST, S8.MIN4_TEST, S8.MIN8_TEST
_unit, _configure, _decode, _expect, _check = S8._unit, S8._configure, S8._decode, S8._expect, S8._check
_lib, _partner, _chunks, _pool, _run = P8._lib, P8._partner, P8._chunks, P8._pool, P8._run


def _served(units, want, got, overlap=W_TEST):
    for i, u in enumerate(units):
        assert got[i][0] == 1 and got[i][1] == _chunks(u, overlap) and got[i][3] == 0, (i, got[i], _chunks(u, overlap))


def _steady(recs):
    """the records without the not-ready count, the one thing timing may move"""
    return recs[:4] + ([p[:2] + p[3:] for p in recs[4]],)


def test_the_hand_over_in_passes_of_either_alignment(mic, mico, synth, gpu_ready):
    torch = pytest.importorskip("torch")
    pool = _pool(mico, synth)
    units = [pool[0], pool[1], pool[3]]                                       # (pool[2] does not meet at the second overlap)
    sess = mic.Session(len(units), max(u.img.size for u in units))
    try:
        for overlap in (W_TEST, W_TEST + 64):
            assert (overlap // 16) % 2 == 0 and (overlap & 63) == 0          # (what the library makes of any overlap)
            want = [_expect(u, overlap) for u in units]
            assert all(w[1][0] == M.DONE and w[1][5] == 8 and w[1][2] == overlap for w in want), want
            _configure(mic, sess, overlap=overlap)
            recs, _ = _run(mic, torch, sess, units, want)
            _served(units, want, recs[4], overlap)
        assert {(W_TEST // 16) % 4, ((W_TEST + 64) // 16) % 4} == {0}
        assert [_chunks(u, W_TEST + 64) - _chunks(u, W_TEST) for u in units] != [0] * len(units)   # the parts end on other chunks
    finally:
        sess.close()


def test_chunk_counts_of_either_parity_and_a_unit_that_runs_to_the_cap(mic, mico, synth, gpu_ready):
    """units whose own chunk count is even and odd (the odd ones get the pass's second chunk on top), alone in their wave; then a unit
    with no hand-over inside its chunks -- every part runs to the cap, count // 16 + 2 -- beside a longer neighbour, in each of a wave's
    three stream slots: it is handed back as not met at boundary 1, as ever, and the neighbour is recorded as modelled"""
    torch = pytest.importorskip("torch")
    pool = _pool(mico, synth)
    even = next(u for u in pool if _chunks(u) % 2 == 0)
    odd = next(u for u in pool if _chunks(u) % 2 == 1)
    assert PP.chunks_pass(_chunks(odd)) == _chunks(odd) + 1 and PP.chunks_pass(_chunks(even)) == _chunks(even)
    sess = mic.Session(3, max(u.img.size for u in pool))
    try:
        _configure(mic, sess)
        for u in (even, odd):
            want = [_expect(u, W_TEST)]
            assert want[0][1][0] == M.DONE and want[0][1][5] == 8
            recs, _ = _run(mic, torch, sess, [u], want)
            _served([u], want, recs[4])
    finally:
        sess.close()
    W = 65536
    short, tall = _unit(mico, synth, 5, 24), _unit(mico, synth, 9, 40)
    cfg = dict(min_tokens8=32768)
    assert W // 16 >= short.ntok // 16 + 2 and W // 16 < tall.ntok // 16 + 2
    assert not M.Parts(short.model, W, n=8).handed and _chunks(short, W) == short.ntok // 16 + 2
    assert _chunks(tall, W) > _chunks(short, W) + 2
    assert M8.split8(short.model, W, R=M8.region(short.img.size)) == (M.NOT_MET, (0,) * 7, 1)
    R = M8.region(short.img.size)
    for c in (_chunks(short, W), _chunks(short, W) + 1):                      # its chunks behind the cap are dropped, every one
        assert PP.extra_chunk_stores(short.ntok, W, R, c)[0] is None
    sess = mic.Session(3, max(short.img.size, tall.img.size))
    try:
        _configure(mic, sess, overlap=W, **cfg)
        for units in ([short, tall, tall], [tall, short, tall], [tall, tall, short]):
            want = [_expect(u, W, **cfg) for u in units]
            st, rec, split, rec4, rec8, imgs, _ = _decode(mic, torch, sess, units)
            _check(units, want, st, rec, rec4, rec8, imgs)
            _served(units, want, _partner(mic, sess, len(units)), W)
    finally:
        sess.close()


def test_the_extra_chunk_writes_nowhere_and_timing_does_not_show(mic, mico, synth, gpu_ready):
    """a full group of nine streams whose neighbours end on different chunks, of both parities: every unit's records and pixels are
    those of the same unit decoded alone (a stray state store would land in a neighbour's tok or region and show in its pixels); the
    batch three times in one session and once in a fresh one gives the same records, the not-ready count aside, and the same pixels"""
    torch = pytest.importorskip("torch")
    units = _pool(mico, synth)[:9]
    want = [_expect(u, W_TEST) for u in units]
    assert all(w[1][0] == M.DONE and w[1][5] == 8 for w in want)
    for k in range(0, 9, 3):
        assert len({_chunks(u) for u in units[k:k + 3]}) == 3                 # neighbours of a wave end at different chunks
    assert {_chunks(u) & 1 for u in units} == {0, 1}
    first = None
    for fresh in range(2):
        sess = mic.Session(len(units), max(u.img.size for u in units))
        try:
            _configure(mic, sess)
            for _ in range(1 if fresh else 3):
                recs, imgs = _run(mic, torch, sess, units, want)
                _served(units, want, recs[4])
                if first is None:
                    first = (_steady(recs), imgs)
                else:
                    assert _steady(recs) == first[0] and all(np.array_equal(a, b) for a, b in zip(imgs, first[1]))
            if fresh:
                for i, u in enumerate(units):
                    r1, im1 = _run(mic, torch, sess, [u], [want[i]])
                    r1 = _steady(r1)
                    assert [x[0] for x in r1] == [x[i] for x in first[0]], (i, r1)
                    assert np.array_equal(im1[0], first[1][i])
        finally:
            sess.close()


def test_the_bail_out_path_under_the_two_chunk_pass(mic, mico, synth, gpu_ready):
    """the wait bound at its minimum, the library's own bounded give-up: a chain wave that finds its partner not ready gives up at its
    first poll, in front of either chunk of a pass; its units are MIC_SPLIT_STALLED, go through the four-part instance and come out
    with the right pixels; at the default bound again every unit joins as eight parts and nothing stalls"""
    torch = pytest.importorskip("torch")
    units = _pool(mico, synth)[:9]
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
        _served(units, want, recs[4])
    finally:
        sess.close()
