"""Every lane-per-state tANS decode class (k_dec_tans_ls<N, ZB, TL>, csrc/mic_decode_ls.hip) at its wave and chunk seams, and a
record of WHICH kernel decoded each unit.

The streams come from tests/decode_class_streams.py: made by the oracle on the CPU, one batch per (table-size class, states, 0-bit
entries) of `a full group + a full wave + one stream beside its clones`, every slot of every wave holding a stream of its own length.
What a unit's class is, is worked out here from the oracle's facts of the stream and a Python restatement of mic_dec_cls -- the
library is only asked which kernel ran (MicUnit.dec_kernel through the debug probe): a class kernel that never ran, or declined its
units, would otherwise pass everything, because k_dec_tans_gl / k_dec_tans_serial take what is left.

Every batch is decoded by a fresh session (launch mask all ones) and again by the same session (the mask has learned and is narrow),
bit-exact against the source images."""
import ctypes as C

import numpy as np
import pytest

import decode_class_streams as D

pytestmark = pytest.mark.gpu

CLASSES = [(b, n, zb) for b in D.BUCKETS for n in (2, 4, 8) for zb in (0, 1)]


def _decode(mic, torch, sess, units, blobs=None, lead=0):
    """one decode_enqueue / decode_finish of the units' blobs laid end to end from byte `lead` of a device buffer on:
    (status, dec_kernel, probe words, images, (address of the bitstream) & 3) per unit"""
    blobs = [u.blob for u in units] if blobs is None else blobs
    offs = np.zeros(len(units) + 1, np.uint64)
    offs[0] = lead
    offs[1:] = lead + np.cumsum([len(b) for b in blobs])
    host = np.zeros(int(offs[-1]) + 64, np.uint8)
    host[lead:int(offs[-1])] = np.frombuffer(b"".join(blobs), np.uint8)
    d_blobs = torch.from_numpy(host).cuda()
    px = np.concatenate([[0], np.cumsum([u.img.size for u in units])]).astype(np.int64)
    tab = mic.Session.make_units([(int(px[i]), u.dims[0], u.dims[1], u.maxv, 2) for i, u in enumerate(units)])
    d_out = torch.zeros(int(px[-1]), dtype=torch.int16, device="cuda")
    sess.decode_enqueue(d_blobs.data_ptr(), offs, tab, d_out.data_ptr())
    st = sess.decode_finish()
    words = []
    for i in range(len(units)):
        buf = (C.c_uint32 * 32)()
        assert mic.lib().mic_hip_debug_unit(sess._h, i, buf) == 0
        words.append(list(buf))
    out = d_out.cpu().numpy().view(np.uint16)
    imgs = [out[px[i]:px[i + 1]].reshape(u.img.shape) for i, u in enumerate(units)]
    align = [(d_blobs.data_ptr() + int(offs[i]) + u.hdr_len) & 3 for i, u in enumerate(units)]
    return st, [w[15] for w in words], words, imgs, align


def _check_exact(units, st, rec, words, imgs, skip=()):
    for i, u in enumerate(units):
        if i in skip:
            continue
        # the device's own parse of the header against the oracle's facts, then who decoded, then the pixels
        assert (words[i][2], words[i][6], words[i][7], words[i][9]) == (u.table_log, u.zero_bits, u.flavour, u.hdr_len), (i, words[i][:16])
        assert st[i] == 0 and rec[i] == u.record, (i, st[i], rec[i], u.record, u.ntok)
        assert words[i][0] == u.ntok, (i, words[i][0], u.ntok)
        assert np.array_equal(imgs[i], u.img), (i, u.ntok)


def _check_shape_of_batch(mico, units, bucket, flavour, zb):
    """the CPU side: every stream made it through the oracle into the intended class, and the batch has the seams it is there for"""
    spw, waves = D.GEOM[bucket]
    assert len(units) == spw * waves + spw + 1
    for u in units:
        assert u.rc == 0 and u.zero_bits == zb and D.states(u.flavour) == D.states(flavour)
        assert (u.table_log <= 12) if bucket == 12 else (u.table_log == bucket)
        assert u.cls == D.dec_cls(flavour, bucket, zb) and u.img.shape[1] <= 1008
        assert u.record == (D.BY_GL if (bucket == 16 and zb) else u.cls + 1)
    chunks = [u.ntok // D.CHUNK for u in units]
    for wave in range(waves + 1):                                           # the full waves: a group's, and the next group's first
        c = chunks[wave * spw:(wave + 1) * spw]
        if bucket == 12 and wave == 0:
            assert max(c) == 0                                              # no whole chunk in the wave at all
            continue
        assert len(set(c)) == spw, (wave, c)                                # lengths differ by whole chunks ...
        assert c.index(min(c)) == wave % spw, (wave, c)                     # ... and the shortest takes each slot in turn
    tails = {u.ntok % D.CHUNK for u in units}
    if bucket <= 14:
        assert tails >= set(D.tail_residues(flavour)), tails
    if bucket in (13, 14):                                                  # k_dec_translate's tile, k_dec_translate_wide's vector tail
        assert {D.TILE - 1, 0, 1} <= {u.ntok % D.TILE for u in units} and any(u.ntok % 8 for u in units)
    if bucket == 12:
        assert [units[i].ntok for i in (5, 10)] == [43, 43] and min(units[i].ntok for i in (4, 6, 7)) > 2000
        assert [units[i].table_log for i in (8, 9, 10, 11)] == [9, 9, 5, 12]
    if bucket == 16 and not zb:
        assert units[0].maxv == 65535 and units[0].ntok > 262144 and len(units[0].blob) > units[0].ntok   # over a byte a token on average
        assert D.worst_chunk_dwords(mico, units[0], 16) >= 63               # a chunk that takes a whole block of 64 dwords off the ring


@pytest.mark.parametrize("bucket,flavour,zb", CLASSES + [(14, 108, 0)])
def test_a_batch_of_one_class_is_decoded_by_that_class(mic, mico, gpu_ready, bucket, flavour, zb):
    torch = pytest.importorskip("torch")
    units = D.class_batch(mico, bucket, flavour, zb)
    _check_shape_of_batch(mico, units, bucket, flavour, zb)
    if bucket in (15, 16):                                                  # four and three units: the six tails over the two batches
        both = D.class_batch(mico, 15, flavour, zb) + D.class_batch(mico, 16, flavour, zb)
        assert {u.ntok % D.CHUNK for u in both} >= set(D.tail_residues(flavour))
    sess = mic.Session(len(units), max(u.img.size for u in units))
    try:
        seen = set()
        for lead in ((0, 0, 1, 2, 3) if bucket == 13 else (0, 0)):           # first: mask all ones; then narrow.  tableLog 13: every
            st, rec, words, imgs, align = _decode(mic, torch, sess, units, lead=lead)   # unit's bitstream at each of the four byte offsets
            _check_exact(units, st, rec, words, imgs)
            seen |= set(align)
        if bucket == 13:
            assert seen == {0, 1, 2, 3}
    finally:
        sess.close()


@pytest.mark.parametrize("bucket,flavour,zb", [c for c in CLASSES if c[1] in (2, 8)])
def test_a_damaged_unit_in_a_full_wave_hurts_nobody_else(mic, mico, gpu_ready, bucket, flavour, zb):
    """the last unit of the full group gets a moved end mark, then changed payload bytes: its verdict and its pixels are the oracle's,
    its neighbours' are untouched"""
    torch = pytest.importorskip("torch")
    units = D.class_batch(mico, bucket, flavour, zb)
    spw, waves = D.GEOM[bucket]
    victim = spw * waves - 1
    sess = mic.Session(len(units), max(u.img.size for u in units))
    try:
        for way in D.DAMAGE:
            bad = D.damaged(units[victim], way)
            rc_o, want = mico.decompress_single_frame(bad, *units[victim].dims)
            blobs = [bad if i == victim else u.blob for i, u in enumerate(units)]
            for again in range(2):
                st, rec, words, imgs, _ = _decode(mic, torch, sess, units, blobs=blobs)
                _check_exact(units, st, rec, words, imgs, skip=(victim,))
                assert st[victim] == rc_o, (way, again, st[victim], rc_o)
                if rc_o == 0:
                    assert np.array_equal(imgs[victim], want), (way, again)
    finally:
        sess.close()


def test_classification_carries_its_bases_past_1024_units(mic, mico, gpu_ready):
    """k_dec_classify compacts its per-class lists in passes of 1024 units: six classes, rANS-8 and 1-state streams unit by unit on
    both sides of unit 1024"""
    torch = pytest.importorskip("torch")
    units = D.tiny_batch(mico)
    assert len(units) > 1024 + 64 and all(u.rc == 0 and u.table_log <= 12 for u in units)
    for part in (units[:1024], units[1024:]):
        assert len({u.cls for u in part} - {-1}) == 6 and any(u.flavour == 1 for u in part) and any(u.flavour == 108 for u in part)
    assert all(u.record == D.BY_SERIAL for u in units if u.flavour == 1)
    assert all(units[i].cls != units[i + 1].cls for i in range(len(units) - 1))
    got = mic.decompress_batch([u.blob for u in units], [u.dims for u in units])
    for i, (u, (st, px)) in enumerate(zip(units, got)):
        assert st == 0 and np.array_equal(px, u.img), i
    sess = mic.Session(len(units), max(u.img.size for u in units))
    try:
        for again in range(2):
            st, rec, words, imgs, _ = _decode(mic, torch, sess, units)
            _check_exact(units, st, rec, words, imgs)
    finally:
        sess.close()
