"""The two-state round of k_dec_tans_ls (LS_CHUNK2, csrc/mic_decode_ls.hip) where its early window read could go wrong.

A round takes its 32-bit window from three ring dwords read a round earlier, so what matters is how far the bit position moves
from one round to the next and where it stands against the dword grid.  tests/tans2_round_streams.py makes, with the oracle on
the CPU, streams that put the extremes side by side -- rounds of 2 * tableLog bits, rounds of no bits at all followed by the largest
step, chunks that take the whole per-chunk budget off the ring, neighbours that end chunks earlier -- and asserts there, from the
oracle's own counts, that each stream has the property it is named after.

Every batch is decoded by a fresh session and again by the same session, bit for bit against the source images, at every byte
alignment of the bitstream where the case says so; MicUnit.dec_kernel (through the debug probe) must name the two-state instance of
the stream's table-size class -- k_dec_tans_gl for tableLog 16 with 0-bit entries, which mic_dec_cls gives to no lane-per-state
class.  All classes share the macro, so the cases run at tableLog 13 and once each at 12, 14, 15 and 16."""
import ctypes as C

import numpy as np
import pytest

import decode_class_streams as D
import tans2_round_streams as T

pytestmark = pytest.mark.gpu

TABLE_LOGS = (13, 12, 14, 15, 16)
BUDGET_15 = 4 * 15                # dwords a chunk of 128 tokens takes off the ring at the most at tableLog 15 (LsGeom)


def _decode(mic, torch, sess, units, lead=0):
    """one decode_enqueue / decode_finish of the units' blobs laid end to end from byte `lead` of a device buffer on:
    (status, dec_kernel, images, (address of the bitstream) & 3) per unit"""
    blobs = [u.blob for u in units]
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
    rec = []
    for i in range(len(units)):
        buf = (C.c_uint32 * 32)()
        assert mic.lib().mic_hip_debug_unit(sess._h, i, buf) == 0
        rec.append(buf[15])
    out = d_out.cpu().numpy().view(np.uint16)
    imgs = [out[px[i]:px[i + 1]].reshape(u.img.shape) for i, u in enumerate(units)]
    align = [(d_blobs.data_ptr() + int(offs[i]) + u.hdr_len) & 3 for i, u in enumerate(units)]
    return st, rec, imgs, align


def _round_trips(mic, torch, units, leads=(0,)):
    """a fresh session, then the same one again (its launch mask has learned), for every lead: exact pixels, the expected kernel"""
    for u in units:
        assert u.flavour == 2 and u.record == (D.BY_GL if (u.table_log == 16 and u.zero_bits) else u.cls + 1)
    seen = set()
    sess = mic.Session(len(units), max(u.img.size for u in units))
    try:
        for lead in (leads[0],) + tuple(leads):
            st, rec, imgs, align = _decode(mic, torch, sess, units, lead=lead)
            for i, u in enumerate(units):
                assert st[i] == 0 and rec[i] == u.record, (lead, i, st[i], rec[i], u.record)
                assert np.array_equal(imgs[i], u.img), (lead, i, u.ntok)
            seen |= set(align)
    finally:
        sess.close()
    return seen


def _rare(mico, table_log):
    s = T.stream(mico, "rare", table_log)
    at = T.rare_triples(mico, s, table_log)
    # three adjacent tokens of tableLog bits each, at several places of both token parities: a round of 2 * tableLog bits (an even
    # start) and a pair that straddles two rounds (an odd one)
    assert sum(1 for i in at if i % 2 == 0) >= 3 and sum(1 for i in at if i % 2 == 1) >= 3, at
    assert s.zero_bits == 0
    return s


def _still(mico, table_log):
    s = T.stream(mico, "still", table_log)
    at = T.still_places(mico, s, table_log)
    # sixteen dominant tokens in a row, then a rare pair: at several places, the pair starting at tokens of both parities
    assert len(at) >= 3 and {i % 2 for i in at} == {0, 1}, at
    assert s.zero_bits == 1
    return s


@pytest.mark.parametrize("table_log", TABLE_LOGS)
def test_rounds_that_take_twice_table_log_bits(mic, mico, gpu_ready, table_log):
    torch = pytest.importorskip("torch")
    s = _rare(mico, table_log)
    _round_trips(mic, torch, [s])


@pytest.mark.parametrize("table_log", TABLE_LOGS)
def test_rounds_that_take_no_bits_then_the_largest_step(mic, mico, gpu_ready, table_log):
    torch = pytest.importorskip("torch")
    s = _still(mico, table_log)
    _round_trips(mic, torch, [s])


def test_every_byte_alignment_of_the_bitstream(mic, mico, gpu_ready):
    """both kinds of stream with the blob at byte 0, 1, 2 and 3: the grid offset, and with it every dword crossing, moves by 8 bits"""
    torch = pytest.importorskip("torch")
    units = [_rare(mico, 13), _still(mico, 13)]
    seen = _round_trips(mic, torch, units, leads=(0, 1, 2, 3))
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("table_log", (13, 15, 16))
def test_ring_wraps_and_chunks_that_take_the_whole_budget(mic, mico, gpu_ready, table_log):
    torch = pytest.importorskip("torch")
    s = T.stream(mico, "deep" if table_log >= 15 else "noisy", table_log)
    assert len(s.blob) - s.hdr_len > 4 * 1024                               # the 256-dword ring (1 KiB) wraps four times at least
    worst = D.worst_chunk_dwords(mico, s, table_log)
    if table_log == 15:
        assert BUDGET_15 - 2 <= worst <= BUDGET_15, worst                   # the tightest class of the three-block ring
    if table_log == 16:
        assert worst >= 63, worst                                           # a whole block of 64 dwords in one chunk
    _round_trips(mic, torch, [s])


def test_neighbours_that_end_chunks_earlier(mic, mico, gpu_ready):
    """tableLog 13: the three streams of a wave end 0, 2 and 5 chunks apart (the run-off and the restore of the shorter ones), the
    next wave holds one stream beside its clones"""
    torch = pytest.importorskip("torch")
    units = T.uneven_batch(mico)
    spw, waves = D.GEOM[13]
    assert len(units) == spw + 1 and waves >= 2
    chunks = [u.ntok // D.CHUNK for u in units]
    assert len(set(chunks[:spw])) == spw and len({u.ntok % D.CHUNK for u in units[:spw]}) == 1
    _round_trips(mic, torch, units)
