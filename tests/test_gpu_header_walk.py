"""The RLE header walks of the decode chain at their seams, one deterministic stream per seam (tests/header_walk_streams.py): a zero
header first and in the last tokens, a run without its value, a literal chunk that ends with and behind the stream, headers on both
sides of k_dec_translate's tile edge and of a walker's 64-token window, and a tile of seven runs in front of a tile without a header.

Every case goes through three doors, and MicUnit.dec_kernel (the probe of tests/test_gpu_decode_classes.py) says which one it took:
two states (k_dec_tans_ls; the walk is k_dec_translate's), one state (k_dec_tans_serial; the walk is k_dec_pixels_wg's) and
k_dec_tans_gl with its own walker.  Status and pixels are the oracle's; what the oracle makes of a case is on record in
tests/golden/header_walk_cases.json, and the CPU half holds it to that."""
import ctypes as C

import numpy as np
import pytest

import header_walk_streams as HW

PAIRS = HW.pairs()


@pytest.mark.parametrize("door,shape", PAIRS)
def test_the_oracle_codes_every_case_and_decodes_it_as_recorded(mico, synth, door, shape):
    ntok, out = HW.streams(mico, synth, door, shape)          # (asserts rc == 0 of fse_compress and the door's kernel for every case)
    assert ntok > 3072 + 1024
    assert set(out) == set(HW.CASES)
    rec = HW.golden()[f"{door}/{shape}"]
    assert rec["tokens"] == ntok
    assert {c: out[c][4] for c in HW.CASES} == rec["status"]
    assert out["clean"][4] == 0 and sum(1 for c in HW.CASES if out[c][4] != 0) >= 2
    for c in HW.CASES:                                        # a decodable case makes pixels of its own: it is not the clean stream again
        if c != "clean" and out[c][4] == 0:
            assert not np.array_equal(out[c][5], out["clean"][5]), c


def _session_decode(mic, torch, sess, blob, w, h, maxv):
    """(status, dec_kernel, pixels) of one unit through a session, as test_gpu_decode_classes reads them"""
    host = np.zeros(len(blob) + 64, np.uint8)
    host[:len(blob)] = np.frombuffer(blob, np.uint8)
    d_blob = torch.from_numpy(host).cuda()
    d_out = torch.zeros(w * h, dtype=torch.int16, device="cuda")
    sess.decode_enqueue(d_blob.data_ptr(), np.array([0, len(blob)], np.uint64), mic.Session.make_units([(0, w, h, maxv, 2)]), d_out.data_ptr())
    st = sess.decode_finish()
    buf = (C.c_uint32 * 32)()
    assert mic.lib().mic_hip_debug_unit(sess._h, 0, buf) == 0
    return int(st[0]), int(buf[15]), d_out.cpu().numpy().view(np.uint16).reshape(h, w)


@pytest.mark.gpu
@pytest.mark.parametrize("case", HW.CASES)
@pytest.mark.parametrize("door,shape", PAIRS)
def test_a_header_on_a_seam_decodes_as_the_oracle_says(mic, mico, synth, gpu_ready, door, shape, case):
    """(zero_first and literal_past_last_token hold a literal chunk that reaches behind the last token while the frame has all its
    pixels in front of it: the oracle pulls a symbol when a pixel needs it and decodes them; so must k_dec_pixels_wg, which fetches
    whole tiles of symbols and judges one behind the tokens only when a pixel wants it)"""
    torch = pytest.importorskip("torch")
    w, h, blob, kernel, rc_o, want = HW.streams(mico, synth, door, shape)[1][case]
    assert rc_o == HW.golden()[f"{door}/{shape}"]["status"][case]
    try:
        got, rc_g = mic.decompress_single_frame(blob, w, h), 0
    except mic.MicError as e:
        got, rc_g = None, e.code
    assert rc_g == rc_o, (rc_g, rc_o)
    if rc_o == 0:
        assert np.array_equal(got, want), int(np.count_nonzero(got != want))
    sess = mic.Session(1, w * h)
    try:
        for again in range(2):                                # launch mask all ones, then the narrow one the session has learned
            st, rec, px = _session_decode(mic, torch, sess, blob, w, h, 255 if door == "gl" else 4095)
            assert rec == kernel, (again, rec, kernel)        # the door it was built for, and no other
            assert st == rc_o, (again, st, rc_o)
            if rc_o == 0:
                assert np.array_equal(px, want), (again, int(np.count_nonzero(px != want)))
    finally:
        sess.close()
