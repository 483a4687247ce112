"""The two tokens-to-pixels kernels at their seams, one hand-written stream per seam (tests/px_seam_streams.py; what the streams are
and that they have the properties they are named for is tests/test_px_seams_cpu.py's business):

  k_dec_pixels_wg (csrc/mic_decode_px.hip, phases 1-3): an escape pair across a tile, wave and thread edge; chains of delimiters --
  one RLE run of D -- of both parities on either side of a tile edge, and whole tiles of them; five depths; the last pixel an escape
  with and without its payload; a frame whose last symbol is 8190, 8191, 8192; a stream that goes on for more than a tile behind the
  last pixel; 5400 and 8192 segments a tile (the LDS segment table reloaded inside a tile); the three fetch forms of a thread's eight
  symbols; and the raw bits into all three predictors behind it.
  k_dec_rows_tok (csrc/mic_decode_fused.hip): 1, 511, 512, 513 and W escapes in the first, a middle and the last row; the slack cut
  short by the stream's end; a pair and a chain across a lane chunk of the marker scan; escapes at a row's end and the next one's
  start; rows of 1, 2, 8, 9 and 12 pieces, piece ends at 0, 1 and 7 mod 8 and two ends in one vector; 16 H + 64 segments and one
  more; the segment window reloaded at every residue; a run's value among the first and last eight tokens; both special forms at once.

Every case goes through the door it names -- one state (k_dec_tans_serial; k_dec_pixels_wg walks the headers and k_dec_rows_tok never
sees the unit) and two states (k_dec_translate leaves MIC_STAGE_SEGS) -- through decompress_single_frame and through a session,
twice: launch mask all ones, then the learned one.  Status and pixels are the oracle's.  The session's output tensor is 4096 pixels
longer than the frame and filled with 0xA5A5: the tail must be intact.  MicUnit.dec_stage reads MIC_STAGE_PIXELS exactly for the units
the model says k_dec_rows_tok takes, and MicUnit.px_paths (MIC_PXP_*, mic_hip_debug_px_paths) is the model's prediction bit for bit:
both kernels carry the probe (its bits are wave-uniform and cost neither of them a register, scratch or occupancy,
profiles/px_seams_resources_{parent,branch}.tsv).  A batch the small slabs cannot hold (the dense cases, the surplus) runs again in
tier 2; the record is the second run's."""
import ctypes as C

import numpy as np
import pytest

import px_seam_streams as S

CANARY = 4096
FILL = 0xA5A5


def _session_decode(mic, torch, sess, blob, w, h, maxv):
    """(status, dec_kernel, dec_stage, px_paths, pixels, the tail behind them) of one unit through a session"""
    host = np.zeros(len(blob) + 64, np.uint8)
    host[:len(blob)] = np.frombuffer(blob, np.uint8)
    d_blob = torch.from_numpy(host).cuda()
    d_out = torch.full((w * h + CANARY,), FILL - 65536, dtype=torch.int16, device="cuda")
    sess.decode_enqueue(d_blob.data_ptr(), np.array([0, len(blob)], np.uint64), mic.Session.make_units([(0, w, h, maxv, 2)]), d_out.data_ptr())
    st = sess.decode_finish()
    buf, stage, paths = (C.c_uint32 * 32)(), C.c_uint32(), C.c_uint32()
    assert mic.lib().mic_hip_debug_unit(sess._h, 0, buf) == 0
    assert mic.lib().mic_hip_debug_dec_stage(sess._h, 0, C.byref(stage)) == 0
    assert mic.lib().mic_hip_debug_px_paths(sess._h, 0, C.byref(paths)) == 0
    out = d_out.cpu().numpy().view(np.uint16)
    return int(st[0]), int(buf[15]), int(stage.value), int(paths.value), out[:w * h].reshape(h, w), out[w * h:]


@pytest.mark.gpu
@pytest.mark.parametrize("name,door", S.ids())
def test_a_seam_case_decodes_as_the_oracle_says_by_the_paths_the_model_predicts(mic, mico, gpu_ready, name, door):
    torch = pytest.importorskip("torch")
    c = S.case(name)
    w, h, blob, kernel, rc_o, want = S.coded(mico, name, door)
    assert rc_o == S.golden()[f"{name}/{door}"]["status"]
    try:
        got, rc_g = mic.decompress_single_frame(blob, w, h), 0
    except mic.MicError as e:
        got, rc_g = None, e.code
    assert rc_g == rc_o, (rc_g, rc_o)
    if rc_o == 0:
        assert np.array_equal(got, want), int(np.count_nonzero(got != want))
    paths, taken = S.expected_paths(c.facts, door)
    sess = mic.Session(1, w * h)
    try:
        for again in range(2):                                # launch mask all ones, then the narrow one the session has learned
            st, rec, stage, got_paths, px, tail = _session_decode(mic, torch, sess, blob, w, h, c.maxv)
            print(name, door, again, "status", st, "kernel", rec, "stage", stage, "paths", hex(got_paths), "model", hex(paths), taken)
            assert rec == kernel, (again, rec, kernel)        # the door it was built for, and no other
            assert st == rc_o, (again, st, rc_o)
            if rc_o == 0:
                assert np.array_equal(px, want), (again, int(np.count_nonzero(px != want)))
            assert (tail == FILL).all(), (again, int(np.count_nonzero(tail != FILL)))
            assert (stage == S.STAGE_PIXELS) == taken, (again, stage, taken)
            assert got_paths == paths, (again, hex(got_paths), hex(paths))
    finally:
        sess.close()


STALE = (("rows/escapes_512_row_4_1100", "two_state"), ("rows/one_literal_2688", "two_state"),       # k_dec_rows_tok's own raw bits (LDS)
         ("rows/escapes_513_row_4_1100", "two_state"), ("px/npx_8190_escapes_0", "two_state"),       # declined: the flag slab, then k_dec_predict
         ("px/pair_at_8191_1100x23", "one_state"), ("rows/one_literal_1100", "two_state"),            # ... k_dec_predict_rows, then k_dec_rows_tok
         ("px/dense_ones_escapes", "one_state"), ("px/npx_8190_escapes_0", "one_state"))              # (tier 2 and back to a small frame)


@pytest.mark.gpu
def test_a_clean_frame_behind_an_escape_frame_sees_none_of_its_raw_bits(mic, mico, gpu_ready):
    """one session, frame after frame: the row of 512 escapes and then a clean frame of another shape, and the same behind every other
    place raw bits are kept in -- every second frame has no escape at all"""
    torch = pytest.importorskip("torch")
    sess = mic.Session(1, max(S.case(n).w * S.case(n).h for n, _ in STALE))
    try:
        for k, (n, door) in enumerate(STALE):
            c = S.case(n)
            w, h, blob, kernel, rc_o, want = S.coded(mico, n, door)
            st, rec, stage, got_paths, px, tail = _session_decode(mic, torch, sess, blob, w, h, c.maxv)
            assert (st, rec, rc_o) == (0, kernel, 0), (n, st, rec)
            assert np.array_equal(px, want), (n, int(np.count_nonzero(px != want)))
            assert (tail == FILL).all(), n
            assert bool((c.facts.kind == S.MARKER).any()) == (k % 2 == 0), n
    finally:
        sess.close()


@pytest.mark.gpu
@pytest.mark.parametrize("door", S.DOORS)
def test_a_frame_of_two_tokens_a_pixel_decodes_in_a_session_through_either_door(mic, mico, gpu_ready, door):
    """every pixel an escape: more tokens than the small token slab holds.  A two-state stream says so in its header and the table
    kernel asks for the large slabs; a one-state stream's count is known only when k_dec_tans_serial has filled the slab, and it used
    to call the stream corrupt there (found by the dense cases above)"""
    torch = pytest.importorskip("torch")
    img, blob, kernel, tok = S.escape_heavy(mico, door)
    h, w = img.shape
    assert np.array_equal(mic.decompress_single_frame(blob, w, h), img)
    sess = mic.Session(1, w * h)
    try:
        for again in range(2):
            st, rec, stage, paths, px, tail = _session_decode(mic, torch, sess, blob, w, h, 4095)
            assert (st, rec) == (0, kernel), (again, st, rec)
            assert np.array_equal(px, img), (again, int(np.count_nonzero(px != img)))
            assert (tail == FILL).all(), again
    finally:
        sess.close()
