"""Every route of k_enc_tokens_wg (csrc/mic_encode.hip) at its seams, and a record of WHICH route ran.

The frames come from tests/tokeniser_streams.py, one session batch per group; tests/test_tokeniser_paths_cpu.py shows on the CPU
that each of them reaches the seam it is named for.  After one encode_enqueue / encode_finish every unit must agree with the oracle
on its status, on its token count and every token (mic_hip_debug_fetch_tok against DeltaRleCompressU16 / GradDeltaRleCompressU16 --
a difference is reported as the first differing token, not as "bytes differ"), on its blob byte for byte (which is what checks the
fused histogram), and on the pixels after a decode; and with the model of tests/tokeniser_paths.py on the nine route counters the
tokeniser leaves in MicUnit.tk_paths (mic_hip_debug_tok_paths): a fast tile that never fired, a vote taken a tile early, a wave that
walked serially where it should have written per lane would otherwise pass everything, because every route writes the same tokens.

Every case is compressible for the oracle (asserted on the CPU), so no unit's token count depends on what a failed entropy stage
leaves behind."""
import ctypes as C

import numpy as np
import pytest

import tokeniser_paths as M
import tokeniser_streams as S
import wavelet_ref as W

pytestmark = pytest.mark.gpu

GROUPS = tuple(S.GROUPS)


def _d2h(d_ptr, nbytes):
    host = np.empty(nbytes, np.uint8)
    assert C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(d_ptr), C.c_size_t(nbytes), 2) == 0
    return host


def _probe(mic, sess, i):
    """(ntok, status, tokens, route counters) of unit i as the session read it back"""
    L = mic.lib()
    L.mic_hip_debug_fetch_tok.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.mic_hip_debug_tok_paths.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    words = (C.c_uint32 * 32)()
    assert L.mic_hip_debug_unit(sess._h, i, words) == 0
    ntok = int(words[0])
    tok = np.zeros(max(ntok, 1), np.uint16)
    assert L.mic_hip_debug_fetch_tok(sess._h, i, tok.ctypes.data, ntok) == 0
    paths = (C.c_uint32 * len(M.NAMES))()
    assert L.mic_hip_debug_tok_paths(sess._h, i, paths) == 0
    return ntok, int(np.int32(words[11])), tok[:ntok], dict(zip(M.NAMES, (int(v) for v in paths)))


def _assert_tokens(name, got, want):
    m = min(got.size, want.size)
    bad = np.flatnonzero(got[:m] != want[:m])
    if bad.size:
        i = int(bad[0])
        raise AssertionError((name, "first differing token", i, "got", got[max(0, i - 6):i + 10].tolist(), "want", want[max(0, i - 6):i + 10].tolist()))
    assert got.size == want.size, (name, "token count", got.size, want.size)


@pytest.mark.parametrize("group", GROUPS)
def test_frames_match_the_oracle_token_by_token_on_the_route_the_model_names(mic, mico, gpu_ready, group):
    torch = pytest.importorskip("torch")
    cases = S.group(group)
    px_off = np.concatenate([[0], np.cumsum([cs.img.size for cs in cases])]).astype(np.int64)
    units = mic.Session.make_units([(int(px_off[i]), cs.img.shape[1], cs.img.shape[0], cs.maxv, 2 | (mic.MIC_HIP_PRED_GRAD if cs.pred else 0))
                                    for i, cs in enumerate(cases)])
    d_px = torch.from_numpy(np.concatenate([cs.img.ravel() for cs in cases]).view(np.int16)).cuda()
    sess = mic.Session(len(cases), max(cs.img.size for cs in cases))
    try:
        sess.encode_enqueue(d_px.data_ptr(), units)
        d_blobs, offs, st, _ = sess.encode_finish()
        host = _d2h(d_blobs, int(offs[-1]))
        for i, cs in enumerate(cases):
            rc, blob = mico.compress_single_frame_grad(cs.img, cs.maxv) if cs.pred else mico.compress_single_frame(cs.img, cs.maxv, 2)
            want = (mico.grad_delta_rle_compress if cs.pred else mico.delta_rle_compress)(cs.img, cs.maxv)
            ntok, status, tok, paths = _probe(mic, sess, i)
            _assert_tokens(cs.name, tok, want)
            assert st[i] == rc == status, (cs.name, st[i], rc, status)
            assert host[int(offs[i]):int(offs[i + 1])].tobytes() == blob, cs.name
            model, trace = S.model(cs)
            assert paths == model, (cs.name, paths, model, [(t[0], t[2], t[4]) for t in trace])
        # and back: the blobs decode to the pixels
        d_host = torch.from_numpy(np.concatenate([host, np.zeros(64, np.uint8)])).cuda()
        d_out = torch.zeros(int(px_off[-1]), dtype=torch.int16, device="cuda")
        sess.decode_enqueue(d_host.data_ptr(), offs, units, d_out.data_ptr())
        dst = sess.decode_finish()
        out = d_out.cpu().numpy().view(np.uint16)
        for i, cs in enumerate(cases):
            assert dst[i] == 0 and np.array_equal(out[px_off[i]:px_off[i + 1]].reshape(cs.img.shape), cs.img), cs.name
    finally:
        sess.close()


def test_a_symbol_unit_matches_the_oracle_token_by_token(mic, mico, gpu_ready):
    """a session WaveletV2 encode: the frame's one symbol unit spans four tiles, a zero run crosses a tile border, a run-free stretch
    follows.  The session keeps the unit's token slab after the finish, so the tokens themselves are compared."""
    torch = pytest.importorskip("torch")
    img = S.wavelet_frame()
    rows, cols = img.shape
    applied, want = W.encode_tokens(img, 5, mico.rle_compress)
    a, _ = W.forward(img, 5)
    sym = W.coeffs_to_u16(W.collect(a, applied)).astype(np.int64)
    model, trace = M.predict(sym, 1, sym.size, int(want[0]), src=1)
    rc, ref = mico.wavelet_v2_compress(img, 4095, 5)
    assert rc == 0
    d_px = torch.from_numpy(img.view(np.int16).copy()).cuda()
    sess = mic.Session(1, rows * cols)
    try:
        d_streams, offs, st, ap = sess.wavelet_v2_encode(d_px.data_ptr(), 1, rows, cols, 5)
        assert st[0] == 0 and ap == applied
        stream = _d2h(d_streams, int(offs[1])).tobytes()
        ntok, status, tok, paths = _probe(mic, sess, 0)
        _assert_tokens("wavelet", tok, want)
        assert status == 0 and paths == model, (paths, model, [(t[0], t[2], t[4]) for t in trace])
        assert ref.endswith(stream) and len(ref) - len(stream) == len(W.header(rows, cols, 4095, applied))
        d_s = torch.from_numpy(np.frombuffer(stream + bytes(64), np.uint8).copy()).cuda()
        d_out = torch.zeros(rows * cols, dtype=torch.int16, device="cuda")
        dst = sess.wavelet_v2_decode(d_s.data_ptr(), offs, 1, rows, cols, applied, d_out.data_ptr())
        assert dst[0] == 0 and np.array_equal(d_out.cpu().numpy().view(np.uint16).reshape(rows, cols), img)
    finally:
        sess.close()
