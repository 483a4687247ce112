"""The inverse gradient-adaptive predictor (k_dec_predict_grad, csrc/mic_decode_px.hip) against the oracle's serial decoder
(deltagradrlecompressu16.go:71-133) at the seams the kernel has: 64-row bands, four-pixel groups and the right edge, the 8-byte
symbol loads and their tail, the two flag words of a group, the row-buffer classes by width, 16-bit wrap-around -- and behind the
last class, frames wider than the LDS row buffer holds.  The cases come from tests/grad_predict_frames.py; tests/test_grad_predict_cpu.py
shows that each reaches its seam and pins the oracle's decoder itself.  Every comparison is array_equal or byte equality."""
import numpy as np
import pytest

import grad_predict_frames as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tuple(F.FAMILIES))
def test_every_frame_both_directions_against_the_oracle(mic, mico, synth, gpu_ready, name):
    cases, streams = F.family(synth, name), F.oracle_streams(mico, synth, name)
    for cs, want in zip(cases, streams):
        h, w = cs.img.shape
        assert want, cs.name
        assert mic.compress_single_frame_grad(cs.img, w, h, cs.maxv) == want, cs.name
        got = mic.decompress_single_frame_grad(want, w, h)
        assert np.array_equal(got, cs.img), (cs.name, np.argwhere(got != cs.img)[:4].tolist())


def _device_decodes(mic, streams):
    out = []
    for s in streams:
        try:
            out.append((0, mic.decompress_single_frame_grad(s.stream, s.w, s.h)))
        except mic.MicError as e:
            out.append((e.code, None))
    return out


def _agree(streams, oracle, device):
    for s, (rc_o, want), (rc_g, got) in zip(streams, oracle, device):
        assert (rc_g == 0) == (rc_o == 0), (s.name, rc_g, rc_o)
        if rc_o == 0:
            assert np.array_equal(got, want), (s.name, int(np.count_nonzero(got != want)), np.argwhere(got != want)[:4].tolist())


def test_wrapping_streams_agree_with_the_oracle(mic, mico, synth, gpu_ready):
    """Symbols no encoder writes: pred + sym - thr leaves 0 .. 65535, is cut to 16 bits as the reference's uint16() does, and the
    wrapped pixel is W / N / NW / NE of what follows.  The floors are recounted on the device's own results."""
    streams = F.wrapping_streams(mico, synth)
    device = _device_decodes(mic, streams)
    _agree(streams, F.oracle_decodes(mico, synth, "wrapping"), device)
    counts = F.stream_counts(streams, device)
    assert all(counts[k] >= v for k, v in F.WRAP_FLOORS.items()), counts


def test_damaged_streams_agree_with_the_oracle(mic, mico, synth, gpu_ready):
    """Zero counts, headers past the end, streams that stop early: refused where the oracle refuses, its pixels elsewhere."""
    streams = F.damaged_streams(mico, synth)
    device = _device_decodes(mic, streams)
    _agree(streams, F.oracle_decodes(mico, synth, "damaged"), device)
    counts = F.stream_counts(streams, device)
    assert all(counts[k] >= v for k, v in F.DAMAGE_FLOORS.items()), counts


# ---- sessions: the class launch follows the batch's widths ---------------------------------------------------------------------
def _session_decode(mic, torch, sess, items):
    """items: [(stream, image, gradient?)] -> every unit must come back.  The streams are uploaded back to back (64 bytes of slack
    behind the last: the decode kernels may read that far past a stream's end)."""
    blob = b"".join(s for s, _, _ in items)
    offs = np.cumsum([0] + [len(s) for s, _, _ in items]).astype(np.uint64)
    px = np.cumsum([0] + [img.size for _, img, _ in items])
    d_blobs = torch.from_numpy(np.frombuffer(blob + bytes(64), np.uint8).copy()).cuda()
    d_out = torch.full((int(px[-1]),), 0x5A5A, dtype=torch.int16, device="cuda")
    units = mic.Session.make_units([(int(px[k]), img.shape[1], img.shape[0], 4095, 2 | (mic.MIC_HIP_PRED_GRAD if g else 0))
                                    for k, (_, img, g) in enumerate(items)])
    sess.decode_enqueue(d_blobs.data_ptr(), offs, units, d_out.data_ptr())
    st = sess.decode_finish()
    back = d_out.cpu().numpy().view(np.uint16)
    for k, (_, img, g) in enumerate(items):
        got = back[int(px[k]): int(px[k + 1])].reshape(img.shape)
        assert st[k] == 0 and np.array_equal(got, img), (k, img.shape, g, int(st[k]), np.argwhere(got != img)[:4].tolist())


def _pair(mico, img):
    """the frame as a gradient unit and as an avg unit"""
    rc_g, g = mico.compress_single_frame_grad(img, 4095)
    rc_a, a = mico.compress_single_frame(img, 4095, 2)
    assert rc_g == 0 and rc_a == 0
    return [(g, img, True), (a, img, False)]


def _narrow_batch(mico, synth):
    return _pair(mico, synth.xr_like(cols=333, rows=100, depth=12, seed=21))


def _class_frame(synth, w):
    (cs,) = [c for c in F.family(synth, "class") if c.img.shape == (65, w)]
    return cs.img


def test_one_batch_with_both_predictors_at_every_class_seam(mic, mico, synth, gpu_ready):
    torch = pytest.importorskip("torch")
    items = [it for w in (4088, 4089, 8184, 8185) for it in _pair(mico, _class_frame(synth, w))] + _narrow_batch(mico, synth)
    sess = mic.Session(len(items), 8185 * 65)
    try:
        _session_decode(mic, torch, sess, items)
        _session_decode(mic, torch, sess, items[::-1])
    finally:
        sess.close()


@pytest.mark.parametrize("w", [8129, 8184, 4089, 4088, 300])
def test_a_single_gradient_unit_launches_the_class_of_its_width(mic, mico, synth, gpu_ready, w):
    """8129 .. 8184 columns are MIC_PRED_WIDE for mic_pred_bit and the SECOND row-buffer class of the gradient kernel; a class that
    is not launched leaves symbols in the output.  Through a fresh session, and through one that has seen 333-wide batches only."""
    torch = pytest.importorskip("torch")
    img = _class_frame(synth, w) if w in F.CLASS_WIDTHS else F.seam_case("single", F.ramp(synth, w, 65), 4095, 1).img
    unit = _pair(mico, img)[:1]
    for seasoned in (False, True):
        sess = mic.Session(2, 8185 * 65)
        try:
            if seasoned:
                for _ in range(2):
                    _session_decode(mic, torch, sess, _narrow_batch(mico, synth))
            _session_decode(mic, torch, sess, unit)
        finally:
            sess.close()


# ---- PICA ---------------------------------------------------------------------------------------------------------------------
def test_pica_files_of_gradient_strips_and_of_avg_strips(mic, mico, synth, gpu_ready):
    images = F.pica_images(synth)
    files = []
    for name, img, strips, kind in images:
        rc, blob = mico.pica_compress(img, 4095, strips)
        assert rc == 0 and F.pica_flags(blob) == [1 if kind == "grad" else 0] * strips, name   # from the 16-byte entries
        files.append(blob)
        assert np.array_equal(mic.decompress_parallel_strips_adaptive(blob), img), name
        h, w = img.shape
        assert mic.compress_parallel_strips_adaptive(img, w, h, 4095, strips) == blob, name
    # all-gradient and all-avg files side by side in one batch call
    res = mic.decompress_parallel_strips_adaptive_batch(files, [(img.shape[1], img.shape[0]) for _, img, _, _ in images])
    for (name, img, _, _), (st, back) in zip(images, res):
        assert st == 0 and np.array_equal(back, img), name


# ---- the width limit ----------------------------------------------------------------------------------------------------------------
def test_the_widest_frame_of_the_lds_row_buffer(mic, mico, synth, gpu_ready):
    for cs, want in zip(F.family(synth, "class"), F.oracle_streams(mico, synth, "class")):
        if cs.img.shape[1] == F.WIDEST and cs.img.shape[0] in (2, 65):
            h, w = cs.img.shape
            assert mic.compress_single_frame_grad(cs.img, w, h, 4095) == want
            assert np.array_equal(mic.decompress_single_frame_grad(want, w, h), cs.img)


def test_frames_wider_than_the_lds_row_buffer(mic, mico, synth, gpu_ready):
    """The reference has no width limit, and neither has the encoder here.  One column past the widest LDS row buffer the decoder
    takes the previous band's last row from the frame itself (it is in px_out by then): the oracle's stream gives the oracle's
    pixels, the project reads every file it writes, and both stay byte for byte the oracle's."""
    w = F.WIDEST + 1
    for h in (2, 65, 130):
        img = F.seam_case("wider", F.ramp(synth, w, h), 4095, h % 4).img if h < 130 else F.wave_image(synth, w, h, "grad")
        rc, want = mico.compress_single_frame_grad(img, 4095)
        assert rc == 0
        mine = mic.compress_single_frame_grad(img, w, h, 4095)
        assert mine == want, h
        assert np.array_equal(mic.decompress_single_frame_grad(mine, w, h), img), h
    rc, want = mico.pica_compress(img, 4095, 2)
    assert rc == 0 and F.pica_flags(want) == [1, 1]
    mine = mic.compress_parallel_strips_adaptive(img, w, 130, 4095, 2)
    assert mine == want
    assert np.array_equal(mic.decompress_parallel_strips_adaptive(mine), img)
    res = mic.decompress_parallel_strips_adaptive_batch([want], [(w, 130)])
    assert res[0][0] == 0 and np.array_equal(res[0][1], img)
