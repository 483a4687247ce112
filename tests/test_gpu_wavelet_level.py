"""WaveletV2 at reduced resolution on the device (csrc/mic_wavelet.hip: wv_decode_level_frames).  The image at level r is the
nr[r] x nc[r] LL band the forward transform holds after r levels, saturated to u16; every expected value here comes from the numpy
restatement of the reference (tests/wavelet_ref.py), never from the device.  The tANS chain stops at wv_level_sym_limit's ceiling
(P + P/4 + 512 symbols, P = nr[r] * nc[r], rounded up to 128) and a frame that ceiling does not cover is decoded again whole: the
symbol counts the entry points report show both."""
import ctypes

import numpy as np
import pytest

import wavelet_ref as W

from test_gpu_wavelet_seams import TILING, _image

pytestmark = pytest.mark.gpu


def _dims(rows, cols, levels):
    nr, nc = [rows], [cols]
    for _ in range(levels):
        nr.append((nr[-1] + 1) // 2)
        nc.append((nc[-1] + 1) // 2)
    return nr, nc


def _bands(px, levels):
    """band r = forward(px, r)'s LL, saturated: one level at a time on the LL of the level before (forward's own loop)"""
    out, ll = [px.astype(np.uint16)], px.astype(np.int64)
    for _ in range(levels):
        a, _ = W.forward(ll, 1)
        ll = a[:(ll.shape[0] + 1) // 2, :(ll.shape[1] + 1) // 2]
        out.append(np.clip(ll, 0, 65535).astype(np.uint16))
    return out


def _ceiling(P):
    """wv_level_sym_limit (csrc/mic_wavelet.hip): the symbols pass 1 decodes"""
    return (P + P // 4 + 512 + 127) // 128 * 128


def _count(f):
    """the stream's tANS symbol count: the FSE prefix behind the 11-byte header (0xFF 0x04, then u32)"""
    return int.from_bytes(f[13:17], "little")


def _escape_frame(rows=512, cols=512, seed=7):
    """16-bit, LL mean above 32767: every LL coefficient is a three-word escape, so P words never cover P coefficients"""
    rng = np.random.default_rng(seed)
    return (40000 + rng.integers(0, 64, (rows, cols))).astype(np.uint16)


def _plain_frame(rows=512, cols=512, seed=8):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return ((y * 5 + x * 3) % 1500 + 1000 + rng.integers(0, 64, (rows, cols))).astype(np.uint16)


def _check_all_levels(mic, px, f, name):
    rows, cols = px.shape
    levels = f[10]
    bands = _bands(px, levels)
    full, _, _ = mic.wavelet_v2_decompress(f)
    for r in range(levels + 1):
        got = mic.wavelet_v2_decompress_level(f, r)
        assert got.shape == bands[r].shape, (name, r)
        assert np.array_equal(got, bands[r]), (name, r)
        if r == 0:
            assert got.tobytes() == full.tobytes(), name
    return bands


# ---- 1. every level equals the numpy band --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,levels,depth", TILING)
def test_tiling_shapes_at_every_level(mic, gpu_ready, rows, cols, levels, depth):
    img = _image(rows, cols, depth, rows * 3 + cols)
    try:
        f = mic.wavelet_v2_compress(img, rows, cols, (1 << depth) - 1, levels)
    except mic.MicError:                                                      # 3 x 3: the FSE stage refuses nine symbols
        assert (rows, cols) == (3, 3)
        return
    bands = _check_all_levels(mic, img, f, (rows, cols, levels))
    if rows * cols < 300_000:                                                  # the band helper is forward(px, r)'s LL
        for r in range(1, f[10] + 1):
            a, ap = W.forward(img, r)
            assert ap == r and np.array_equal(np.clip(a[:bands[r].shape[0], :bands[r].shape[1]], 0, 65535), bands[r])


def test_cr_like_and_16_bit_frames_at_every_level(mic, synth, gpu_ready):
    cr = synth.cr_like()
    f = mic.wavelet_v2_compress(cr, cr.shape[0], cr.shape[1], 4095, 8)
    assert f[10] == 8
    _check_all_levels(mic, cr, f, "cr_like")
    px16 = synth.cr_like(cols=640, rows=512, depth=16, seed=5)
    f16 = mic.wavelet_v2_compress(px16, 512, 640, 65535, 6)
    _check_all_levels(mic, px16, f16, "16-bit")
    esc = _escape_frame()
    fe = mic.wavelet_v2_compress(esc, 512, 512, 65535, 2)
    b = _check_all_levels(mic, esc, fe, "escape")
    assert b[2].min() > 32767                                                  # (the case the second pass is for)


# ---- 2. the chain stops early --------------------------------------------------------------------------------------------------
def test_the_chain_stops_early(mic, synth, gpu_ready):
    cr = synth.cr_like()
    rows, cols = cr.shape
    f = mic.wavelet_v2_compress(cr, rows, cols, 4095, 8)
    count, levels = _count(f), f[10]
    nr, nc = _dims(rows, cols, levels)
    syms = []
    for r in range(levels + 1):
        st, out, s = mic.wavelet_v2_decompress_level_batch([f], r, counts=True)
        assert st == [0]
        syms.append(int(s[0]))
    assert syms[0] == count
    for r in range(1, levels + 1):
        assert syms[r] == min(count, _ceiling(nr[r] * nc[r])), (r, syms[r])  # one pass, stopped at the ceiling
        assert syms[r] <= syms[r - 1]
    assert syms[levels] < 0.05 * count, (syms[levels], count)


# ---- 3. the second pass ----------------------------------------------------------------------------------------------------------
def test_escape_heavy_frames_take_a_second_pass_alone(mic, gpu_ready):
    esc = [_escape_frame(seed=s) for s in (7, 9)]
    plain = [_plain_frame(seed=s) for s in (8, 10)]
    imgs = [esc[0], plain[0], esc[1], plain[1]]
    files = [mic.wavelet_v2_compress(im, 512, 512, 65535, 2) for im in imgs]
    assert all(f[10] == 2 for f in files)
    bands = [_bands(im, 2) for im in imgs]
    nr, nc = _dims(512, 512, 2)
    for r in range(3):
        st, out, syms = mic.wavelet_v2_decompress_level_batch(files, r, counts=True)
        assert st == [0] * 4, r
        for i in range(4):
            assert np.array_equal(out[i], bands[i][r]), (r, i)
            count = _count(files[i])
            if r == 0:
                assert syms[i] == count
            elif i % 2 == 0:                                                   # pass 1 fell short: the ceiling, then the whole stream
                assert _ceiling(nr[r] * nc[r]) < count and syms[i] == _ceiling(nr[r] * nc[r]) + count, (r, i, int(syms[i]), count)
            else:                                                              # plain frames stay single-pass
                assert syms[i] == min(count, _ceiling(nr[r] * nc[r])), (r, i, int(syms[i]), count)


# ---- 4. batch semantics -------------------------------------------------------------------------------------------------------
def test_batch_statuses_follow_decompress_batch(mic, gpu_ready):
    imgs = [_plain_frame(256, 320, seed=s) for s in range(3)]
    good = [mic.wavelet_v2_compress(im, 256, 320, 4095, 4) for im in imgs]
    other = mic.wavelet_v2_compress(_plain_frame(256, 256, seed=3), 256, 256, 4095, 4)
    bad_fse = bytearray(good[1]); bad_fse[11] = 0
    files = [good[0], b"\x01\x02\x03", other, bytes(bad_fse), good[2]]
    st_full, _ = mic.wavelet_v2_decompress_batch(files)
    assert st_full == [0, mic.MIC_ERR_CORRUPT, mic.MIC_ERR_ARGS, mic.MIC_ERR_CORRUPT, 0]
    for r in (0, 2, 4):
        st, out = mic.wavelet_v2_decompress_level_batch(files, r)
        assert st == st_full, r
        assert np.array_equal(out[0], _bands(imgs[0], r)[r]) and np.array_equal(out[4], _bands(imgs[2], r)[r]), r
    with pytest.raises(mic.MicError) as e:
        mic.wavelet_v2_decompress_level(good[0], 5)
    assert e.value.code == mic.MIC_ERR_ARGS


def test_capacity_is_checked_against_the_reduced_size(mic, gpu_ready):
    im = _plain_frame(256, 320, seed=4)
    f = np.frombuffer(mic.wavelet_v2_compress(im, 256, 320, 4095, 4), dtype=np.uint8)
    L = mic.lib()
    want = _bands(im, 2)[2]
    out = np.zeros(want.size, dtype=np.uint16)
    assert L.mic_hip_wavelet_v2_decompress_level(f.ctypes.data, f.size, 2, out.ctypes.data, want.size - 1) == mic.MIC_ERR_CAPACITY
    assert L.mic_hip_wavelet_v2_decompress_level(f.ctypes.data, f.size, 2, out.ctypes.data, want.size) == 0
    assert np.array_equal(out.reshape(want.shape), want)
    ptrs = (ctypes.c_void_p * 2)(f.ctypes.data, f.ctypes.data); lens = (ctypes.c_size_t * 2)(f.size, f.size); st = (ctypes.c_int32 * 2)()
    out2 = np.zeros(2 * want.size, dtype=np.uint16)
    assert L.mic_hip_wavelet_v2_decompress_level_batch(ptrs, lens, 2, 2, out2.ctypes.data, 2 * want.size - 1, st, None) == mic.MIC_ERR_CAPACITY
    assert L.mic_hip_wavelet_v2_decompress_level_batch(ptrs, lens, 2, 2, out2.ctypes.data, 2 * want.size, st, None) == 0
    assert list(st) == [0, 0] and np.array_equal(out2.reshape(2, *want.shape)[1], want)


# ---- 5. the session form ----------------------------------------------------------------------------------------------------------
def test_session_decode_level_on_device_resident_streams(mic, synth, gpu_ready):
    torch = pytest.importorskip("torch")
    rows, cols = 1024, 768
    frames = np.stack([synth.cr_like(cols=cols, rows=rows, seed=40 + i) for i in range(2)] + [_escape_frame(rows, cols, seed=11)])
    d_px = torch.from_numpy(frames.view(np.int16).copy()).cuda()
    sess = mic.Session(3, rows * cols + 16, device=0)
    d_streams, offs, st, applied = sess.wavelet_v2_encode(d_px.data_ptr(), 3, rows, cols, 5)
    assert (st == 0).all() and applied == 5
    packed = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda")
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(packed.data_ptr()), ctypes.c_void_p(d_streams), ctypes.c_size_t(int(offs[-1])), 3) == 0
    bands = [_bands(frames[i], applied) for i in range(3)]
    nr, nc = _dims(rows, cols, applied)
    for r in range(applied + 1):
        d_out = torch.zeros((3, nr[r], nc[r]), dtype=torch.int16, device="cuda")
        st, syms = sess.wavelet_v2_decode_level(packed.data_ptr(), offs, 3, rows, cols, applied, r, d_out.data_ptr())
        assert (st == 0).all(), r
        got = d_out.cpu().numpy().view(np.uint16)
        for i in range(3):
            assert np.array_equal(got[i], bands[i][r]), (r, i)
        if r == applied:                                                       # the escape frame: the ceiling, then the whole stream
            assert syms[0] == syms[1] == _ceiling(nr[r] * nc[r]) and syms[2] > syms[0] + 3 * nr[r] * nc[r], (r, syms)
    sess.close()


# ---- 6. several devices -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def device_lists(mic, gpu_ready):
    yield ([0], [0, 0], [0, 0, 0])
    mic.set_devices([0])


def test_level_batches_over_device_lists(mic, synth, device_lists):
    imgs = [synth.cr_like(cols=400, rows=300, seed=60 + i) for i in range(4)] + [_escape_frame(300, 400, seed=12)]
    files = [mic.wavelet_v2_compress(im, 300, 400, 65535, 4) for im in imgs]
    want = {}
    for devs in device_lists:
        mic.set_devices(devs)
        assert mic.get_devices() == devs
        for r in (1, 3):
            st, out, syms = mic.wavelet_v2_decompress_level_batch(files, r, counts=True)
            assert st == [0] * 5, (devs, r)
            for i, im in enumerate(imgs):
                assert np.array_equal(out[i], _bands(im, r)[r]), (devs, r, i)
            if r in want:
                assert np.array_equal(out, want[r][0]) and np.array_equal(syms, want[r][1]), (devs, r)
            else:
                want[r] = (out, syms)
