"""WaveletV2 on the device at its seams (csrc/mic_wavelet.hip): the strip and wave tiling of k_wv_fwd2d / k_wv_inv2d, the 8-wide
subband scan of k_wv_symbols_par, the parallel RLE header walk (k_rle_walk_parts / _fix / _compact) and k_wv_scatter's table
rounds, the hand-over to k_wv_expand + k_wv_coeffs, and crafted headers.  Every result is the oracle's -- the same bytes, the same
pixels or the same error code -- and, where tests/wavelet_ref.py restates the case, the numpy reference's as well."""
import numpy as np
import pytest

import wavelet_ref as W

pytestmark = pytest.mark.gpu


def _dev_decode(mic, f):
    try:
        px, _, _ = mic.wavelet_v2_decompress(f)
        return 0, px
    except mic.MicError as e:
        return e.code, None


def _agree(mic, mico, f, name, ref=True):
    """device == oracle (and == the numpy reference) on file f; returns the status"""
    rc_o, want = mico.wavelet_v2_decompress(f)
    rc_g, got = _dev_decode(mic, f)
    assert rc_g == rc_o, (name, rc_g, rc_o)
    if rc_o == 0:
        assert np.array_equal(got, want), name
    if ref:
        rows, cols = int.from_bytes(f[0:4], "little"), int.from_bytes(f[4:8], "little")
        rc, tok = mico.fse_decompress_auto(f[11:], rows * cols * 8 + 64)
        st, mine = W.decode(rows, cols, f[10], tok if rc == 0 else None)
        assert st == rc_o, (name, st, rc_o)
        if st == 0:
            assert np.array_equal(mine, want), name
    return rc_o


def _image(rows, cols, depth, seed):
    """a ramp with a little noise: few distinct symbols, so that the 4-state FSE stage takes even small and thin frames"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    px = (y * 7 + x * 3) % 97 + rng.integers(0, 3, (rows, cols))
    if depth == 16:
        px = px * 613 + rng.integers(0, 2, (rows, cols))
    return px.astype(np.uint16)


# ---- 1. tiling: a level's (c + 1) / 2 at a wave's 62 written pairs, a block's 4 waves; (r + 1) / 2 at a 64-row strip ---------
# cols 122 / 124 / 125 -> 61 / 62 / 63 pairs; 246 / 248 / 249 -> 123 / 124 / 125; 494 / 496 / 497 -> 247 / 248 / 249 (a block
# writes 248); 990 -> 495 -> 248 at level 2; 1985 -> 993 -> 497 -> 249 at level 3.  rows 125 / 128 / 129 -> 63 / 64 / 65;
# 254 / 256 / 257 -> 127 / 128 / 129; 515 -> 258 -> 129 at level 2.  Odd widths read unaligned pixel pairs.
TILING = [(125, 122, 1, 12), (128, 124, 2, 12), (129, 125, 3, 12), (254, 246, 4, 16), (256, 248, 5, 12), (257, 249, 6, 16),
          (515, 494, 7, 12), (129, 496, 8, 16), (254, 497, 1, 16), (125, 990, 2, 12), (257, 1985, 3, 16), (515, 990, 8, 16),
          (1, 700, 5, 12), (700, 1, 5, 12), (2, 333, 4, 12), (3, 3, 8, 16), (2, 2, 1, 12), (64, 1985, 6, 12)]


@pytest.mark.parametrize("rows,cols,levels,depth", TILING)
def test_tiling_sweep_matches_the_oracle_and_the_reference(mic, mico, gpu_ready, rows, cols, levels, depth):
    img = _image(rows, cols, depth, rows * 3 + cols)
    mv = (1 << depth) - 1
    rc, want = mico.wavelet_v2_compress(img, mv, levels)
    if rc != 0:                                                               # 3 x 3: the FSE stage refuses nine symbols
        with pytest.raises(mic.MicError) as e:
            mic.wavelet_v2_compress(img, rows, cols, mv, levels)
        assert e.value.code == rc and (rows, cols) == (3, 3)
        return
    applied, tok = W.encode_tokens(img, levels, mico.rle_compress)
    assert want[:11] == W.header(rows, cols, mv, applied)
    assert np.array_equal(mico.fse_decompress_auto(want[11:], img.size * 8 + 64)[1], tok)
    got = mic.wavelet_v2_compress(img, rows, cols, mv, levels)
    assert got == want
    px, r, c = mic.wavelet_v2_decompress(want)
    assert (r, c) == (rows, cols) and np.array_equal(px, img)


def test_tiling_sweep_in_batches(mic, mico, gpu_ready):
    for rows, cols, levels, depth in ((257, 249, 6, 16), (129, 496, 8, 12), (125, 990, 2, 12)):
        frames = np.stack([_image(rows, cols, depth, 100 + k) for k in range(3)])
        mv = (1 << depth) - 1
        res = mic.wavelet_v2_compress_batch(frames, mv, levels)
        wants = [mico.wavelet_v2_compress(f, mv, levels)[1] for f in frames]
        assert [st for st, _ in res] == [0] * 3 and [b for _, b in res] == wants
        sts, back = mic.wavelet_v2_decompress_batch(wants)
        assert sts == [0] * 3 and np.array_equal(back, frames)


# ---- 2. the subband scan: n around multiples of WS_T = 8192 (8191, 8193, 16383, 16385, 24575, 24577), n mod 8 = 1, 3, 5, 7 ------
# ---- (the tiling shapes above add 0, 2, 4, 6), 8 levels: the coarsest subband rows are shorter than 8 --------------------------
SCAN = [(1, 8191), (8191, 1), (3, 2731), (129, 127), (145, 113), (25, 983), (7, 3511), (101, 103), (33, 35), (61, 67), (21, 29),
        (17, 47), (13, 43), (13, 41), (5, 9), (255, 257)]


@pytest.mark.parametrize("rows,cols", SCAN)
def test_symbol_scan_at_group_and_row_edges(mic, mico, gpu_ready, rows, cols):
    img = _image(rows, cols, 12, rows * cols)
    rc, want = mico.wavelet_v2_compress(img, 4095, 8)
    assert rc == 0
    assert mic.wavelet_v2_compress(img, rows, cols, 4095, 8) == want
    _agree(mic, mico, want, (rows, cols))


def test_one_wide_coefficient_in_a_batch(mic, mico, gpu_ready):
    """a frame with exactly one coefficient outside +-32767 (k_wv_symbols) next to frames with none (k_wv_symbols_par)"""
    rows, cols = 160, 210
    frames = np.stack([_image(rows, cols, 12, 40 + k) for k in range(4)])
    frames[2] //= 16
    frames[2, 81, 101] = 65535                                                # one HH coefficient of level 1 at (odd, odd)
    wide = [int(np.count_nonzero(np.abs(W.forward(f, 3)[0]) > 32767)) for f in frames]
    assert wide == [0, 0, 1, 0]
    res = mic.wavelet_v2_compress_batch(frames, 65535, 3)
    wants = [mico.wavelet_v2_compress(f, 65535, 3)[1] for f in frames]
    assert [st for st, _ in res] == [0] * 4 and [b for _, b in res] == wants
    sts, back = mic.wavelet_v2_decompress_batch(wants)
    assert sts == [0] * 4 and np.array_equal(back, frames)


# ---- 3. crafted token streams (tests/wavelet_ref.py: crafted_cases; their paths are checked on the CPU as well) --------------
def _crafted_files(mico):
    out = []
    for name, rows, cols, levels, tok, path, check in W.crafted_cases():
        rc, stream = mico.fse_compress(tok, 4)
        assert rc == 0, name
        out.append((name, rows, cols, levels, tok, path, check, W.header(rows, cols, 4095, levels) + stream))
    return out


def test_crafted_streams_agree_with_the_oracle_and_the_reference(mic, mico, gpu_ready):
    const = W.device_constants()
    paths, rounds, statuses = set(), 0, set()
    for name, rows, cols, levels, tok, path, check, f in _crafted_files(mico):
        info = W.walk_model(tok, rows * cols, const)
        assert info["path"] == path and check(info), (name, info)
        paths.add(path)
        rounds = max(rounds, info["rounds"])
        statuses.add(_agree(mic, mico, f, name))
    assert paths == set(W.PATHS) and rounds >= 3 and statuses == {0, W.CORRUPT}


# ---- 4. header mutations of valid payloads -----------------------------------------------------------------------------------
def test_header_mutations(mic, mico, gpu_ready):
    """levels 0..8 on any payload (more than the dimensions allow included), rows / cols swapped or refactored to the same product.
    Levels 9 and 255 are MIC_ERR_CORRUPT on both sides: a deliberate departure from Go, which would run an inverse of that many
    levels (waveletfsecompressu16.go:403-413; DESIGN.md section 4, WaveletV2)."""
    for rows, cols, levels in ((40, 30, 3), (6, 10, 2), (120, 90, 5)):
        img = _image(rows, cols, 12, rows + cols)
        rc, good = mico.wavelet_v2_compress(img, 4095, levels)
        assert rc == 0
        body = good[11:]
        for lv in range(0, 9):
            _agree(mic, mico, good[:10] + bytes([lv]) + body, (rows, cols, lv))
        for lv in (9, 255):
            f = good[:10] + bytes([lv]) + body
            assert _agree(mic, mico, f, (rows, cols, lv)) == W.CORRUPT
        for r2, c2 in ((cols, rows), (rows * 2, cols // 2), (rows // 2, cols * 2), (1, rows * cols), (rows * cols, 1)):
            for lv in (levels, 8):
                _agree(mic, mico, W.header(r2, c2, 4095, lv) + body, (r2, c2, lv))


# ---- 5. fast-path and slow-path frames in one batch, and through a session ----------------------------------------------------
def test_mixed_batch_and_session(mic, mico, gpu_ready):
    torch = pytest.importorskip("torch")
    by_shape = {}
    for name, rows, cols, levels, tok, path, check, f in _crafted_files(mico):
        by_shape.setdefault((rows, cols, levels), []).append((name, path, f))
    groups = [g for g in by_shape.values() if len({p for _, p, _ in g}) > 1]
    assert groups
    for g in groups:
        files = [f for _, _, f in g]
        sts, back = mic.wavelet_v2_decompress_batch(files)
        for k, (name, path, f) in enumerate(g):
            rc_o, want = mico.wavelet_v2_decompress(f)
            assert sts[k] == rc_o, (name, sts[k], rc_o)
            if rc_o == 0:
                assert np.array_equal(back[k], want), name
    # one mixed set through Session.wavelet_v2_decode: header-less streams back to back on the device
    g = max(groups, key=len)
    rows, cols = int.from_bytes(g[0][2][0:4], "little"), int.from_bytes(g[0][2][4:8], "little")
    levels = g[0][2][10]
    streams = [f[11:] for _, _, f in g]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.uint64)
    packed = torch.from_numpy(np.frombuffer(b"".join(streams), dtype=np.uint8).copy()).cuda()
    d_out = torch.zeros((len(g), rows, cols), dtype=torch.int16, device="cuda")
    sess = mic.Session(len(g), 2 * rows * cols + 16)
    try:
        st = sess.wavelet_v2_decode(packed.data_ptr(), offs, len(g), rows, cols, levels, d_out.data_ptr())
        out = d_out.cpu().numpy().view(np.uint16)
        for k, (name, path, f) in enumerate(g):
            rc_o, want = mico.wavelet_v2_decompress(f)
            assert st[k] == rc_o, (name, st[k], rc_o)
            if rc_o == 0:
                assert np.array_equal(out[k], want), name
    finally:
        sess.close()
