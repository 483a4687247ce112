"""The numpy restatement of WaveletV2 (tests/wavelet_ref.py) against the oracle, on the CPU: the transform, the oracle's token
stream and header byte for byte, RLE both ways, the crafted streams of tests/test_gpu_wavelet_seams.py (their decoder paths and
what the oracle makes of them), and the kernel constants walk_model restates."""
import os

import numpy as np
import pytest

import wavelet_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

DIMS = [1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 31, 101, 251]


def _shapes():
    """a covering design: every dimension value as rows and as cols, every level 0..8, paired so that each dimension meets
    small and large partners and several level counts"""
    out = []
    for k, d in enumerate(DIMS):
        out.append((d, DIMS[(k * 7 + 3) % len(DIMS)], k % 9))
        out.append((DIMS[(k * 5 + 1) % len(DIMS)], d, (k + 4) % 9))
    return out


@pytest.mark.parametrize("rows,cols,levels", _shapes())
def test_transform_matches_the_oracle(mico, rows, cols, levels):
    rng = np.random.default_rng(rows * 1000 + cols)
    px = rng.integers(0, 65536, (rows, cols)).astype(np.int32)
    px[: rows // 2] = rng.integers(0, 4096, (rows // 2, cols))
    a = px.copy()
    applied = mico.wt53_forward(a, levels) if levels else 0
    mine, mine_applied = W.forward(px, levels) if levels else (px.astype(np.int64), 0)
    assert mine_applied == applied
    assert np.array_equal(mine, a)
    back = W.inverse(a, applied)
    mico.wt53_inverse(a, applied)
    assert np.array_equal(back, a) and np.array_equal(back, px)
    # the inverse of ANY level count a header may carry (more than the dimensions allow, too) agrees
    for lv in (min(levels + 3, 8), 8):
        b = px.copy()
        mico.wt53_inverse(b, lv)
        assert np.array_equal(W.inverse(px, lv), b), lv


def _pin_images(synth):
    mr = np.fromfile(os.path.join(GOLDEN, "MR_256_256_image.bin"), dtype="<u2").reshape(256, 256)
    ct = np.fromfile(os.path.join(GOLDEN, "CT_512_512_image.bin"), dtype="<u2").reshape(512, 512)
    esc = synth.xr_like(cols=300, rows=200, depth=16, seed=4)                 # test_wavelet_v2_escape_path_full_16bit's frame
    esc[50:60, 100:140] = 65535
    esc[60:70, 100:140] = 0
    return [("MR", mr, int(mr.max()), 5), ("CT", ct, int(ct.max()), 5),
            ("XR12", synth.xr_like(cols=333, rows=271, depth=12, seed=21), 4095, 6),
            ("XR16", synth.xr_like(cols=257, rows=190, depth=16, seed=22, noise=40.0), 65535, 8),
            ("escape", esc, 65535, 5)]


def test_oracle_token_stream_and_header_are_pinned(mico, synth):
    """forward -> collect -> zigzag -> RLE of the restatement == the tokens inside the oracle's file; the 11 header bytes too.
    (The 4-state FSE stage around them is pinned to the reference's C codec elsewhere.)"""
    escapes = 0
    for name, img, mv, levels in _pin_images(synth):
        rc, f = mico.wavelet_v2_compress(img, mv, levels)
        assert rc == 0, name
        applied, tok = W.encode_tokens(img, levels, mico.rle_compress)
        rc, want = mico.fse_decompress_auto(f[11:], img.size * 8 + 64)
        assert rc == 0 and np.array_equal(tok, want), name
        assert f[:11] == W.header(img.shape[0], img.shape[1], mv, applied), name
        st, px = W.decode(img.shape[0], img.shape[1], applied, want)
        assert st == 0 and np.array_equal(px, img), name
        escapes += int(np.count_nonzero(W.coeffs_to_u16(W.collect(W.forward(img, levels)[0], applied)) == W.ESCAPE))
    assert escapes > 0                                                        # the escape path was part of it


def test_rle_builder_and_decoder_round_trip(mico, synth):
    rng = np.random.default_rng(7)
    for k in range(6):
        sym = rng.integers(0, 4096 if k % 2 else 300, 5000 + 977 * k).astype(np.uint16)
        sym[100:900] = 5
        sym[2000:2003] = 7
        mv = (1 << max(int(sym.max()).bit_length(), 4)) - 1
        tok = mico.rle_compress(sym, mv)
        st, back = W.rle_decode(tok)
        assert st == 0 and np.array_equal(back, sym)
        rc, back = mico.rle_decompress(tok, sym.size)
        assert rc == 0 and np.array_equal(back, sym)
    # the builder's structures, read by both decoders: runs of one, literal chunks of every length up to 65535 - midCount,
    # zero counts, another maxValue
    for mv in (4095, 15, 65535):
        tb = W.Tokens(mv)
        tb.runs(rng.integers(0, mv + 1, 300)).run(3, tb.mid).literal(rng.integers(0, mv + 1, 65535 - tb.mid))
        tb.literal([mv]).zero(rng.integers(0, mv + 1, 65536 - tb.mid)).run(mv, 1)
        tok = tb.build()
        st, mine = W.rle_decode(tok)
        rc, want = mico.rle_decompress(tok, tb.nsym)
        assert st == 0 and rc == 0 and mine.size == tb.nsym and np.array_equal(mine, want), mv
    # streams Go cannot read: both say so
    for tok in (tb.build(tb.nsym + 1), tb.build()[:-1], np.array([0, 0, 1, 1, 1], np.uint16), np.array([15, 0], np.uint16)):
        st, _ = W.rle_decode(tok)
        rc, _ = mico.rle_decompress(tok, tb.nsym + 1)
        assert st != 0 and rc != 0


def test_device_constants_have_not_drifted():
    """walk_model reads these from csrc/: a change there must be a change here, and in walk_model if the rule changed"""
    assert W.device_constants() == {"WP_PARTS": 64, "WP_MINLEN": 4096, "WP_EXTRA": 1024, "WS_T": 8192, "WS_ROWS": 64, "WS_LANES": 62,
                                    "ws_px": (2, 16), "tok_cap": (4, 16), "seg_cap": (2, 8), "sym_pad": 64, "sym_ceiling": (3, 8)}


def test_crafted_streams_take_the_paths_they_were_built_for(mico):
    """every case of tests/test_gpu_wavelet_seams.py takes its path in walk_model; together they take every path, and one needs
    three or more table rounds in k_wv_scatter.  The numpy decoder and the oracle make the same of each (pixels or the error)."""
    const = W.device_constants()
    paths, rounds = set(), 0
    for name, rows, cols, levels, tok, path, check in W.crafted_cases():
        info = W.walk_model(tok, rows * cols, const)
        assert info["path"] == path and check(info), (name, info)
        paths.add(info["path"])
        rounds = max(rounds, info["rounds"])
        rc, stream = mico.fse_compress(tok, 4)
        assert rc == 0, name
        f = W.header(rows, cols, 4095, levels) + stream
        rc_o, want = mico.wavelet_v2_decompress(f)
        st, mine = W.decode(rows, cols, levels, tok)
        assert st == rc_o, (name, st, rc_o)
        if st == 0:
            assert np.array_equal(mine, want), name
    assert paths == set(W.PATHS) and rounds >= 3


def test_walk_model_is_fast_on_two_million_tokens():
    """2 M tokens -- runs of one (a zero value every 25 lets the part walks join) and long literal chunks -- take the fast path,
    with every part entered and the table rounds counted, in well under a second"""
    import time
    rng = np.random.default_rng(3)
    tb = W.Tokens()
    for _ in range(100):
        v = rng.integers(1, 2048, 5000)
        v[::25] = 0
        tb.runs(v)
        tb.literal(rng.integers(0, 4096, 10000))
    tok = tb.build()
    assert tok.size > 2_000_000
    const = W.device_constants()
    t0 = time.perf_counter()
    info = W.walk_model(tok, tb.nsym, const)
    assert time.perf_counter() - t0 < 1.0
    assert info["path"] == "fast" and info["parts"] == 64 and info["rounds"] >= 2, info


def test_vectorised_walks_equal_the_serial_ones():
    """header_walk (pointer jumping) and walk_model's k_wv_expand window check against the plain serial loops they replace, on the
    crafted streams and on damaged copies of them"""
    def serial_heads(t, mid):
        pos, out = 3, []
        while pos < t.size:
            out.append(pos)
            v = int(t[pos])
            pos = pos + 1 + 65536 - mid if v == 0 else (pos + 2 if v <= mid else pos + 1 + v - mid)
        return np.array(out, dtype=np.int64)

    def serial_j63(t, mid, h, run, cap):                                  # k_wv_expand's window loop (csrc/mic_wavelet.hip)
        pos, out, k = 3, 0, 0
        while k < h.size and out < cap:
            if h[k] - pos == 63 and run[k]:
                return True
            if h[k] - pos >= 64:
                pos = int(h[k])
                continue
            v = int(t[h[k]])
            out += v if run[k] else (65536 - mid if v == 0 else v - mid)
            k += 1
        return False

    rng = np.random.default_rng(11)
    streams = [c[4] for c in W.crafted_cases()]
    for k in range(len(streams)):
        t = streams[k].astype(np.int64)
        i = rng.integers(3, t.size, 20)
        t[i] = rng.choice([0, 1, 2, 2047, 2048, 3000], 20)
        streams.append(t[: int(rng.integers(4, t.size + 1))] if k % 3 == 0 else t)
    j63 = 0
    for t in streams:
        t = np.asarray(t, dtype=np.int64)
        mid = W.mid_count(t[0])
        h, length, run = W.header_walk(t, mid)
        assert np.array_equal(h, serial_heads(t, mid))
        cap = (int(t[1]) << 16) + int(t[2])
        want = serial_j63(t, mid, h, run, cap)
        assert W._expand_j63(h, run, length, cap) == want
        j63 += want
    assert j63 >= 1
