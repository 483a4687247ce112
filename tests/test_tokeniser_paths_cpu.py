"""What can be said without a device about the cases of tests/test_gpu_tokeniser_paths.py: every frame has the symbol stream it was
built for (by the oracle's own predictor), passes the oracle's round trip, is compressible for the oracle (the GPU test compares
blobs), and under the model of tests/tokeniser_paths.py takes the route it is named for -- a case cannot silently stop aiming at
its seam.  The model's constants are compared with the kernel's source."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tokeniser_paths as M
import tokeniser_streams as S
import wavelet_ref as W

GROUPS = tuple(S.GROUPS)


def _oracle_tokens(mico, case):
    return (mico.grad_delta_rle_compress if case.pred else mico.delta_rle_compress)(case.img, case.maxv)


def _oracle_decode_tokens(mico, tok, w, h, pred):
    if pred:
        return mico.grad_delta_rle_decompress(tok, w, h)
    tok = np.ascontiguousarray(tok, np.uint16)
    out = np.empty((h, w), np.uint16)
    rc = mico.lib().mico_delta_rle_decompress(C.c_void_p(tok.ctypes.data), C.c_size_t(tok.size), w, h, C.c_void_p(out.ctypes.data))
    return rc, out


def _same_runs(x):
    """(start, length) of the maximal runs of three and more"""
    first = np.ones(x.size, bool); first[1:] = x[1:] != x[:-1]
    st = np.flatnonzero(first)
    ln = np.diff(np.append(st, x.size))
    return [(int(a), int(b)) for a, b in zip(st, ln) if b >= 3]


def _check_aim(case, k, trace):
    x, aim = case.sym, case.aim
    c = M.mid_count(case.maxv, 0) - 3
    runs = _same_runs(x)
    if aim[0] == "chunk-opens":                                             # the symbol at (tile, thread, position) is a multiple of c into its stretch
        _, tile, th, bq = aim
        i = tile * M.TILE + th * 8 + bq - 2
        start = max(a + b for a, b in runs if a + b <= i)
        assert (i - start) % c == 0 and i > start and not any(a <= i + 8 and a + b > i - 8 for a, b in runs), (case.name, i, start)
        assert trace[tile][4] == "fast" and trace[tile][1] - 3 <= i < trace[tile][1] - 3 + M.TILE
        if bq == 0:                                                         # the thread before closes a chunk on its last position
            assert th > 0 or trace[tile - 1][4] in ("fast", "general")
    elif aim[0] == "last-stretch":
        a, b = runs[-1]
        assert x.size - (a + b) == aim[1], (case.name, x.size - a - b)
    elif aim[0] == "last-run":
        n = aim[1]
        assert (x[-n:] == x[-1]).all() and x[-n - 1] != x[-1], case.name
    elif aim[0] == "wraps-at":                                              # global window position of the run's (c + 3)-th symbol
        _, pos, length, cc = aim
        assert cc == c and length > 2 * c + 3
        a, b = max(runs, key=lambda r: r[1])
        assert b == length and a + 2 + c + 2 == pos, (case.name, a, b, pos)


@pytest.mark.parametrize("group", GROUPS)
def test_every_case_reaches_its_seam_under_the_model(mico, group):
    cases = S.group(group)
    assert len({cs.name for cs in cases}) == len(cases)
    for cs in cases:
        h, w = cs.img.shape
        tok = _oracle_tokens(mico, cs)
        mid = M.mid_count(cs.maxv, 0)
        assert tok[0] == (1 << int(cs.maxv).bit_length()) - 1
        # the stream the case was built for is the one the oracle's predictor sees, and the one its tokens stand for
        if not cs.pred:
            assert np.array_equal(mico.delta_symbols(cs.img, cs.maxv), cs.sym), cs.name
        assert np.array_equal(M.rle_expand(tok[1:], mid), cs.sym), cs.name
        rc, back = _oracle_decode_tokens(mico, tok, w, h, cs.pred)
        assert rc == 0 and np.array_equal(back, cs.img), cs.name
        # compressible: the GPU test checks the fused histogram through the blob
        rc, blob = mico.compress_single_frame_grad(cs.img, cs.maxv) if cs.pred else mico.compress_single_frame(cs.img, cs.maxv, 2)
        assert rc == 0 and len(blob) > 6, (cs.name, rc)
        k, trace = S.model(cs)
        assert cs.expect(k, trace), (cs.name, k, [(t[0], t[2], t[4]) for t in trace])
        assert k["fast"] + k["general"] == len(trace) and k["general"] >= 1
        if cs.aim:
            _check_aim(cs, k, trace)


def test_the_groups_cover_every_route_between_them(mico):
    tot = dict.fromkeys(M.NAMES, 0)
    for group in S.GROUPS:
        for cs in S.group(group):
            for name, v in S.model(cs)[0].items():
                tot[name] += v
    assert all(tot[n] > 0 for n in M.NAMES), tot


def test_the_histogram_case_leaves_the_window(mico):
    """16 bits: tokens above the 8192-bin window (the delimiter, the escaped value) and below it; a thread of eight plain literals
    with exactly one of them outside (the mixed branch)"""
    (cs,) = S.group("hist")
    thr = S.thr_of(cs.maxv)
    lo, hi = thr - 4096, thr + 4096
    tok = _oracle_tokens(mico, cs)
    assert (tok >= hi).sum() >= 6 and (tok < lo).sum() >= 3
    x = cs.sym
    same, _, _ = M.symbol_facts(x, thr - 3)
    outside = (x < lo) | (x >= hi)
    mixed = 0
    for t in S.model(cs)[1]:
        if t[2] == 0:
            continue
        i = t[1] - 3 + np.arange(M.TILE)
        ok = (np.arange(M.TILE) < t[2]) & (i >= 0)
        ii = np.clip(i, 0, x.size - 1)
        o8 = (outside[ii] & ok).reshape(-1, 8).sum(1)
        plain = ok.reshape(-1, 8).all(1) & ~(same[ii] & ok).reshape(-1, 8).any(1)
        mixed += int(((o8 == 1) & plain).sum())
    assert mixed >= 1


def test_the_symbol_unit_has_its_run_and_its_stretch(mico):
    """the WaveletV2 frame: over three tiles, a zero run across a tile border, a run-free stretch"""
    img = S.wavelet_frame()
    a, applied = W.forward(img, 5)
    sym = W.coeffs_to_u16(W.collect(a, applied)).astype(np.int64)
    assert applied == 5 and sym.size >= 3 * M.TILE and not (sym == W.ESCAPE).any()
    runs = _same_runs(sym)
    # symbol i sits at window position i + 3 of the unit (nothing is pre-seeded for a symbol unit)
    assert any(sym[s] == 0 and (s + 3) // M.TILE != (s + n + 2) // M.TILE and n > 1000 for s, n in runs)
    ends = [0] + [s + n for s, n in runs]
    starts = [s for s, n in runs] + [sym.size]
    assert max(b - e for e, b in zip(ends, starts)) > 512
    maxv = (1 << int(sym.max()).bit_length()) - 1
    k, trace = M.predict(sym, 1, sym.size, maxv, src=1)
    assert k["general"] == len(trace) - k["fast"] and k["packed"] == sym.size // 8 and k["kind2"] == 0 and k["perlane"] > 0
    rc, back = mico.rle_decompress(mico.rle_compress(sym.astype(np.uint16), maxv), sym.size)
    assert rc == 0 and np.array_equal(back, sym)


def test_the_model_and_the_kernel_share_their_constants():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "medical-image-codec_amd", "csrc", "mic_encode.hip")).read()
    dev = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "medical-image-codec_amd", "csrc", "mic_dev.h")).read()

    def define(text, name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))

    assert define(src, "TK_THREADS") == M.THREADS and define(src, "TK_PPT") == M.PPT and define(src, "TK_SPT") == M.PPT
    assert M.TILE == M.THREADS * M.PPT
    assert re.search(r"fast_cool = tile_fast \? 0u : (\d+)u", src).group(1) == str(M.COOL)
    assert "__popcll(cf_bal) > 16" in src and "rank < 8" in src and "c >= 16 && g0 >= 6" in src
    assert [define(dev, "MIC_TKP_" + n.upper()) for n in M.NAMES] == list(range(len(M.NAMES))) and define(dev, "MIC_TK_PATHS") == len(M.NAMES)
