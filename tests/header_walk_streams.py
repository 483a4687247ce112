"""Token streams that put an RLE header on every seam of the decode chain's header walks (tests/test_gpu_header_walk.py): the
serial walker of csrc/mic_rlewalk.h inside k_dec_translate and k_dec_tans_gl, the all-lanes walk of k_dec_translate, and phase 1 of
k_dec_pixels_wg.

A stream is the oracle's delta_rle_compress of a frame with one header rewritten (two tokens where one cannot do it, the dense case a
handful), coded again by the oracle's FSE so that the entropy stage accepts it.  What such a stream MEANS is the oracle's business:
its decode status per case is recorded in tests/golden/header_walk_cases.json and checked without a device.

Token 0 fixes midCount; a header h <= midCount is a run (count, value: two tokens), a larger one a literal chunk of h - midCount
symbols behind it (rledecompressu16.go:59-85)."""
import json
import os

import numpy as np

import decode_class_streams as D

TILE = D.TILE                     # tokens per tile of k_dec_translate (TR_TILE)
DENSE = 6                         # headers in a tile from which on k_dec_translate walks the next one with all lanes (TR_DENSE)
WINDOW = 64                       # tokens a walker holds in registers
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "header_walk_cases.json")

SHAPES = {"fused": (1100, 6), "narrow": (300, 24)}        # the narrowest class of k_dec_rows_tok; the two-kernel path
DOORS = ("two_state", "one_state", "gl")
CASES = ("clean", "zero_first", "zero_last24", "run_at_last_token", "literal_to_last_token", "literal_past_last_token",
         "header_at_1535", "header_at_1536", "header_at_1537", "next_header_63", "next_header_64", "next_header_65", "dense_then_none")


def mid_count(t):
    return (1 << (int(t[0]).bit_length() - 1)) - 1


def headers(t):
    """token positions of the headers of a well-formed stream, and the position behind the last payload"""
    mid, pos, out = mid_count(t), 1, []
    while pos < t.size:
        out.append(pos)
        h = int(t[pos])
        assert h != 0
        pos += 2 if h <= mid else 1 + h - mid
    return out, pos


def frame(synth, shape):
    """w x h pixels out of an xr_like frame, between its collimator border (which would leave a frame of a few rows empty) and its
    markers (whose runs would leave it short of tokens)"""
    w, h = SHAPES[shape]
    return np.ascontiguousarray(synth.xr_like(cols=w + 64, rows=h + 256, depth=12, seed=11, noise=18.0)[8:8 + h, 32:32 + w])


def gl_frame(mico):
    """a frame of the tableLog-16 class with 0-bit entries, which k_dec_tans_gl decodes (decode_class_streams.class_batch)"""
    return D.class_batch(mico, 16, 2, 1)[0].img


def edited(t, case):
    """the tokens of `case`.  The stream must begin and end with a literal chunk and have a header behind token 4 TILE."""
    t = t.copy()
    mid = mid_count(t)
    H, end = headers(t)
    n = t.size
    assert end == n and n > 4 * TILE + WINDOW and t[H[-1]] > mid and t[1] > mid

    def literal(p, nxt):                                    # header p becomes a literal chunk, the next header is token nxt
        assert nxt - p >= 2 and mid + nxt - p - 1 <= 65535
        t[p] = mid + (nxt - p - 1)

    last = H[-1]
    before = max(p for p in H[:-1] if t[p] > mid)           # the last literal chunk but one
    if case == "clean":
        pass
    elif case == "zero_first":
        t[1] = 0
    elif case == "zero_last24":
        z = last
        if z < n - 24:                                      # the last chunk is cut short: the walk lands twelve tokens from the end
            z = n - 12
            literal(last, z)
        t[z] = 0
    elif case == "run_at_last_token":                       # the last chunk one token shorter; a count without a value behind it
        literal(last, n - 1)
        t[n - 1] = 3
    elif case == "literal_to_last_token":                   # the chunk before the last takes the last one in, header and all
        literal(before, n)
    elif case == "literal_past_last_token":
        literal(before, n + 1)
    elif case.startswith("header_at_"):
        at = int(case[len("header_at_"):])
        literal(max(p for p in H if p <= at - 2), at)       # whatever lies at `at` is read as a header
    elif case.startswith("next_header_"):
        literal(1, 1 + int(case[len("next_header_"):]))     # the first header's window is tokens 1 .. 64
    elif case == "dense_then_none":
        # Written over whatever lies there.  Tile 0: one header (walked header to header, as is tile 1 behind it); tile 1: seven runs
        # side by side and a literal chunk that reaches over ALL of tile 2 (no header: the walk is not called, the all-lanes choice
        # stands) into tile 3, which the all-lanes walk takes and leaves with one header: header to header again in tile 4, and back
        # to the stream's own headers.  The runs are long enough to make up for the symbols the long chunks' headers cost.
        a, b, c = TILE + 10, 3 * TILE + 100, 4 * TILE + 20
        literal(1, a)
        for k in range(7):
            t[a + 2 * k], t[a + 2 * k + 1] = 64, mid              # (a value that is no delimiter)
        literal(a + 14, b)
        literal(b, c)
        literal(c, min([p for p in H if p >= c + 2] + [n]))       # (back on the stream's own chain, or at its end)
    else:
        raise KeyError(case)
    return t


def code(mico, t, door):
    """(rc, blob, facts) of the tokens coded for a door"""
    nstates, tl = {"two_state": (2, 0), "one_state": (1, 0), "gl": (2, 16)}[door]
    rc, blob = mico.fse_compress_tl(t, nstates, tl) if tl else mico.fse_compress(t, nstates)
    frc, facts = mico.fse_stream_facts(t, nstates, tl)
    return rc or frc, blob, facts


def expected_kernel(door, facts):
    """MicUnit.dec_kernel of the door: 1 + class of k_dec_tans_ls (states go through k_dec_translate), k_dec_tans_serial (symbols; the
    walk is k_dec_pixels_wg's), k_dec_tans_gl (symbols and its own walker)"""
    rec = D.dec_record(1 if door == "one_state" else 2, facts["table_log"], facts["zero_bits"])
    assert {"two_state": 1 <= rec <= 30, "one_state": rec == D.BY_SERIAL, "gl": rec == D.BY_GL}[door], (door, facts, rec)
    return rec


_tokens = {}


def streams(mico, synth, door, shape):
    """{case: (w, h, blob, expected dec_kernel, oracle status, oracle pixels or None)} of one door and frame"""
    key = (door, shape)
    if key not in _tokens:
        img = gl_frame(mico) if door == "gl" else frame(synth, shape)
        tok = mico.delta_rle_compress(img, 255 if door == "gl" else 4095)
        out = {}
        for case in CASES:
            rc, blob, facts = code(mico, edited(tok, case), door)
            assert rc == 0, (door, shape, case, rc)          # no case may drop out
            h, w = img.shape
            rc_o, want = mico.decompress_single_frame(blob, w, h)
            out[case] = (w, h, blob, expected_kernel(door, facts), rc_o, want)
        _tokens[key] = (int(tok.size), out)
    return _tokens[key]


def pairs():
    return [(door, shape) for door in DOORS for shape in (("gl",) if door == "gl" else tuple(SHAPES))]


def golden():
    return json.load(open(GOLDEN))
