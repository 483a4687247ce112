"""What can be said without a device about the cases of tests/test_gpu_grad_predict.py (tests/grad_predict_frames.py): the oracle
codes every frame and brings it back, every pixel a case is named for really is an escape (or really is not), the set as a whole
reaches every seam of k_dec_predict_grad, and the stream sets hold enough decodable, differing, out-of-range and refused streams
by the oracle alone -- a case cannot silently stop aiming at its seam.

And the one job no GPU test can do: the oracle's gradient DECODER, which every device comparison trusts, is pinned by a serial
pure-Python restatement of GradDeltaRleDecompressU16.Decompress (deltagradrlecompressu16.go:71-133) -- on every tiny frame and on
token streams whose pixels wrap around 16 bits, where a round trip says nothing."""
import numpy as np
import pytest

import grad_predict_frames as F
from test_oracle_pica import grad_predict_np, rle_expand_py
from tokeniser_streams import grad_predict, thr_of


def _is_escape(cs, y, x):
    return abs(int(cs.img[y, x]) - F.predict_at(cs.img, y, x)) >= thr_of(cs.maxv)


@pytest.mark.parametrize("name", tuple(F.FAMILIES))
def test_every_frame_is_coded_and_holds_the_escapes_it_is_named_for(mico, synth, name):
    cases = F.family(synth, name)
    assert len({cs.name for cs in cases}) == len(cases)
    for cs in cases:
        h, w = cs.img.shape
        rc, blob = mico.compress_single_frame_grad(cs.img, cs.maxv)
        assert rc == 0 and len(blob) > 6, (cs.name, rc)                      # (an incompressible frame would test nothing)
        rc, back = mico.decompress_single_frame_grad(blob, w, h)
        assert rc == 0 and np.array_equal(back, cs.img), cs.name
        assert cs.aim["esc"], cs.name
        for y, x in cs.aim["esc"]:
            assert _is_escape(cs, y, x), (cs.name, y, x)
        for y, x in cs.aim["plain"]:
            assert not _is_escape(cs, y, x), (cs.name, y, x)
        # the named pixels are escapes for the oracle's tokeniser too: it writes at least as many delimiters
        tok = mico.grad_delta_rle_compress(cs.img, cs.maxv)
        if w * h <= 70000:
            assert int((rle_expand_py(tok)[1:] == (1 << int(cs.maxv).bit_length()) - 1).sum()) >= len(cs.aim["esc"]), cs.name


def _all_cases(synth):
    return [cs for name in F.FAMILIES for cs in F.family(synth, name)]


def test_the_frames_reach_every_group_band_and_flag_seam(synth):
    cases = _all_cases(synth)
    # the four code paths of the last column, each with an escape in it
    assert {cs.img.shape[1] % 4 for cs in cases if any(x == cs.img.shape[1] - 1 for _, x in cs.aim["esc"])} == {0, 1, 2, 3}
    # the band hand-over: escapes in the row lane 63 writes and in the row lane 0 rebuilds, at every position of a group
    upper = {x % 4 for cs in cases for y, x in cs.aim["esc"] if y % 64 == 63}
    lower = {x % 4 for cs in cases for y, x in cs.aim["esc"] if y % 64 == 0 and y >= 64}
    assert upper == lower == {0, 1, 2, 3}
    # ... and plain pixels beside them, so that the handed-over row is read by a prediction
    # (in one of a shape's variants at least: three columns of a last row can all be escapes)
    plain64 = {}
    for cs in cases:
        h, w = cs.img.shape
        if h > 64 and w > 2 and cs.name.startswith(("tiny", "band")):
            plain64[(w, h)] = plain64.get((w, h), False) or any(not _is_escape(cs, 64, x) for x in range(w))
    assert plain64 and all(plain64.values()), plain64
    # the hand-over inside a step: column 4 q + 3 under an escape in column 4 q + 4 of the row above, itself an escape / plain
    both = [(cs.name, y) for cs in cases for y, x in cs.aim["esc"] if x % 4 == 3 and (y - 1, x + 1) in cs.aim["esc"]]
    alone = [(cs.name, y) for cs in cases for y, x in cs.aim["plain"] if x % 4 == 3 and (y - 1, x + 1) in cs.aim["esc"]]
    assert both and alone
    assert any(y % 64 == 0 for _, y in both) and any(y % 64 == 0 for _, y in alone) and any(y % 64 for _, y in both)
    # the two flag words of a group, recounted from the escapes themselves
    straddle = spare = 0
    for cs in cases:
        h, w = cs.img.shape
        hit = any(w % 2 and ((y * w + (x & ~3)) % 32) + (x & 3) >= 32 and _is_escape(cs, y, x) for y, x in cs.aim["esc"])
        assert hit == ("straddle" in cs.aim["props"]), cs.name
        straddle += hit
        last = (w * h) % 32 == 0 and _is_escape(cs, h - 1, w - 1)
        assert last == ("spare" in cs.aim["props"]), cs.name
        spare += last
    assert straddle >= 1 and spare >= 1
    assert any(cs.img.shape == (64, 64) and "spare" in cs.aim["props"] for cs in cases)
    # every row-buffer class at both ends, and 16-bit frames
    assert {cs.img.shape[1] for cs in F.family(synth, "class")} == set(F.CLASS_WIDTHS)
    assert all(cs.maxv == 65535 for cs in F.family(synth, "deep"))


def test_the_stream_sets_meet_their_floors_by_the_oracle_alone(mico, synth):
    wrap = F.stream_counts(F.wrapping_streams(mico, synth), F.oracle_decodes(mico, synth, "wrapping"))
    assert all(wrap[k] >= v for k, v in F.WRAP_FLOORS.items()), wrap
    dmg = F.stream_counts(F.damaged_streams(mico, synth), F.oracle_decodes(mico, synth, "damaged"))
    assert all(dmg[k] >= v for k, v in F.DAMAGE_FLOORS.items()), dmg
    print("wrapping", wrap, "damaged", dmg)


# ---- the oracle's decoder against a serial restatement ---------------------------------------------------------------------------
def grad_decode_py(tok, w, h):
    """GradDeltaRleDecompressU16.Decompress: row 0 from the left pixel (the corner from 0), column 0 from the pixel above, the
    interior from gradPredict, every sum cut to 16 bits (uint16(predicted + diff), :120)"""
    sym = rle_expand_py(tok).tolist()
    depth = int(sym[0]).bit_length()
    thr, delim = (1 << (depth - 1)) - 1, (1 << depth) - 1
    out = [[0] * w for _ in range(h)]
    i = 1
    for y in range(h):
        row, up = out[y], out[y - 1]
        for x in range(w):
            s = sym[i]; i += 1
            if s == delim:
                row[x] = sym[i]; i += 1
                continue
            if y == 0:
                pred = row[x - 1] if x else 0
            elif x == 0:
                pred = up[0]
            else:
                pred = grad_predict(row[x - 1], up[x], up[x - 1], up[x + 1] if x + 1 < w else up[x - 1])
            row[x] = (pred + s - thr) & 0xFFFF
    return np.asarray(out, np.uint16).reshape(h, w)


def test_the_scalar_predictor_is_the_numpy_restatement():
    """grad_decode_py calls the scalar gradPredict of tokeniser_streams pixel by pixel; it is the vectorised one of
    test_oracle_pica.py, wrapped neighbours (any 16-bit values) included"""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 65536, (4, 20000))
    a[:, :2000] = rng.integers(1000, 1040, (4, 2000))                        # (flat neighbourhoods: g = 0 and small g)
    want = grad_predict_np(*a)
    assert [grad_predict(*(int(v) for v in a[:, k])) for k in range(a.shape[1])] == want.tolist()
    assert int(want.min()) < 0 and int(want.max()) > 65535                   # the prediction itself leaves 16 bits


def test_the_oracles_decoder_is_the_serial_restatement_on_tiny_frames(mico, synth):
    for cs in F.family(synth, "tiny"):
        h, w = cs.img.shape
        tok = mico.grad_delta_rle_compress(cs.img, cs.maxv)
        rc, got = mico.grad_delta_rle_decompress(tok, w, h)
        assert rc == 0 and np.array_equal(got, grad_decode_py(tok, w, h)) and np.array_equal(got, cs.img), cs.name


def test_the_oracles_decoder_is_the_serial_restatement_on_wrapping_streams(mico, synth):
    """token streams whose pixels wrap (the layout of runs and chunks untouched): here only a second decoder can speak"""
    done = wrapped = 0
    for s in F.wrapping_streams(mico, synth):
        if (s.h, s.w) not in ((130, 61), (70, 258)) or s.structural:
            continue
        rc, got = mico.grad_delta_rle_decompress(s.tok, s.w, s.h)
        assert rc == 0, s.name
        assert np.array_equal(got, grad_decode_py(s.tok, s.w, s.h)), s.name
        done += 1
        wrapped += int(got.max()) > s.maxv
    # of 2 x 14 streams those with a replaced header drop out; the clean pair says nothing new: ask for a third of the rest
    assert done >= 10 and wrapped >= 8, (done, wrapped)


# ---- PICA -------------------------------------------------------------------------------------------------------------------------
def test_the_pica_images_flag_every_strip_as_named(mico, synth):
    for name, img, strips, kind in F.pica_images(synth):
        rc, blob = mico.pica_compress(img, 4095, strips)
        assert rc == 0, name
        assert F.pica_flags(blob) == [1 if kind == "grad" else 0] * strips, name
        if kind == "grad":                                                     # every strip one band and 0 .. 4 rows
            edges = F.pica_starts(blob) + [img.shape[0]]
            assert all(64 <= b - a <= 68 for a, b in zip(edges, edges[1:])), (name, edges)
