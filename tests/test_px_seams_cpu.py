"""What tests/test_gpu_px_seams.py rests on, checked without a device (tests/px_seam_streams.py): every hand-written stream codes
through both doors with rc 0 and for the kernel of its door, the oracle decodes it to the status, token count and pixel hash on
record in tests/golden/px_seam_cases.json and to exactly what the plain decoder gives, every case HAS the property it is named for
-- the model of the kernels' geometry finds the marker at the named symbol, the named tile scanned with entry state 1, the row of
nine pieces or 513 escapes, the table reload -- and the set as a whole reaches every path bit in both of its states.  No case is
skipped: a stream that did not code would fail here."""
import numpy as np
import pytest

import px_seam_streams as S

CASES = S.cases()
NAMES = [c.name for c in CASES]


def test_every_case_codes_and_the_oracle_decodes_it_as_recorded_and_as_the_plain_decoder_does(mico):
    rec = S.golden()
    assert set(rec) == {f"{n}/{d}" for n, d in S.ids()}
    rejected = 0
    for name, door in S.ids():
        c = S.case(name)
        w, h, blob, kernel, rc, px = S.coded(mico, name, door)            # (asserts rc == 0 of fse_compress and the door's kernel)
        g = rec[f"{name}/{door}"]
        assert (rc, int(c.tokens.size)) == (g["status"], g["tokens"]), (name, door, rc)
        assert rc == c.claims.get("status", 0), (name, door, rc)
        if rc == 0:
            assert f"{mico.fnv1a64(px.tobytes()):016x}" == g["pixels_fnv1a64"], (name, door)
            assert c.facts.pixels is not None and np.array_equal(px, c.facts.pixels), (name, door)
        else:
            assert c.facts.pixels is None and S.model_px(c.facts)["status"] == rc, (name, door)
            rejected += 1
    assert rejected == len(S.case("px/last_pixel_escape_without_payload").doors)


def test_the_writer_and_the_plain_decoder_agree_with_the_oracles_tokeniser(mico, synth):
    """a natural frame's tokens, written by the oracle: the plain decoder's pixels are the frame, and the writer puts the same tokens
    back together from the segments the decoder found"""
    img = np.ascontiguousarray(synth.xr_like(cols=364, rows=40, depth=12, seed=5, noise=18.0)[:, 32:332])
    img[7, 100:103] = (0, 4095, 0)                                        # (escapes)
    tok = mico.delta_rle_compress(img, 4095)
    f = S.Facts(tok, 300, 40)
    assert np.array_equal(f.pixels, img) and f.used == f.nsym == len(f.syms) and (f.kind == S.MARKER).sum() >= 3
    items = [("run", int((list(f.segy) + [f.nsym])[i + 1] - f.segy[i]), int(tok[f.segx[i]])) if f.segrun[i] else
             ("lit", tok[f.segx[i]:f.segx[i] + (list(f.segy) + [f.nsym])[i + 1] - f.segy[i]]) for i in range(f.nseg)]
    assert np.array_equal(S.write_tokens(4095, items), tok)


def test_the_escape_heavy_frame_overflows_the_small_token_slab_and_nothing_else(mico):
    for door in S.DOORS:
        img, blob, kernel, tok = S.escape_heavy(mico, door)
        px = img.size
        assert px + px // 8 + 4096 < tok.size <= 4 * px + 16             # tier 1's token slab < tokens <= tier 2's
        assert len(np.unique(tok)) < 64 and (S.Facts(tok, img.shape[1], img.shape[0]).kind == S.MARKER).sum() >= px - 1
        rc, got = mico.decompress_single_frame(blob, img.shape[1], img.shape[0])
        assert rc == 0 and np.array_equal(got, img)


def _tile_word(t):
    return t["kind"] if t["kind"] == "plain" else "scan%d" % t["entry"]


@pytest.mark.parametrize("name", NAMES)
def test_a_case_has_the_property_it_is_named_for(name):
    c = S.case(name)
    f, cl = c.facts, c.claims
    px, rows = S.model_px(f), S.model_rows(f)
    assert f.nseg == len(f.segy) and f.syms[0] == c.maxv and f.ntok == c.tokens.size
    # the kernels' recurrence and the pull decoder name the same markers over the symbols the pixels use
    used = f.used if f.pixels is not None else f.nsym
    assert np.array_equal(f.marker[:used], f.kind[:used] == S.MARKER), name
    for s in cl.get("markers", ()):
        assert f.kind[s] == S.MARKER, (name, s)
    for s in cl.get("payloads", ()):
        assert f.kind[s] == S.PAYLOAD, (name, s)
    for i, word in cl.get("tiles", {}).items():
        assert _tile_word(px["tiles"][i]) == word, (name, i, _tile_word(px["tiles"][i]))
    if "run_at" in cl:
        j = f.seg_of(cl["run_at"])
        assert f.segrun[j] and f.segy[j] == cl["run_at"] and c.tokens[f.segx[j]] == f.delim
    if "delim" in cl:
        assert f.delim == cl["delim"] and (f.syms[0] == f.delim) == (c.maxv in (255, 2047, 65535))
    if "last_token_is_payload" in cl:
        assert f.used == f.nsym and f.kind[f.nsym - 1] == S.PAYLOAD and not f.segrun[-1] and f.segx[-1] + (f.nsym - f.segy[-1]) == f.ntok
    if "last_symbol" in cl:
        assert f.used - 1 == cl["last_symbol"] and f.npx == 8190
    if "ntiles" in cl:
        assert len(px["tiles"]) == cl["ntiles"]
    if "surplus" in cl:
        assert f.nsym - f.used >= cl["surplus"] and (f.syms[f.used:f.nsym] == f.delim).any()
        assert (f.syms[f.used:len(px["tiles"]) * S.PX_T] == f.delim).any() and (f.syms[len(px["tiles"]) * S.PX_T:f.nsym] == f.delim).any()
    if "reload" in cl:
        assert any(t["reload"] for t in px["tiles"]) == cl["reload"]
    if "min_segments_per_tile" in cl:
        assert max(t["segments"] for t in px["tiles"]) >= cl["min_segments_per_tile"]
    if "fetch" in cl:
        i0, form, nsegs = cl["fetch"]
        assert i0 % S.PX_SPT == 0 and S.fetch_form(f, i0) == (form, nsegs)
    if "vector_ends_stream" in cl:
        i0 = cl["fetch"][0]
        j = f.seg_of(i0)
        assert i0 + S.PX_SPT == f.nsym and f.segx[j] + (i0 - f.segy[j]) + S.PX_SPT == f.ntok
    # ---- k_dec_rows_tok ----
    if name.startswith("rows/"):
        assert rows["seen"] and rows["taken"] == cl["taken"], (name, rows["why"])
        assert 8 <= f.h <= 24 and rows["ch"] == {1100: 26, 2688: 50}[f.w]
    else:
        assert f.npx <= 27000 and (not rows["seen"] or c.doors == ("one_state",))
    for y, want in cl.get("row", {}).items():
        got = rows["rows"][y]
        for k, v in want.items():
            assert got[k] == v, (name, y, k, got[k], v)
    if "have" in cl:
        last = rows["rows"][-1]
        assert min(f.w + S.RF_SLACK, f.nsym - last["spos"]) == f.nsym - last["spos"] == cl["have"]
    if "nseg" in cl:
        assert f.nseg == cl["nseg"]
    if "nseg_delta" in cl:
        assert f.nseg == 16 * f.h + 64 + cl["nseg_delta"] and (rows["why"] == "unit") == (cl["nseg_delta"] > 0)
    if "row_is_run" in cl:
        assert f.segrun[rows["rows"][cl["row_is_run"]]["first_seg"]]
    if "piece_ends" in cl:
        y, ends = cl["piece_ends"]
        r = rows["rows"][y]
        assert [int(f.segy[r["first_seg"] + 1 + i]) - r["spos"] for i in range(len(ends))] == ends
    if "slack_pieces" in cl:
        y, n = cl["slack_pieces"]
        assert rows["rows"][y]["slack_pieces"] >= n
    if "run_value_token" in cl:
        end, n = cl["run_value_token"]
        j = f.seg_of(1) if end == "first" else f.nseg - 1
        assert f.segrun[j] and (f.segx[j] == n if end == "first" else f.ntok - f.segx[j] == n) and (f.segx[j] < 8 or f.segx[j] >= f.ntok - 8)


def test_the_cases_reach_every_path_bit_in_both_states():
    for door in S.DOORS:
        seen = [S.expected_paths(c.facts, door) for c in CASES if door in c.doors]
        for bit in S.PX_BITS + (S.ROW_BITS if door == "two_state" else ()):
            states = {bool(b & bit) for b, taken in seen if taken == (bit in S.ROW_BITS)}
            assert states == {False, True}, (door, bit, states)
    taken = {S.expected_paths(c.facts, "two_state")[1] for c in CASES if c.name.startswith("rows/")}
    assert taken == {False, True}
    why = {S.model_rows(c.facts)["why"] for c in CASES if c.name.startswith("rows/")}
    assert {"", "escapes", "unit"} <= why


def test_the_models_constants_are_the_sources(mic):
    """the constants the model restates, read back from the sources they name"""
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.abspath(mic.__file__)), "csrc")
    text = {n: open(os.path.join(src, n)).read() for n in ("mic_decode_px.hip", "mic_decode_fused.hip", "mic_launch.h", "mic_dev.h")}

    def define(name, where):
        return re.search(r"#define\s+%s\s+(.+?)\s*(//.*)?$" % name, text[where], re.M).group(1)
    assert int(define("PX_T", "mic_decode_px.hip")) == S.PX_T and int(define("PX_THREADS", "mic_decode_px.hip")) == S.PX_THREADS
    assert define("PX_SPT", "mic_decode_px.hip") == "(PX_T / PX_THREADS)" and S.PX_T // S.PX_THREADS == S.PX_SPT
    assert "r0 += PX_THREADS - PX_SPT" in text["mic_decode_px.hip"] and S.PX_STEP == S.PX_THREADS - S.PX_SPT
    assert int(define("RF_SLACK", "mic_decode_fused.hip")) == S.RF_SLACK and "CH = K + 8" in text["mic_decode_fused.hip"]
    assert "nseg > 16u * (uint32_t)H + 64u" in text["mic_decode_fused.hip"] and "need_m & 0x100ull" in text["mic_decode_fused.hip"]
    assert (int(define("MIC_ROWS_LO", "mic_launch.h")), int(define("MIC_ROWS_HI", "mic_launch.h"))) == (S.ROWS_LO, S.ROWS_HI)
    assert [S.rows_k(w) for w in (1008, 1009, 1100, 1152, 1153, 2688, 2689)] == [0, 18, 18, 18, 22, 42, 0]
    for name, bit in (("PLAIN_TILE", S.PLAIN_TILE), ("SCAN_TILE", S.SCAN_TILE), ("SCAN_ENTRY1", S.SCAN_ENTRY1), ("TABLE_RELOAD", S.TABLE_RELOAD),
                      ("PREFETCH", S.PREFETCH), ("ROW_GATHER", S.ROW_GATHER), ("ROW_PIECEWISE", S.ROW_PIECEWISE), ("ROW_ESCAPE", S.ROW_ESCAPE),
                      ("ROW_REDO", S.ROW_REDO)):
        assert 1 << int(re.fullmatch(r"\(1u << (\d+)\)", define("MIC_PXP_" + name, "mic_dev.h")).group(1)) == bit, name
    assert re.search(r"MIC_STAGE_PIXELS\s*=\s*%d," % S.STAGE_PIXELS, text["mic_dev.h"])
