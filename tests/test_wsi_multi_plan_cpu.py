"""mic_hip_wsi_multi_patch_plan (no device): the (slide, tile) units a batch of patches over many slides and levels needs decoded,
against the single-level planner mic_hip_wsi_patch_plan applied to each (slide, level) group.  The files come from the oracle's
CompressWSI, which must encode every test slide."""
import ctypes as C

import numpy as np
import pytest

import wsi_patch_slides as S
import wsi_multi_slides as M

GARBAGE = bytes(range(256)) * 2


@pytest.fixture(scope="module")
def files(mico):
    """fmt -> ([file of A, B, C], [Mic3File])"""
    out = {}
    for fmt in S.FORMATS:
        data = []
        for name in M.NAMES:
            rc, d = M.oracle_file(mico, name, fmt)
            assert rc == 0, (fmt, name, rc)
            data.append(d)
        out[fmt] = (data, [S.Mic3File(d) for d in data])
    return out


def _want(mic, parsed, q, pw, ph):
    """units and pieces of the patches q from the single-level planner, group by group"""
    units, pieces = set(), 0
    for s, f in enumerate(parsed):
        tw, th = M.tile_size(f)
        for level, (lw, lh, _, _, first) in enumerate(f.levels):
            xy = [(x, y) for x, y, fs, fl in q if (fs, fl) == (s, level)]
            tiles, npc = mic.wsi_patch_plan(lw, lh, tw, th, xy, pw, ph)
            units.update((s, first + int(t)) for t in tiles)
            pieces += npc
    return sorted(units), pieces


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_the_oracle_encodes_every_slide(mico, files, fmt):
    data, parsed = files[fmt]
    for name, d, f in zip(M.NAMES, data, parsed):
        w, h, tw, th, levels = M.GEOMETRY[name]
        assert f.nlev == levels and f.levels[0][:2] == (w, h) and M.tile_size(f) == (tw, th), name
    assert 3 in parsed[0].modes(S.NOISE_TILE)


@pytest.mark.parametrize("fmt", S.FORMATS)
@pytest.mark.parametrize("patch", M.PATCHES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_units_ascend_and_counts_are_the_groups_sums(mic, files, fmt, patch):
    data, parsed = files[fmt]
    pw, ph = patch
    q = M.patch_list(parsed, pw, ph)
    slide_of, tile_of, pieces, fs = mic.wsi_multi_patch_plan(data, q, pw, ph, **S.fmt_args(fmt))
    units = list(zip(slide_of.tolist(), tile_of.tolist()))
    assert units == sorted(set(units))                                   # ascending by (slide, tile), each once
    want_units, want_pieces = _want(mic, parsed, q, pw, ph)
    assert units == want_units and pieces == want_pieces
    assert {s for s, _ in units} == {0, 1, 2} and (fs == mic.MIC_OK).all()


def test_a_garbage_file_is_looked_at_only_when_named(mic, files):
    data, parsed = files["rgb"]
    pw, ph = 24, 20
    q = [(x, y, 2 * s, level) for x, y, s, level in M.patch_list(parsed[:2], pw, ph)]          # slides 0 and 2 of [A, garbage, B]
    three = [data[0], GARBAGE, data[1]]
    slide_of, tile_of, pieces, fs = mic.wsi_multi_patch_plan(three, q, pw, ph)
    assert fs.tolist() == [mic.MIC_OK] * 3 and set(slide_of.tolist()) == {0, 2}
    base = (slide_of.tolist(), tile_of.tolist(), pieces)
    # named: it fails alone, with the header's code, and adds no unit and no piece
    slide_of, tile_of, pieces, fs = mic.wsi_multi_patch_plan(three, q + [(0, 0, 1, 0), (5, 5, 1, 1)], pw, ph)
    assert fs.tolist() == [mic.MIC_OK, mic.MIC_ERR_CORRUPT, mic.MIC_OK]
    assert (slide_of.tolist(), tile_of.tolist(), pieces) == base


def test_a_level_out_of_range_contributes_nothing(mic, files):
    data, parsed = files["grey8"]
    pw, ph = 24, 20
    q = M.patch_list(parsed, pw, ph)
    base = mic.wsi_multi_patch_plan(data, q, pw, ph, channels=1, bits_per_sample=8)
    more = q + [(0, 0, 0, S.LEVELS), (0, 0, 1, 2), (0, 0, 2, -1), (0, 0, 0, 1000)]
    got = mic.wsi_multi_patch_plan(data, more, pw, ph, channels=1, bits_per_sample=8)
    assert got[0].tolist() == base[0].tolist() and got[1].tolist() == base[1].tolist() and got[2] == base[2]
    assert (got[3] == mic.MIC_OK).all()
    only = mic.wsi_multi_patch_plan(data, more[len(q):], pw, ph, channels=1, bits_per_sample=8)
    assert only[0].size == 0 and only[2] == 0


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_a_slide_of_another_format_fails_alone(mic, files, fmt):
    data, parsed = files[fmt]
    other = files[M.OTHER_FORMAT[fmt]][0][1]                            # slide D: B in another format
    pw, ph = 24, 20
    q = M.patch_list(parsed, pw, ph)
    base = mic.wsi_multi_patch_plan(data, q, pw, ph, **S.fmt_args(fmt))
    got = mic.wsi_multi_patch_plan(data + [other], q + [(0, 0, 3, 0), (10, 10, 3, 1)], pw, ph, **S.fmt_args(fmt))
    assert got[3].tolist() == [mic.MIC_OK] * 3 + [mic.MIC_ERR_ARGS]
    assert got[0].tolist() == base[0].tolist() and got[1].tolist() == base[1].tolist() and got[2] == base[2]


def test_argument_errors(mic, files):
    data, parsed = files["rgb"]
    for q in ([(0, 0, 3, 0)], [(0, 0, -1, 0)], [(0, 0, 0, 0), (0, 0, 99, 0)]):      # a slide index outside [0, nfiles)
        with pytest.raises(mic.MicError) as e:
            mic.wsi_multi_patch_plan(data, q, 24, 20)
        assert e.value.code == mic.MIC_ERR_ARGS
    for pw, ph in ((0, 20), (24, 0), (-1, 20)):
        with pytest.raises(mic.MicError) as e:
            mic.wsi_multi_patch_plan(data, [(0, 0, 0, 0)], pw, ph)
        assert e.value.code == mic.MIC_ERR_ARGS
    for ch, bps in ((3, 16), (2, 8), (1, 12), (4, 8)):                     # not a format Mic3 codes: before a file is looked at
        with pytest.raises(mic.MicError) as e:
            mic.wsi_multi_patch_plan([GARBAGE], [(0, 0, 0, 0)], 24, 20, channels=ch, bits_per_sample=bps)
        assert e.value.code == mic.MIC_ERR_UNSUPPORTED


def test_too_small_a_cap_reports_the_counts_and_leaves_the_arrays(mic, files):
    data, parsed = files["rgb"]
    pw, ph = 71, 37
    q = M.patch_list(parsed, pw, ph)
    slide_of, tile_of, pieces, fs = mic.wsi_multi_patch_plan(data, q, pw, ph)
    with pytest.raises(mic.MicError) as e:
        mic.wsi_multi_patch_plan(data + [GARBAGE], q + [(0, 0, 3, 0)], pw, ph, cap=slide_of.size - 1)
    assert e.value.code == mic.MIC_ERR_CAPACITY and e.value.ntiles == slide_of.size and e.value.pieces == pieces
    assert e.value.file_status.tolist() == [0, 0, 0, mic.MIC_ERR_CORRUPT]
    # the arrays are untouched
    arrs = [np.frombuffer(d, dtype=np.uint8) for d in data]
    ptrs = np.asarray([a.ctypes.data for a in arrs], dtype=np.uintp)
    lens = np.asarray([a.size for a in arrs], dtype=np.uintp)
    a = np.asarray(q, dtype=np.int32)
    so, to = np.full(slide_of.size, 0xABCD, dtype=np.uint32), np.full(slide_of.size, 0xABCD, dtype=np.uint64)
    nt, npc = C.c_uint64(0), C.c_uint64(0)
    rc = mic.lib().mic_hip_wsi_multi_patch_plan(ptrs.ctypes.data, lens.ctypes.data, 3, a.ctypes.data, len(a), pw, ph, 3, 8,
                                                so.ctypes.data, to.ctypes.data, slide_of.size - 1, C.byref(nt), C.byref(npc), None)
    assert rc == mic.MIC_ERR_CAPACITY and (nt.value, npc.value) == (slide_of.size, pieces)
    assert (so == 0xABCD).all() and (to == 0xABCD).all()
    rc = mic.lib().mic_hip_wsi_multi_patch_plan(ptrs.ctypes.data, lens.ctypes.data, 3, a.ctypes.data, len(a), pw, ph, 3, 8,
                                                so.ctypes.data, to.ctypes.data, slide_of.size, C.byref(nt), C.byref(npc), None)
    assert rc == mic.MIC_OK and so.tolist() == slide_of.tolist() and to.tolist() == tile_of.tolist()


def test_no_patches_and_no_files(mic, files):
    data, _ = files["rgb"]
    slide_of, tile_of, pieces, fs = mic.wsi_multi_patch_plan(data, [], 24, 20)
    assert slide_of.size == 0 and tile_of.size == 0 and pieces == 0 and fs.tolist() == [0, 0, 0]
    slide_of, tile_of, pieces, fs = mic.wsi_multi_patch_plan([], [], 24, 20)
    assert slide_of.size == 0 and pieces == 0 and fs.size == 0
    L = mic.lib()
    nt = C.c_uint64(9)
    assert L.mic_hip_wsi_multi_patch_plan(None, None, 0, None, 0, 24, 20, 3, 8, None, None, 0, C.byref(nt), None, None) == mic.MIC_OK
    assert nt.value == 0
    assert L.mic_hip_wsi_multi_patch_plan(None, None, 1, None, 0, 24, 20, 3, 8, None, None, 0, None, None, None) == mic.MIC_ERR_ARGS
    assert L.mic_hip_wsi_multi_patch_plan(None, None, 0, None, 1, 24, 20, 3, 8, None, None, 0, None, None, None) == mic.MIC_ERR_ARGS
    assert L.mic_hip_wsi_multi_patch_plan(None, None, 0, None, -1, 24, 20, 3, 8, None, None, 0, None, None, None) == mic.MIC_ERR_ARGS
    assert L.mic_hip_wsi_multi_patch_plan(None, None, -1, None, 0, 24, 20, 3, 8, None, None, 0, None, None, None) == mic.MIC_ERR_ARGS
