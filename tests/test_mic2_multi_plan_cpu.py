"""mic_hip_mic2_multi_crop_plan (csrc/mic_mic2_crops.hip), the host planner behind the MIC2 crop calls over many volumes, against
the per-volume enumeration of mic2_crop_volumes.brute_plan.  The files are headers and frame tables made by hand (the planner
reads nothing else).  No device is needed."""
import ctypes as C
import struct

import numpy as np
import pytest

import mic2_multi_volumes as M

# (w, h, n, temporal): the shapes of the GPU tests' volumes
DIMS = [(150, 70, 11, False), (150, 70, 11, True), (160, 96, 6, True), (160, 96, 6, False), (33, 9, 3, True), (7, 5, 1, True), (7, 5, 1, False)]


def _files(dims=DIMS):
    return [M.hand_file(*d) for d in dims]


def _crops(dims, cw, ch, cd):
    return M.interleave([M.V.origins(w, h, n, cw, ch, cd) for w, h, n, _ in dims])


@pytest.mark.parametrize("shape", M.SHAPES)
def test_plan_equals_the_enumeration_volume_by_volume(mic, shape):
    cw, ch, cd = shape
    xyzv = _crops(DIMS, cw, ch, cd)
    assert all(a[3] != b[3] for a, b in zip(xyzv, xyzv[1:]))              # consecutive crops name different volumes
    units, pieces, fs = mic.mic2_multi_crop_plan(_files(), xyzv, cw, ch, cd)
    want_units, want_pieces = M.brute_multi_plan(DIMS, xyzv, cw, ch, cd)
    assert [tuple(u) for u in units.tolist()] == want_units and pieces == want_pieces and pieces > 0
    assert units.dtype == np.uint32 and (fs == 0).all() and fs.size == len(DIMS)
    assert want_units == sorted(set(want_units))                          # ascending by volume, then frame, each once
    got = {v: [f for vv, f in want_units if vv == v] for v in range(len(DIMS))}
    assert got[1] == list(range(11)) and got[5] == [0]                    # temporal: 0 .. the last overlapped frame; n = 1: frame 0 only


def test_a_volume_listed_twice_is_two_volumes(mic):
    f = M.hand_file(150, 70, 11, False)
    t = M.hand_file(150, 70, 11, True)
    xyzv = [(0, 0, 2, 0), (5, 5, 3, 1), (0, 0, 6, 2), (0, 0, 1, 3)]
    units, pieces, fs = mic.mic2_multi_crop_plan([f, f, t, t], xyzv, 17, 5, 2)
    assert [tuple(u) for u in units.tolist()] == [(0, 2), (0, 3), (1, 3), (1, 4)] + [(2, k) for k in range(8)] + [(3, k) for k in range(3)]
    assert pieces == 8 and (fs == 0).all()


def test_unnamed_volumes_are_not_touched(mic):
    good = M.hand_file(150, 70, 11, True)
    xyzv = [(0, 0, 0, 1), (3, 3, 1, 1)]
    units, pieces, fs = mic.mic2_multi_crop_plan([None, good, b"garbage", b"MIC2"], xyzv, 8, 8, 2)
    assert [tuple(u) for u in units.tolist()] == [(1, 0), (1, 1), (1, 2)] and pieces == 4
    assert fs.tolist() == [0, 0, 0, 0]
    # named, they carry their own codes and yield no units
    units, pieces, fs = mic.mic2_multi_crop_plan([None, good, b"garbage", b"MIC2"], xyzv + [(0, 0, 0, 0), (0, 0, 0, 2), (0, 0, 0, 3)], 8, 8, 2)
    assert [tuple(u) for u in units.tolist()] == [(1, 0), (1, 1), (1, 2)] and pieces == 4
    assert fs.tolist() == [mic.MIC_ERR_ARGS, 0, mic.MIC_ERR_CORRUPT, mic.MIC_ERR_CORRUPT]


def test_refused_volumes_keep_their_code_and_yield_no_units(mic):
    good = M.hand_file(33, 9, 3, True)
    bad_magic = M.hand_file(33, 9, 3, True, magic=b"MIC3")
    flat = M.hand_file(0, 9, 3, False)                                    # width 0
    huge = M.hand_file(1 << 15, (1 << 13) + 1, 1, False)                  # more than 2^28 pixels a frame
    short = M.hand_file(33, 9, 3, False)[: 20 + 8 * 3 - 1]                # the table overruns the file
    xyzv = [(0, 0, 0, v) for v in range(5)]
    units, pieces, fs = mic.mic2_multi_crop_plan([bad_magic, good, flat, huge, short], xyzv, 4, 4, 1)
    assert [tuple(u) for u in units.tolist()] == [(1, 0)] and pieces == 1
    info = lambda b: mic.lib().mic_hip_mic2_info(b, len(b), None, None, None, None)
    assert fs.tolist() == [info(bad_magic), 0, mic.MIC_ERR_CORRUPT, mic.MIC_ERR_UNSUPPORTED, info(short)]
    assert info(bad_magic) == info(short) == mic.MIC_ERR_CORRUPT


@pytest.mark.parametrize("temporal", [False, True])
def test_a_bad_table_entry_matters_only_when_its_frame_is_needed(mic, temporal):
    good = M.hand_file(150, 70, 11, temporal)
    for damage in ("empty", "outside"):
        lens = [16] * 11
        if damage == "empty":
            lens[5] = 0
            bad = M.hand_file(150, 70, 11, temporal, lens=lens)
        else:
            b = bytearray(good)
            struct.pack_into("<I", b, 20 + 8 * 5, len(good))              # frame 5's offset: past the end of the file
            bad = bytes(b)
        # frames 0 .. 4 of the bad file are needed: fine; then frame 5 of it: that volume alone fails
        units, pieces, fs = mic.mic2_multi_crop_plan([good, bad], [(0, 0, 4, 0), (0, 0, 3, 1)], 8, 8, 2)
        assert fs.tolist() == [0, 0] and pieces == 4
        assert [tuple(u) for u in units.tolist()] == ([(0, k) for k in range(6)] + [(1, k) for k in range(5)] if temporal else [(0, 4), (0, 5), (1, 3), (1, 4)])
        units, pieces, fs = mic.mic2_multi_crop_plan([good, bad], [(0, 0, 4, 0), (0, 0, 4, 1)], 8, 8, 2)
        assert fs.tolist() == [0, mic.MIC_ERR_CORRUPT] and pieces == 2, damage
        assert [tuple(u) for u in units.tolist()] == ([(0, k) for k in range(6)] if temporal else [(0, 4), (0, 5)])
        if not temporal:                                                  # an independent file's later frames do not depend on it
            units, pieces, fs = mic.mic2_multi_crop_plan([good, bad], [(0, 0, 6, 1)], 8, 8, 2)
            assert fs.tolist() == [0, 0] and [tuple(u) for u in units.tolist()] == [(1, 6), (1, 7)]


def test_a_short_list_is_a_capacity_error_with_the_counts(mic):
    files = _files(DIMS[:3])
    xyzv = [(0, 0, 2, 0), (5, 5, 6, 1), (1, 1, 1, 2), (0, 0, 0, 0)]
    want_units, want_pieces = M.brute_multi_plan(DIMS[:3], xyzv, 17, 5, 3)
    nu = len(want_units)
    with pytest.raises(mic.MicError) as e:
        mic.mic2_multi_crop_plan(files, xyzv, 17, 5, 3, cap=nu - 1)
    assert e.value.code == mic.MIC_ERR_CAPACITY and e.value.nframes == nu and e.value.pieces == want_pieces
    assert e.value.file_status.tolist() == [0, 0, 0]
    units, pieces, fs = mic.mic2_multi_crop_plan(files, xyzv, 17, 5, 3, cap=nu)
    assert [tuple(u) for u in units.tolist()] == want_units and pieces == want_pieces
    # the arrays are left alone when they are too short, the counts and the codes are set
    arrs, ptrs, lens = mic._volume_table(files + [b"garbage"])
    a = np.asarray(xyzv + [(0, 0, 0, 3)], dtype=np.int32)
    vo, fo = np.full(4, 77, dtype=np.uint32), np.full(4, 77, dtype=np.uint32)
    fs = np.full(4, 9, dtype=np.int32)
    nf, npc = C.c_uint64(0), C.c_uint64(0)
    rc = mic.lib().mic_hip_mic2_multi_crop_plan(ptrs.ctypes.data, lens.ctypes.data, 4, a.ctypes.data, len(a), 17, 5, 3,
                                                vo.ctypes.data, fo.ctypes.data, 4, C.byref(nf), C.byref(npc), fs.ctypes.data)
    assert rc == mic.MIC_ERR_CAPACITY and (vo == 77).all() and (fo == 77).all()
    assert (nf.value, npc.value) == (nu, want_pieces) and fs.tolist() == [0, 0, 0, mic.MIC_ERR_CORRUPT]


def test_argument_errors(mic):
    files = _files(DIMS[:2])
    arrs, ptrs, lens = mic._volume_table(files)
    a = np.asarray([(0, 0, 0, 0), (0, 0, 0, 1)], dtype=np.int32)
    vo, fo = np.zeros(16, dtype=np.uint32), np.zeros(16, dtype=np.uint32)
    nf, npc = C.c_uint64(0), C.c_uint64(0)

    def call(files=ptrs.ctypes.data, lens=lens.ctypes.data, nfiles=2, xyzv=a.ctypes.data, n=2, cw=8, ch=8, cd=2, vo=vo.ctypes.data, fo=fo.ctypes.data, cap=16):
        return mic.lib().mic_hip_mic2_multi_crop_plan(files, lens, nfiles, xyzv, n, cw, ch, cd, vo, fo, cap, C.byref(nf), C.byref(npc), None)
    assert call() == mic.MIC_OK and (nf.value, npc.value) == (4, 4)
    for kw in (dict(cw=0), dict(ch=0), dict(cd=0), dict(cd=-1), dict(n=-1), dict(nfiles=-1), dict(xyzv=None), dict(files=None), dict(lens=None),
               dict(vo=None), dict(fo=None)):
        assert call(**kw) == mic.MIC_ERR_ARGS, kw
    assert call(xyzv=None, n=0) == mic.MIC_OK and (nf.value, npc.value) == (0, 0)
    assert call(vo=None, fo=None, cap=0) == mic.MIC_ERR_CAPACITY and (nf.value, npc.value) == (4, 4)   # counting only
    for v in (-1, 2, 1 << 20):                                            # a volume index outside the list
        b = np.asarray([(0, 0, 0, 0), (0, 0, 0, v)], dtype=np.int32)
        assert call(xyzv=b.ctypes.data) == mic.MIC_ERR_ARGS, v
        with pytest.raises(mic.MicError) as e:
            mic.mic2_multi_crop_plan(files, b, 8, 8, 2)
        assert e.value.code == mic.MIC_ERR_ARGS
    assert call(nfiles=1) == mic.MIC_ERR_ARGS                             # ... the second crop's volume is outside a list of one
