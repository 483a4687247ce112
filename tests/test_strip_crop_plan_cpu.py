"""mic_hip_strips_crop_plan (csrc/mic_strip_crops.hip), the host planner behind the strip-file crop calls, against a plan made by
enumerating every crop's coordinates against every strip's rows in numpy.  The files come from the CPU oracle's PICS and PICA
encoders; no device is needed."""
import ctypes as C
import struct

import numpy as np
import pytest

import strip_crop_files as F


@pytest.fixture(scope="module")
def files(synth, mico):
    return F.build(synth, *F.oracle_encoders(mico))


def _plan(mic, files, xyf, cw, ch, **kw):
    units, pieces, fs = mic.strips_crop_plan([d for _, _, d in files], xyf, cw, ch, **kw)
    return [tuple(int(v) for v in u) for u in units], pieces, fs.tolist()


def test_the_three_calls_are_exported(mic):
    L = C.CDLL(mic.LIB_PATH)
    for name in ("mic_hip_strips_crop_plan", "mic_hip_strips_read_crops", "mic_hip_session_strips_read_crops"):
        assert hasattr(L, name) and name in mic.ABI_SYMBOLS, name


def test_the_fixture_files_are_what_the_table_says(files):
    for name, img, data in files:
        w, h, maxv, kind, strips, states = F.FILES[name]
        m = F.StripFile(data)
        assert (m.kind, m.w, m.h, m.n) == (kind, w, h, strips) and img.shape == (h, w), name
    a = F.StripFile(files[0][2])
    assert [a.rows(k)[1] - a.rows(k)[0] for k in range(8)] == [9] * 7 + [7]
    b = files[1][1]
    assert b.min() < 32768 < b.max()
    c = F.StripFile(files[2][2])
    kept = [c.grad(k) for k in range(c.n)]
    assert any(kept) and not all(kept), kept                              # both predictors
    assert len({c.rows(k)[1] - c.rows(k)[0] for k in range(c.n)}) > 2     # uneven boundaries


@pytest.mark.parametrize("shape", F.SHAPES)
def test_plan_equals_the_enumerated_one(mic, files, shape):
    cw, ch = shape
    xyf = F.origins(files, cw, ch)
    units, pieces, fs = _plan(mic, files, xyf, cw, ch)
    want_units, want_pieces, _ = F.brute_plan(files, xyf, cw, ch)
    assert units == want_units and pieces == want_pieces and pieces > 0   # ascending by file, then strip, each once
    assert fs == [0] * len(files)
    for o in xyf:                                                         # ... and crop by crop
        u1, p1, _ = _plan(mic, files, [o], cw, ch)
        assert (u1, p1) == F.brute_plan(files, [o], cw, ch)[:2], o


def test_seams_outside_duplicates_and_nothing(mic, files):
    a = F.StripFile(files[0][2])                                          # strips of 9 rows
    assert _plan(mic, files, [], 32, 16)[:2] == ([], 0)                   # n = 0
    assert _plan(mic, files, [(5, 8, 0)], 10, 2)[:2] == ([(0, 0), (0, 1)], 2)       # rows 8 and 9: on the seam, both strips
    assert _plan(mic, files, [(5, 9, 0)], 10, 9)[:2] == ([(0, 1)], 1)               # exactly strip 1
    assert _plan(mic, files, [(5, 9, 0)], 10, 10)[:2] == ([(0, 1), (0, 2)], 2)
    for o in [(a.w, 0, 0), (-32, 0, 0), (0, a.h, 0), (0, -16, 0), (500, 500, 0), (-500, -500, 0)]:
        assert _plan(mic, files, [o], 32, 16)[:2] == ([], 0), o           # wholly outside: nothing to decode
    assert _plan(mic, files, [(0, 0, 0)], a.w, a.h)[:2] == ([(0, k) for k in range(8)], 8)
    assert _plan(mic, files, [(-1, -1, 0)], a.w + 2, a.h + 2)[:2] == ([(0, k) for k in range(8)], 8)
    assert _plan(mic, files, [(a.w - 1, a.h - 1, 0)], 5, 5)[:2] == ([(0, 7)], 1)
    assert _plan(mic, files, [(3, 3, 0)] * 3, 17, 10)[:2] == ([(0, 0), (0, 1)], 6)  # duplicates: each strip once, every piece counted
    assert _plan(mic, files, [(0, 0, 4), (0, 60, 0), (0, 0, 2)], 8, 8)[:2] == ([(0, 6), (0, 7), (2, 0), (4, 0)], 4)   # file order, not crop order
    c = F.StripFile(files[2][2])                                          # PICA: the boundaries are the table's
    y1 = c.rows(0)[1]
    assert _plan(mic, files, [(0, y1 - 1, 2)], 4, 2)[:2] == ([(2, 0), (2, 1)], 2)
    assert _plan(mic, files, [(0, y1, 2)], 4, 1)[:2] == ([(2, 1)], 1)


def test_a_bad_header_sets_the_files_status_only(mic, files):
    datas = [d for _, _, d in files]
    xyf = [(0, 0, f) for f in range(len(files))]
    good, _, _ = _plan(mic, files, xyf, 8, 8)

    def plan_with(f, data):
        ds = list(datas)
        ds[f] = data
        units, pieces, fs = mic.strips_crop_plan(ds, xyf, 8, 8)
        return [tuple(int(v) for v in u) for u in units], fs.tolist()
    b = F.StripFile(datas[1])
    bad = bytearray(datas[1]); bad[:4] = b"PICX"                          # not a strip file
    want = [u for u in good if u[0] != 1]
    assert plan_with(1, bytes(bad)) == (want, [0, mic.MIC_ERR_CORRUPT, 0, 0, 0])
    assert plan_with(1, datas[1][:10]) == (want, [0, mic.MIC_ERR_CORRUPT, 0, 0, 0])           # a truncated header
    bad = bytearray(datas[1]); struct.pack_into("<I", bad, b.entry_at(3), len(datas[1]))      # strip 3 points outside the file
    assert plan_with(1, bytes(bad)) == (want, [0, mic.MIC_ERR_CORRUPT, 0, 0, 0])              # (a strip no crop needs: the file fails whole)
    bad = bytearray(datas[1]); struct.pack_into("<I", bad, b.entry_at(2) + 4, 0)              # length 0
    assert plan_with(1, bytes(bad)) == (want, [0, mic.MIC_ERR_CORRUPT, 0, 0, 0])
    c = F.StripFile(datas[2])
    bad = bytearray(datas[2]); struct.pack_into("<I", bad, c.entry_at(2), c.rows(3)[0])       # PICA: an empty row range
    want = [u for u in good if u[0] != 2]
    assert plan_with(2, bytes(bad)) == (want, [0, 0, mic.MIC_ERR_CORRUPT, 0, 0])
    # a file no crop names is not looked at
    bad = bytearray(datas[1]); bad[:4] = b"PICX"
    units, pieces, fs = mic.strips_crop_plan([datas[0], bytes(bad)], [(0, 0, 0)], 8, 8)
    assert fs.tolist() == [0, 0] and units.tolist() == [[0, 0]]


def test_a_short_unit_list_is_a_capacity_error_with_the_counts(mic, files):
    datas = [d for _, _, d in files]
    xyf = [(0, 0, 0), (5, 5, 1), (0, 20, 0)]                              # A: strips 0, 1 and 2, 3; B: strips 0, 1
    with pytest.raises(mic.MicError) as e:
        mic.strips_crop_plan(datas, xyf, 17, 12, cap=5)
    assert e.value.code == mic.MIC_ERR_CAPACITY and e.value.nstrips == 6 and e.value.pieces == 6
    units, pieces, _ = mic.strips_crop_plan(datas, xyf, 17, 12, cap=6)
    assert units.tolist() == [[0, 0], [0, 1], [0, 2], [0, 3], [1, 0], [1, 1]] and pieces == 6
    # the lists are left alone when they are too short
    arrs = [np.frombuffer(d, dtype=np.uint8) for d in datas]
    ptrs = np.asarray([a.ctypes.data for a in arrs], dtype=np.uintp)
    lens = np.asarray([a.size for a in arrs], dtype=np.uintp)
    a = np.asarray(xyf, dtype=np.int32)
    fo, so = np.full(4, 77, dtype=np.uint32), np.full(4, 78, dtype=np.uint32)
    ns, npc = C.c_uint64(0), C.c_uint64(0)
    fs = np.full(len(datas), 9, dtype=np.int32)
    rc = mic.lib().mic_hip_strips_crop_plan(ptrs.ctypes.data, lens.ctypes.data, len(datas), a.ctypes.data, 3, 17, 12,
                                            fo.ctypes.data, so.ctypes.data, 4, C.byref(ns), C.byref(npc), fs.ctypes.data)
    assert rc == mic.MIC_ERR_CAPACITY and (fo == 77).all() and (so == 78).all() and (ns.value, npc.value) == (6, 6)
    assert fs.tolist() == [0] * len(datas)


def test_argument_errors(mic, files):
    datas = [d for _, _, d in files]
    arrs = [np.frombuffer(d, dtype=np.uint8) for d in datas]
    ptrs = np.asarray([a.ctypes.data for a in arrs], dtype=np.uintp)
    lens = np.asarray([a.size for a in arrs], dtype=np.uintp)
    a = np.asarray([(0, 0, 0)], dtype=np.int32)
    fo, so = np.zeros(16, dtype=np.uint32), np.zeros(16, dtype=np.uint32)
    ns, npc = C.c_uint64(0), C.c_uint64(0)

    def call(files_=ptrs.ctypes.data, lens_=lens.ctypes.data, nfiles=len(datas), xyf=a.ctypes.data, n=1, cw=8, ch=8,
             file_of=fo.ctypes.data, strip_of=so.ctypes.data, cap=16):
        return mic.lib().mic_hip_strips_crop_plan(files_, lens_, nfiles, xyf, n, cw, ch, file_of, strip_of, cap, C.byref(ns), C.byref(npc), None)
    assert call() == mic.MIC_OK and (ns.value, npc.value) == (1, 1)
    for kw in (dict(cw=0), dict(ch=0), dict(cw=-4), dict(n=-1), dict(nfiles=-1), dict(xyf=None), dict(files_=None), dict(lens_=None),
               dict(file_of=None), dict(strip_of=None)):
        assert call(**kw) == mic.MIC_ERR_ARGS, kw
    for f in (-1, len(datas)):                                            # a file index outside the list
        b = np.asarray([(0, 0, f)], dtype=np.int32)
        assert call(xyf=b.ctypes.data) == mic.MIC_ERR_ARGS, f
    assert call(xyf=None, n=0) == mic.MIC_OK and (ns.value, npc.value) == (0, 0)
    assert call(file_of=None, strip_of=None, cap=0) == mic.MIC_ERR_CAPACITY and (ns.value, npc.value) == (1, 1)   # counting only
    assert mic.strips_head(datas[0]) == F.StripFile(datas[0]).head() and mic.strips_head(datas[2]) == F.StripFile(datas[2]).head()
