"""mic_hip_rgb_crop_plan (csrc/mic_rgb_crops.hip), the host planner behind the RGB file crop calls, against a plan made by clipping
every crop against its image in numpy and reading the plane modes out of the blobs.  The files come from the CPU oracle
(mico.wsi_compress_tile / mico.micr_write) and two are assembled by hand (rgb_crop_files.py); no device is needed.  The codes of
refused files are the ones mic_hip_rgb_decompress_batch gives the same files (tests/test_gpu_rgb_batch.py,
test_a_job_fails_alone_on_decode; the GPU test asks that door itself)."""
import ctypes as C

import numpy as np
import pytest

import rgb_crop_files as F


@pytest.fixture(scope="module")
def files(synth, mico):
    return F.build(synth, mico)


def _plan(mic, files, xyf, cw, ch, **kw):
    file_of, planes, pieces, fs = mic.rgb_crop_plan([f for _, f, _ in files], xyf, cw, ch, **kw)
    return file_of.tolist(), planes, pieces, fs.tolist()


def test_the_five_calls_are_exported(mic):
    L = C.CDLL(mic.LIB_PATH)
    for name in ("mic_hip_rgb_crop_plan", "mic_hip_rgb_read_crops", "mic_hip_session_rgb_read_crops",
                 "mic_hip_rgb_read_crops_as", "mic_hip_session_rgb_read_crops_as"):
        assert hasattr(L, name) and name in mic.ABI_SYMBOLS, name
    assert C.sizeof(mic.RgbFile) == 32 and C.sizeof(mic.RgbCropStats) == 32


def test_the_fixture_files_are_what_the_table_says(files):
    assert len(files) == len(F.WANT_MODES)
    for (im, f, m), want in zip(files, F.WANT_MODES):
        if want is not None:
            assert m == want
    assert 2 in files[8][2][1:]                                              # the frame with the colour box has a coded chroma plane
    assert isinstance(files[5][1], bytes) and files[5][1][:4] == b"MICR" and isinstance(files[9][1], tuple)
    # raw planes at odd and at even byte addresses of their blob: Y at 12 + 1, Co at 12 + (1 + 2 npx) + 1
    assert len(files[10][1][0]) == 12 + 3 * (1 + 2 * F.W70 * F.H33)


@pytest.mark.parametrize("shape", F.SHAPES)
def test_plan_equals_the_enumerated_one(mic, files, shape):
    cw, ch = shape
    xyf = F.origins(files, cw, ch, skip=(2, 6))
    file_of, planes, pieces, fs = _plan(mic, files, xyf, cw, ch)
    want = F.brute_plan(files, xyf, cw, ch)
    assert (file_of, planes, pieces) == want and pieces > 0                  # ascending, each once
    assert 2 not in file_of and 6 not in file_of and fs == [0] * len(files)
    assert file_of == sorted(set(file_of))
    for o in xyf:                                                            # ... and crop by crop
        assert _plan(mic, files, [o], cw, ch)[:3] == F.brute_plan(files, [o], cw, ch), o
    assert _plan(mic, files, xyf[::-1], cw, ch)[:3] == want                  # file order, not crop order


def test_outside_touching_duplicates_and_nothing(mic, files):
    im = files[7][0]
    h, w = im.shape[:2]
    cw, ch = 32, 16
    assert _plan(mic, files, [], cw, ch)[:3] == ([], 0, 0)                   # n = 0
    for o in [(500, 500, 7), (-500, -500, 7), (-cw, 0, 7), (0, h, 7), (w, 0, 7), (0, -ch, 7)]:
        assert _plan(mic, files, [o], cw, ch) == ([], 0, 0, [0] * len(files)), o     # no piece, and the file is not named
    assert _plan(mic, files, [(-cw + 1, 0, 7)], cw, ch)[:3] == ([7], 3, 1)   # one column
    assert _plan(mic, files, [(0, h - 1, 7)], cw, ch)[:3] == ([7], 3, 1)     # one row
    assert _plan(mic, files, [(3, 3, 9)] * 3, cw, ch)[:3] == ([9], 1, 3)     # duplicates: the file once, every piece counted; modes [2, 0, 0]
    assert _plan(mic, files, [(0, 0, 9), (0, 0, 0), (0, 0, 4), (0, 0, 11)], cw, ch)[:3] == ([0, 4, 9, 11], 3, 4)
    assert _plan(mic, files, [(0, 0, 10), (-1, -1, 3)], 300, 40)[:3] == ([3, 10], 0, 2)   # raw planes only: nothing to entropy-decode


def _status_with(mic, files, f, entry, xyf=None):
    fl = [e for _, e, _ in files]
    fl[f] = entry
    xyf = [(0, 0, k) for k in range(len(files))] if xyf is None else xyf
    file_of, planes, pieces, fs = mic.rgb_crop_plan(fl, xyf, 8, 8)
    return file_of.tolist(), fs.tolist()


def test_a_refused_file_sets_its_own_status_only(mic, mico, files):
    nf = len(files)
    everyone = list(range(nf))

    def want(f, code):
        st = [0] * nf
        st[f] = code
        return [k for k in everyone if k != f], st
    fa = files[7][1][0]                                                      # a blob of three coded planes
    w, h = files[7][1][1:3]
    ma = files[5][1]                                                         # a MICR file
    assert _status_with(mic, files, 7, (fa, w, h)) == (everyone, [0] * nf)
    assert _status_with(mic, files, 7, (None, w, h)) == want(7, mic.MIC_ERR_ARGS)                 # NULL data
    assert _status_with(mic, files, 7, (fa, 0, h)) == want(7, mic.MIC_ERR_ARGS)                   # width 0
    assert _status_with(mic, files, 7, (fa, w, -1)) == want(7, mic.MIC_ERR_ARGS)
    assert _status_with(mic, files, 7, (fa, w, h, 2)) == want(7, mic.MIC_ERR_ARGS)                # neither blob nor MICR
    assert _status_with(mic, files, 7, (fa, 1 << 14, 1 << 13)) == want(7, mic.MIC_ERR_UNSUPPORTED)   # 2^27 pixels
    assert _status_with(mic, files, 7, (fa[:-1], w, h)) == want(7, mic.MIC_ERR_CORRUPT)           # cut by one byte: the lengths reach past the blob
    long_co = fa[:4] + (int.from_bytes(fa[4:8], "little") + len(fa)).to_bytes(4, "little") + fa[8:]
    assert _status_with(mic, files, 7, (long_co, w, h)) == want(7, mic.MIC_ERR_CORRUPT)           # the Co length pushed past the blob
    assert _status_with(mic, files, 7, (fa[:11], w, h)) == want(7, mic.MIC_ERR_CORRUPT)
    l0 = int.from_bytes(fa[0:4], "little")
    bad_mode = bytearray(fa); bad_mode[12 + l0] = 4
    assert _status_with(mic, files, 7, (bytes(bad_mode), w, h)) == want(7, mic.MIC_ERR_CORRUPT)   # "unknown plane mode"
    assert _status_with(mic, files, 5, b"MICX" + ma[4:]) == want(5, mic.MIC_ERR_CORRUPT)
    assert _status_with(mic, files, 5, ma[:11]) == want(5, mic.MIC_ERR_CORRUPT)
    assert _status_with(mic, files, 5, (ma, 64, 64, 1)) == (everyone, [0] * nf)                   # dims that agree with the header
    assert _status_with(mic, files, 5, (ma, 66, 64, 1)) == want(5, mic.MIC_ERR_ARGS)              # ... and that disagree
    assert _status_with(mic, files, 5, (ma, 0, 64, 1)) == want(5, mic.MIC_ERR_ARGS)
    # a raw plane needs 2 * w * h bytes: the hand-made blob under a larger size
    assert _status_with(mic, files, 10, (files[10][1][0], F.W70 + 1, F.H33)) == want(10, mic.MIC_ERR_CORRUPT)
    # a file no crop names is not looked at: by index, or because its crops lie outside the image it states
    others = [(0, 0, k) for k in everyone if k != 7]
    assert _status_with(mic, files, 7, (fa[:-1], w, h), xyf=others) == want(7, 0)
    assert _status_with(mic, files, 7, (fa[:-1], w, h), xyf=others + [(w, 0, 7), (0, h, 7), (-8, 0, 7)]) == want(7, 0)
    assert _status_with(mic, files, 7, (None, w, h), xyf=others) == want(7, 0)


def test_a_short_file_list_is_a_capacity_error_with_the_counts(mic, files):
    xyf = [(0, 0, 9), (5, 5, 7), (0, 20, 9), (0, 0, 4)]
    with pytest.raises(mic.MicError) as e:
        mic.rgb_crop_plan([f for _, f, _ in files], xyf, 17, 12, cap=2)
    assert e.value.code == mic.MIC_ERR_CAPACITY and (e.value.nfiles, e.value.planes_coded, e.value.pieces) == (3, 4, 4)
    assert e.value.file_status.tolist() == [0] * len(files)
    assert _plan(mic, files, xyf, 17, 12, cap=3)[:3] == ([4, 7, 9], 4, 4)
    # the list is left alone when it is too short
    tab, keep = mic.rgb_files([f for _, f, _ in files])
    a = np.asarray(xyf, dtype=np.int32)
    fo = np.full(4, 77, dtype=np.uint32)
    nf, npl, npc = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    fs = np.full(len(files), 9, dtype=np.int32)
    rc = mic.lib().mic_hip_rgb_crop_plan(tab, len(files), a.ctypes.data, len(xyf), 17, 12, fo.ctypes.data, 2,
                                         C.byref(nf), C.byref(npl), C.byref(npc), fs.ctypes.data)
    assert rc == mic.MIC_ERR_CAPACITY and (fo == 77).all() and (nf.value, npl.value, npc.value) == (3, 4, 4)
    assert fs.tolist() == [0] * len(files)


def test_argument_errors(mic, files):
    tab, keep = mic.rgb_files([f for _, f, _ in files])
    a = np.asarray([(0, 0, 0)], dtype=np.int32)
    fo = np.zeros(16, dtype=np.uint32)
    nf, npl, npc = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)

    def call(files_=tab, nfiles=len(files), xyf=a.ctypes.data, n=1, cw=8, ch=8, file_of=fo.ctypes.data, cap=16):
        return mic.lib().mic_hip_rgb_crop_plan(files_, nfiles, xyf, n, cw, ch, file_of, cap, C.byref(nf), C.byref(npl), C.byref(npc), None)
    assert call() == mic.MIC_OK and (nf.value, npl.value, npc.value) == (1, 0, 1)
    for kw in (dict(cw=0), dict(ch=0), dict(cw=-4), dict(n=-1), dict(nfiles=-1), dict(xyf=None), dict(files_=None), dict(file_of=None)):
        assert call(**kw) == mic.MIC_ERR_ARGS, kw
    for f in (-1, len(files)):                                               # a file index outside the list
        b = np.asarray([(0, 0, f)], dtype=np.int32)
        assert call(xyf=b.ctypes.data) == mic.MIC_ERR_ARGS, f
    assert call(xyf=None, n=0) == mic.MIC_OK and (nf.value, npl.value, npc.value) == (0, 0, 0)
    assert call(files_=None, nfiles=0, xyf=None, n=0) == mic.MIC_OK
    assert call(file_of=None, cap=0) == mic.MIC_ERR_CAPACITY and (nf.value, npl.value, npc.value) == (1, 0, 1)   # counting only
    assert mic.lib().mic_hip_rgb_crop_plan(tab, len(files), a.ctypes.data, 1, 8, 8, fo.ctypes.data, 16, None, None, None, None) == mic.MIC_OK
