"""Many 3-D crops per call into a device tensor (csrc/mic_mic2_crops.hip: mic_hip_mic2_read_crops, mic_hip_mic2_reader_read_crops,
mic_hip_session_mic2_read_crops).  The codec is lossless, so the expected value of every crop is the stack of the existing
decompress_multi_frame (pinned to the oracle by test_gpu_parity.py, and compared with the source here), padded with zeros and
cropped in numpy (mic2_crop_volumes.expected)."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import mic2_crop_volumes as V

pytestmark = pytest.mark.gpu

VOLUMES = ["xr12", "wrap16"]


@pytest.fixture(scope="module")
def volumes(mic, synth, gpu_ready):
    """name -> dict(vol, files = {temporal: bytes}); each file decoded once and compared with its source, never written to"""
    out = {}
    for name, make in (("xr12", V.volume_12bit), ("wrap16", V.volume_16bit)):
        vol, maxv = make(synth)
        n, h, w = vol.shape
        files = {}
        for temporal in (False, True):
            data = mic.compress_multi_frame(vol, w, h, maxv, temporal=temporal)
            assert np.array_equal(mic.decompress_multi_frame(data), vol)
            files[temporal] = data
        vol.setflags(write=False)
        out[name] = dict(vol=vol, files=files)
    d = out["wrap16"]["vol"].astype(np.int32)
    assert (np.abs(d[1:] - d[:-1]) > 32768).any()                        # some inter-frame differences do wrap mod 2^16
    return out


def _tensor(n, cd, ch, cw):
    import torch
    return torch.full((max(n, 1), cd, ch, cw, 2), 0xA5, dtype=torch.uint8, device="cuda")   # (every byte must be overwritten)


def _read(call, xyz, cw, ch, cd):
    """call(xyz, cw, ch, cd, d_out, out_cap) -> (status, stats); the crops as (n, cd, ch, cw) u16"""
    t = _tensor(len(xyz), cd, ch, cw)
    st, stats = call(xyz, cw, ch, cd, t.data_ptr(), len(xyz) * cd * ch * cw * 2)
    return t.cpu().numpy()[: len(xyz)].view("<u2")[..., 0], st, stats


class _Doors:
    """the three entry points on one file: .file, .reader, .session, each call(xyz, cw, ch, cd, d_out, out_cap)"""

    def __init__(self, mic, data):
        import torch
        self.mic, self.data = mic, data
        m = V.Mic2File(data)
        self.rd = mic.Mic2Reader(data)
        self.sess = mic.Session(4, m.w * m.h)
        self.d_file = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
        head = m.head()
        self.file = lambda xyz, cw, ch, cd, d, cap: mic.mic2_read_crops(data, xyz, cw, ch, cd, d, cap)
        self.reader = lambda xyz, cw, ch, cd, d, cap: self.rd.read_crops(xyz, cw, ch, cd, d, cap)
        self.session = lambda xyz, cw, ch, cd, d, cap: self.sess.mic2_read_crops(head, self.d_file.data_ptr(), len(data), xyz, cw, ch, cd, d, cap)
        self.all = [("file", self.file), ("reader", self.reader), ("session", self.session)]

    def close(self):
        self.rd.close()
        self.sess.close()


@pytest.mark.parametrize("temporal", [False, True])
@pytest.mark.parametrize("name", VOLUMES)
def test_crops_equal_the_padded_volume(mic, volumes, name, temporal):
    vol, data = volumes[name]["vol"], volumes[name]["files"][temporal]
    n, h, w = vol.shape
    doors = _Doors(mic, data)
    try:
        for cw, ch, cd in V.SHAPES:
            xyz = V.origins(w, h, n, cw, ch, cd)
            want = V.expected(vol, xyz, cw, ch, cd)
            frames, pieces = mic.mic2_crop_plan(w, h, n, temporal, xyz, cw, ch, cd)
            for door, call in doors.all:
                got, st, stats = _read(call, xyz, cw, ch, cd)
                for i in range(len(xyz)):
                    assert np.array_equal(got[i], want[i]), (door, (cw, ch, cd), xyz[i])
                assert (st == mic.MIC_OK).all(), (door, st)
                assert stats["frames_decoded"] == frames.size and stats["pieces"] == pieces and stats["slabs"] >= 1, (door, stats)
        outside = [(w, 0, 0), (0, h + 3, 0), (0, 0, n), (0, 0, -3), (-48, 0, 1)]
        for door, call in doors.all:
            got, st, stats = _read(call, outside, 48, 40, 3)
            assert not got.any() and (st == 0).all() and stats == dict(frames_decoded=0, pieces=0, slabs=0), door
    finally:
        doors.close()


@pytest.mark.parametrize("temporal", [False, True])
def test_the_reader_pulls_the_plans_blobs_only(mic, volumes, temporal):
    vol, data = volumes["xr12"]["vol"], volumes["xr12"]["files"][temporal]
    n, h, w = vol.shape
    m = V.Mic2File(data)
    xyz = [(10, 5, 1), (60, 20, 2), (100, 30, 7), (-4, 40, 7), (w, 0, 9)]    # frames 1 .. 4 and 7 .. 9 (the last crop: outside)
    cw, ch, cd = 48, 40, 3
    src = V.RecordingSource(data)
    with mic.Mic2Reader(src, len(data)) as rd:
        src.reads.clear()
        got, st, stats = _read(lambda *a: rd.read_crops(*a), xyz, cw, ch, cd)
    assert np.array_equal(got, V.expected(vol, xyz, cw, ch, cd)) and (st == 0).all()
    frames, _ = mic.mic2_crop_plan(w, h, n, temporal, xyz, cw, ch, cd)
    assert frames.tolist() == (list(range(10)) if temporal else [1, 2, 3, 4, 7, 8, 9])
    want = np.zeros(len(data), dtype=np.int32)
    for f in frames:
        b, e = m.span(int(f))
        want[b:e] += 1
    assert want.max() == 1 and np.array_equal(src.coverage(), want)          # exactly those streams, each byte once
    assert max(off + ln for off, ln in src.reads) == m.span(9)[1] < len(data)   # nothing behind the last needed frame
    assert len(src.reads) == (1 if temporal else 2)                           # neighbours in the file in one read


@pytest.mark.parametrize("temporal", [False, True])
def test_pinned_host_output(mic, volumes, temporal):
    vol, data = volumes["xr12"]["vol"], volumes["xr12"]["files"][temporal]
    n, h, w = vol.shape
    a = 4
    buf = mic.host_alloc(3 * h * w * 2)
    try:
        buf[:] = 0xA5
        st, stats = mic.mic2_read_crops(data, [(0, 0, a)], w, h, 3, buf.ctypes.data, buf.size)
        assert (st == 0).all() and stats["pieces"] == 3
        assert np.array_equal(buf.view("<u2").reshape(3, h, w), vol[a: a + 3])
    finally:
        mic.host_free(buf)


def _frame_code(mic, m, data, temporal):
    """(code, volume) the existing decoders give for the damaged file: the unit codec's code of frame 5, and -- should the damaged
    stream still decode -- the pixels it decodes to"""
    if temporal:
        try:
            return mic.MIC_OK, np.asarray(mic.decompress_multi_frame(data)).reshape(m.n, m.h, m.w)
        except mic.MicError as e:
            return e.code, None
    b, e = m.span(5)
    (code, px), = mic.decompress_batch([bytes(data[b:e])], [(m.w, m.h)])
    return code, px


@pytest.mark.parametrize("temporal", [False, True])
def test_a_damaged_frame_fails_its_dependants_only(mic, volumes, temporal):
    vol = volumes["xr12"]["vol"]
    n, h, w = vol.shape
    m = V.Mic2File(volumes["xr12"]["files"][temporal])
    b, e = m.span(5)
    m.data[(b + e) // 2] ^= 0x5A
    data = bytes(m.data)
    code, px = _frame_code(mic, m, data, temporal)
    want_vol = vol
    if code == mic.MIC_OK:                                                # the flipped stream still decodes: to these pixels
        want_vol = vol.copy()
        if temporal:
            want_vol = px
        else:
            want_vol[5] = np.asarray(px).reshape(h, w)
    cw, ch, cd = 48, 40, 3
    xyz = V.origins(w, h, n, cw, ch, cd) + [(5, 5, 5), (60, 10, 6), (60, 10, 8)]
    want = V.expected(want_vol, xyz, cw, ch, cd)
    doors = _Doors(mic, data)
    try:
        for door, call in doors.all:
            got, st, stats = _read(call, xyz, cw, ch, cd)
            hit = 0
            for i, o in enumerate(xyz):
                frames, pieces = V.brute_plan(w, h, n, False, [o], cw, ch, cd)
                depends = bool(pieces) and (max(frames) >= 5 if temporal else 5 in frames)
                hit += depends
                assert st[i] == (code if depends else mic.MIC_OK), (door, o, st[i])
                if not depends or code == mic.MIC_OK:
                    assert np.array_equal(got[i], want[i]), (door, o)
            assert 0 < hit < len(xyz)
    finally:
        doors.close()
    # a table entry of a needed frame with length 0 fails the call, as decompress_multi_frame does; a call that does not need it runs
    m = V.Mic2File(volumes["xr12"]["files"][temporal])
    struct.pack_into("<I", m.data, 20 + 8 * 5 + 4, 0)
    data = bytes(m.data)
    with pytest.raises(mic.MicError) as e:
        mic.decompress_multi_frame(data)
    assert e.value.code == mic.MIC_ERR_CORRUPT
    doors = _Doors(mic, data)
    try:
        for door, call in doors.all:
            with pytest.raises(mic.MicError) as e:
                _read(call, [(0, 0, 4)], cw, ch, cd)
            assert e.value.code == mic.MIC_ERR_CORRUPT, door
            got, st, stats = _read(call, [(0, 0, 2)], cw, ch, cd)
            assert (st == 0).all() and np.array_equal(got, V.expected(vol, [(0, 0, 2)], cw, ch, cd)), door
    finally:
        doors.close()


def test_argument_errors_come_back_before_any_launch(mic, volumes):
    import torch
    vol, data = volumes["xr12"]["vol"], volumes["xr12"]["files"][False]
    n, h, w = vol.shape
    cw, ch, cd = 48, 40, 3
    xyz = [(0, 0, 0), (10, 10, 2)]
    t = _tensor(2, cd, ch, cw)
    cap = 2 * cd * ch * cw * 2
    pageable = np.zeros(cap, dtype=np.uint8)
    many = [(0, 0, 0)] * 64                                               # 64 whole volumes: 14.8 MB, far past the allocation t lies in
    doors = _Doors(mic, data)
    a = np.asarray(xyz, dtype=np.int32)
    st2 = np.zeros(2, dtype=np.int32)
    head = V.Mic2File(data).head()
    raw = [lambda nn: mic.lib().mic_hip_mic2_read_crops(data, len(data), a.ctypes.data, nn, cw, ch, cd, t.data_ptr(), cap, st2.ctypes.data, None),
           lambda nn: mic.lib().mic_hip_mic2_reader_read_crops(doors.rd._h, a.ctypes.data, nn, cw, ch, cd, t.data_ptr(), cap, st2.ctypes.data, None),
           lambda nn: mic.lib().mic_hip_session_mic2_read_crops(doors.sess._h, head, len(head), doors.d_file.data_ptr(), len(data), a.ctypes.data, nn,
                                                                cw, ch, cd, t.data_ptr(), cap, st2.ctypes.data, None)]
    try:
        for (door, call), raw_call in zip(doors.all, raw):
            for args, want in [((xyz, 0, ch, cd, t.data_ptr(), cap), mic.MIC_ERR_ARGS), ((xyz, cw, 0, cd, t.data_ptr(), cap), mic.MIC_ERR_ARGS),
                               ((xyz, cw, ch, -1, t.data_ptr(), cap), mic.MIC_ERR_ARGS), ((xyz, cw, ch, cd, t.data_ptr(), cap - 1), mic.MIC_ERR_CAPACITY),
                               ((xyz, cw, ch, cd, pageable.ctypes.data, cap), mic.MIC_ERR_ARGS),
                               ((many, w, h, n, t.data_ptr(), 64 * n * h * w * 2), mic.MIC_ERR_ARGS)]:
                with pytest.raises(mic.MicError) as e:
                    call(*args)
                assert e.value.code == want, (door, args)
            assert raw_call(-1) == mic.MIC_ERR_ARGS, door                 # n = -1
            assert raw_call(2) == mic.MIC_OK, door                        # (the same call with n = 2 is a good one)
            assert np.array_equal(t.cpu().numpy().view("<u2")[..., 0], V.expected(vol, xyz, cw, ch, cd)), door
            t.fill_(0xA5)
            st, stats = call([], cw, ch, cd, t.data_ptr(), 0)             # n = 0: nothing to do, and that is no error
            assert st.size == 0 and stats == dict(frames_decoded=0, pieces=0, slabs=0)
            assert (t.cpu().numpy() == 0xA5).all() and not pageable.any()  # none of the refused calls wrote a byte
    finally:
        doors.close()


def test_the_gather_kernel_is_timed_under_its_name(mic, volumes):
    doors = _Doors(mic, volumes["xr12"]["files"][False])
    try:
        doors.sess.set_timing(True)
        _read(doors.session, [(0, 0, 0), (5, 5, 3)], 48, 40, 3)
        assert "k_mic2_gather_crops" in dict(doors.sess.last_timings())
    finally:
        doors.close()


def test_sub_batch_seams_under_a_small_workspace():
    """tests/mic2_crops_chunking_check.py in a fresh process with a 7 MiB workspace ceiling.  A sub-batch holds
    budget / (unit_ws_bytes(npx) + 2 npx) frames (mic2_batch_cuts over frames of one size); for 150 x 70 = 10500 pixels the tier-2 slabs
    of a unit are 4 * 42016 (tokens, symbols) + 215136 (blob) + 8 * 21008 (segments) + 1312 (flags) + 26 * 65536 (tables) + 8192 = 2264704 bytes,
    with the frame 2285704: 7 MiB = 7340032 bytes hold three frames, 11 frames take four sub-batches and the carry crosses three
    seams (1 MiB steps are fine enough: 6 MiB would give two frames, 9 MiB four)."""
    env = dict(os.environ, MIC_HIP_WS_BUDGET_MB="7")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mic2_crops_chunking_check.py")], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "mic2 crop seams ok" in r.stdout, r.stdout + r.stderr
