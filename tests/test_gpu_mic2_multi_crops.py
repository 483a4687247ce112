"""Crops of many MIC2 volumes per call into a device tensor (csrc/mic_mic2_crops.hip: mic_hip_mic2_multi_read_crops,
mic_hip_mic2_readers_read_crops, mic_hip_session_mic2_multi_read_crops).  The codec is lossless, so the expected value of every crop
is its volume's source, padded with zeros and cropped in numpy (mic2_crop_volumes.expected); the tensor must also equal, byte for
byte, what the single-volume call (test_gpu_mic2_crops.py) returns volume by volume.
Two things differ from the plain description of these cases.  The one-frame volume is 7 x 35, not 7 x 5: no frame of 35 pixels can be
coded (mic2_multi_volumes.volume_tiny).  And no reader opens on a file with a bad magic, so through the readers door that volume is a
None entry that crops name: it fails alone with MIC_ERR_ARGS, where the other two doors give the header's code."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import mic2_multi_volumes as M

pytestmark = pytest.mark.gpu

V = M.V
# (volume, temporal) in the order of the call's list: sizes, depths and pipelines mixed
ORDER = [("xr12", False), ("xr12", True), ("wrap16", True), ("wrap16", False), ("narrow", True), ("tiny", True), ("tiny", False)]


@pytest.fixture(scope="module")
def volumes(mic, synth, gpu_ready):
    """name -> dict(vol, files = {temporal: bytes}); each file decoded once and compared with its source, never written to"""
    out = {}
    for name, make in (("xr12", M.volume_12bit), ("wrap16", M.volume_16bit), ("narrow", M.volume_narrow), ("tiny", M.volume_tiny)):
        vol, maxv = make(synth)
        n, h, w = vol.shape
        files = {}
        for temporal in (False, True):
            data = mic.compress_multi_frame(vol, w, h, maxv, temporal=temporal)
            assert np.array_equal(mic.decompress_multi_frame(data), vol)
            assert M.Mic2File(data).temporal == temporal
            files[temporal] = data
        vol.setflags(write=False)
        out[name] = dict(vol=vol, files=files)
    assert out["narrow"]["vol"].shape == (3, 9, 33) and out["tiny"]["vol"].shape == (1, 35, 7)
    return out


def _listed(volumes, order=ORDER):
    return [volumes[name]["vol"] for name, _ in order], [volumes[name]["files"][t] for name, t in order]


def _tensor(n, cd, ch, cw):
    import torch
    return torch.full((max(n, 1), cd, ch, cw, 2), 0xA5, dtype=torch.uint8, device="cuda")   # (every byte must be overwritten)


def _read(call, xyzv, cw, ch, cd):
    """call(xyzv, cw, ch, cd, d_out, out_cap) -> (status, failed_frame, stats); the crops as (n, cd, ch, cw) u16"""
    t = _tensor(len(xyzv), cd, ch, cw)
    st, bad, stats = call(xyzv, cw, ch, cd, t.data_ptr(), len(xyzv) * cd * ch * cw * 2)
    return t.cpu().numpy()[: len(xyzv)].view("<u2")[..., 0], st, bad, stats


class _Doors:
    """the three entry points on one list of files (entries may be None or garbage): .files, .readers, .session, each
    call(xyzv, cw, ch, cd, d_out, out_cap)"""

    def __init__(self, mic, files, sources=None):
        import torch
        self.mic, self.data = mic, files
        ok = [f is not None and bytes(f[:4]) == b"MIC2" and len(f) >= 20 for f in files]
        self.rds = [mic.Mic2Reader(sources[v] if sources else f, len(f)) if ok[v] else None for v, f in enumerate(files)]
        self.sess = mic.Session(4, 150 * 70)
        self.d_files = [torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy()).cuda() if f else None for f in files]
        self.heads = [None if f is None else (M.Mic2File(f).head() if ok[v] else bytes(f)) for v, f in enumerate(files)]
        self.ptrs = [0 if d is None else d.data_ptr() for d in self.d_files]
        self.lens = [0 if f is None else len(f) for f in files]
        self.files = lambda xyzv, cw, ch, cd, d, cap: mic.mic2_multi_read_crops(files, xyzv, cw, ch, cd, d, cap)
        self.readers = lambda xyzv, cw, ch, cd, d, cap: mic.mic2_readers_read_crops(self.rds, xyzv, cw, ch, cd, d, cap)
        self.session = lambda xyzv, cw, ch, cd, d, cap: self.sess.mic2_multi_read_crops(self.heads, self.ptrs, self.lens, xyzv, cw, ch, cd, d, cap)
        self.all = [("files", self.files), ("readers", self.readers), ("session", self.session)]

    def close(self):
        for r in self.rds:
            if r is not None:
                r.close()
        self.sess.close()


def _single_volume_calls(mic, files, xyzv, cw, ch, cd):
    """what the single-volume call returns per volume, put at the places of the volume's crops"""
    out = np.zeros((len(xyzv), cd, ch, cw), dtype=np.uint16)
    for v, data in enumerate(files):
        idx, xyz = M.crops_of(xyzv, v)
        if idx:
            t = _tensor(len(xyz), cd, ch, cw)
            st, _ = mic.mic2_read_crops(data, xyz, cw, ch, cd, t.data_ptr(), len(xyz) * cd * ch * cw * 2)
            assert (st == 0).all()
            out[idx] = t.cpu().numpy().view("<u2")[..., 0]
    return out


@pytest.mark.parametrize("shape", M.SHAPES)
def test_crops_of_every_volume_in_one_chain(mic, volumes, shape):
    cw, ch, cd = shape
    vols, files = _listed(volumes)
    xyzv = M.interleave([V.origins(v.shape[2], v.shape[1], v.shape[0], cw, ch, cd) for v in vols])
    assert all(a[3] != b[3] for a, b in zip(xyzv, xyzv[1:]))              # consecutive crops name different volumes
    want = M.expected_multi(vols, xyzv, cw, ch, cd)
    single = _single_volume_calls(mic, files, xyzv, cw, ch, cd)
    assert want.tobytes() == single.tobytes()
    units, pieces, fs = mic.mic2_multi_crop_plan(files, xyzv, cw, ch, cd)
    assert (fs == 0).all()
    doors = _Doors(mic, files)
    try:
        for door, call in doors.all:
            got, st, bad, stats = _read(call, xyzv, cw, ch, cd)
            for i in range(len(xyzv)):
                assert np.array_equal(got[i], want[i]), (door, shape, xyzv[i])
            assert got.tobytes() == single.tobytes(), door
            assert (st == mic.MIC_OK).all() and (bad == -1).all(), (door, st, bad)
            assert stats == dict(frames_decoded=len(units), pieces=pieces, slabs=1, volumes_read=len(files)), (door, stats)
        outside = [(v.shape[2], 0, 0, k) for k, v in enumerate(vols)] + [(0, 0, -cd, 1), (0, 0, 11, 0)]
        for door, call in doors.all:
            got, st, bad, stats = _read(call, outside, cw, ch, cd)
            assert not got.any() and (st == 0).all() and (bad == -1).all(), door
            assert stats == dict(frames_decoded=0, pieces=0, slabs=0, volumes_read=len(files)), (door, stats)
    finally:
        doors.close()


def test_a_volume_twice_and_unnamed_entries(mic, volumes):
    cw, ch, cd = 48, 40, 3
    xr, wrap = volumes["xr12"], volumes["wrap16"]
    vols = [None, xr["vol"], None, xr["vol"], wrap["vol"], None, xr["vol"]]
    files = [None, xr["files"][True], b"garbage, and not a little of it", xr["files"][True], wrap["files"][False], b"MIC2", xr["files"][False]]
    per = [None if v is None else V.origins(v.shape[2], v.shape[1], v.shape[0], cw, ch, cd)[:7] for v in vols]
    per[3] = [(9, 9, 4), (40, 20, 7), (3, 30, 8)]                         # the second listing of the temporal file: other crops
    xyzv = M.interleave(per)
    want = M.expected_multi(vols, xyzv, cw, ch, cd)
    units, pieces, fs = mic.mic2_multi_crop_plan(files, xyzv, cw, ch, cd)
    assert (fs == 0).all()
    assert [f for v, f in units.tolist() if v == 1] != [f for v, f in units.tolist() if v == 3] == list(range(11))   # two sets of units
    doors = _Doors(mic, files)
    try:
        for door, call in doors.all:
            got, st, bad, stats = _read(call, xyzv, cw, ch, cd)
            assert np.array_equal(got, want) and (st == 0).all() and (bad == -1).all(), door
            assert stats == dict(frames_decoded=len(units), pieces=pieces, slabs=1, volumes_read=4), (door, stats)
        # one reader as two volumes: the same streams, pulled once
        src = M.RecordingSource(files[1])
        with mic.Mic2Reader(src, len(files[1])) as rd:
            src.reads.clear()
            rds = [None, rd, None, rd, doors.rds[4], None, doors.rds[6]]
            got, st, bad, stats = _read(lambda *a: mic.mic2_readers_read_crops(rds, *a), xyzv, cw, ch, cd)
            assert np.array_equal(got, want) and (st == 0).all() and stats["volumes_read"] == 4
            m = M.Mic2File(files[1])
            cover = src.coverage()
            assert cover.max() == 1 and cover[m.span(0)[0]: m.span(10)[1]].all() and len(src.reads) == 1
    finally:
        doors.close()


def _frame_code(mic, m, data, temporal):
    """(code, volume) the existing decoders give for the damaged file: the unit codec's code of frame 5, and -- should the damaged
    stream still decode -- the pixels it decodes to (as test_gpu_mic2_crops.py)"""
    if temporal:
        try:
            return mic.MIC_OK, np.asarray(mic.decompress_multi_frame(data)).reshape(m.n, m.h, m.w)
        except mic.MicError as e:
            return e.code, None
    b, e = m.span(5)
    (code, px), = mic.decompress_batch([bytes(data[b:e])], [(m.w, m.h)])
    return code, px


def test_a_refused_volume_fails_alone(mic, volumes):
    cw, ch, cd = 48, 40, 3
    vols, files = _listed(volumes)
    bad_magic = b"MIC3" + files[1][4:]
    code = mic.lib().mic_hip_mic2_info(bad_magic, len(bad_magic), None, None, None, None)
    assert code == mic.MIC_ERR_CORRUPT
    files = files[:1] + [bad_magic] + files[2:]
    xyzv = M.interleave([V.origins(v.shape[2], v.shape[1], v.shape[0], cw, ch, cd) for v in vols])
    want = M.expected_multi(vols[:1] + [None] + vols[2:], xyzv, cw, ch, cd)
    doors = _Doors(mic, files)
    try:
        assert doors.rds[1] is None                                       # (no reader opens on it: a None entry that crops name)
        for door, call in doors.all:
            got, st, bad, stats = _read(call, xyzv, cw, ch, cd)
            mine = np.asarray([c[3] == 1 for c in xyzv])
            assert (st[mine] == (mic.MIC_ERR_ARGS if door == "readers" else code)).all() and (st[~mine] == 0).all(), (door, st)
            assert (bad == -1).all() and not got[mine].any() and np.array_equal(got, want), door
            assert stats["volumes_read"] == len(files) - 1 and stats["slabs"] == 1, (door, stats)
    finally:
        doors.close()


@pytest.mark.parametrize("temporal", [False, True])
def test_a_damaged_frame_fails_its_dependants_only(mic, volumes, temporal):
    cw, ch, cd = 48, 40, 3
    vols, files = _listed(volumes)
    at = ORDER.index(("xr12", temporal))
    vol = vols[at]
    n, h, w = vol.shape
    m = M.Mic2File(files[at])
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
    files = files[:at] + [data] + files[at + 1:]
    per = [V.origins(v.shape[2], v.shape[1], v.shape[0], cw, ch, cd) for v in vols]
    per[at] = per[at] + [(5, 5, 5), (60, 10, 6), (60, 10, 8)]
    xyzv = M.interleave(per)
    want = M.expected_multi(vols[:at] + [want_vol] + vols[at + 1:], xyzv, cw, ch, cd)
    doors = _Doors(mic, files)
    try:
        for door, call in doors.all:
            got, st, bad, stats = _read(call, xyzv, cw, ch, cd)
            assert stats["slabs"] == 1                                    # every other volume shares the damaged one's sub-batch
            hit = 0
            for i, o in enumerate(xyzv):
                frames, pieces = V.brute_plan(w, h, n, False, [o[:3]], cw, ch, cd)
                depends = o[3] == at and bool(pieces) and (max(frames) >= 5 if temporal else 5 in frames)
                hit += depends
                assert st[i] == (code if depends else mic.MIC_OK), (door, o, st[i])
                assert bad[i] == (5 if depends and code != mic.MIC_OK else -1), (door, o, bad[i])
                if not depends or code == mic.MIC_OK:
                    assert np.array_equal(got[i], want[i]), (door, o)
            assert 0 < hit < len(per[at])
    finally:
        doors.close()


@pytest.mark.parametrize("temporal", [False, True])
def test_an_empty_table_entry_fails_its_volume_alone(mic, volumes, temporal):
    cw, ch, cd = 48, 40, 3
    vols, files = _listed(volumes)
    at = ORDER.index(("xr12", temporal))
    m = M.Mic2File(files[at])
    struct.pack_into("<I", m.data, 20 + 8 * 5 + 4, 0)
    files = files[:at] + [bytes(m.data)] + files[at + 1:]
    per = [V.origins(v.shape[2], v.shape[1], v.shape[0], cw, ch, cd)[:8] for v in vols]
    doors = _Doors(mic, files)
    try:
        for needs, mine in ((True, [(0, 0, 4), (20, 10, 0)]), (False, [(0, 0, 2), (20, 10, 0)])):
            per[at] = mine
            xyzv = M.interleave(per)
            full = M.expected_multi(vols, xyzv, cw, ch, cd)
            want = M.expected_multi(vols[:at] + [None] + vols[at + 1:], xyzv, cw, ch, cd) if needs else full
            sel = np.asarray([c[3] == at for c in xyzv])
            for door, call in doors.all:
                got, st, bad, stats = _read(call, xyzv, cw, ch, cd)
                assert np.array_equal(got, want) and (bad == -1).all(), (door, needs)
                assert (st[sel] == (mic.MIC_ERR_CORRUPT if needs else 0)).all() and (st[~sel] == 0).all(), (door, needs, st)
                assert stats["volumes_read"] == len(files) - needs, (door, stats)
    finally:
        doors.close()


def test_the_readers_pull_the_plans_streams_only(mic, volumes):
    cw, ch, cd = 48, 40, 3
    vols, files = _listed(volumes)
    per = [[(10, 5, 1), (60, 20, 2), (100, 30, 7), (-4, 40, 7), (150, 0, 9)],     # independent: frames 1 .. 4 and 7 .. 9 (the last crop: outside)
           [(10, 5, 1), (100, 30, 6)],                                            # temporal: frames 0 .. 8
           [(3, 3, 1)], None, [(0, 0, 0)], None, [(0, 0, 0)]]
    xyzv = M.interleave(per)
    srcs = [M.RecordingSource(f) for f in files]
    doors = _Doors(mic, files, sources=srcs)
    try:
        for s in srcs:
            s.reads.clear()
        got, st, bad, stats = _read(doors.readers, xyzv, cw, ch, cd)
        assert np.array_equal(got, M.expected_multi(vols, xyzv, cw, ch, cd)) and (st == 0).all()
        units, pieces, fs = mic.mic2_multi_crop_plan(files, xyzv, cw, ch, cd)
        assert stats == dict(frames_decoded=len(units), pieces=pieces, slabs=1, volumes_read=5)
        for v, (f, s) in enumerate(zip(files, srcs)):
            m = M.Mic2File(f)
            want = np.zeros(len(f), dtype=np.int32)
            for vv, fr in units.tolist():
                if vv == v:
                    b, e = m.span(fr)
                    want[b:e] += 1
            assert want.max() <= 1 and np.array_equal(s.coverage(), want), v     # exactly the plan's streams, each byte once
        assert [len(s.reads) for s in srcs] == [2, 1, 1, 0, 1, 0, 1]              # neighbours in one read; an unnamed reader: none

        # a failing callback: MIC_ERR_IO, and the tensor is untouched
        def broken(off, n):
            raise OSError("no such sector")
        ok = mic.Mic2Reader(files[1])
        failing = mic.Mic2Reader(lambda off, n: files[0][off: off + n] if off + n <= 20 + 8 * 11 else broken(off, n), len(files[0]))
        t = _tensor(2, cd, ch, cw)
        a = np.asarray([(0, 0, 0, 0), (0, 0, 0, 1)], dtype=np.int32)
        st2 = np.zeros(2, dtype=np.int32)
        hs = np.asarray([failing._h.value, ok._h.value], dtype=np.uintp)
        rc = mic.lib().mic_hip_mic2_readers_read_crops(hs.ctypes.data, 2, a.ctypes.data, 2, cw, ch, cd, t.data_ptr(), t.numel(), st2.ctypes.data, None, None)
        assert rc == mic.MIC_ERR_IO and (t.cpu().numpy() == 0xA5).all()
        failing._cb.exc = None
        with pytest.raises(OSError):                                     # through the Python door the source's own exception comes back
            mic.mic2_readers_read_crops([failing, ok], a, cw, ch, cd, t.data_ptr(), t.numel())
        assert (t.cpu().numpy() == 0xA5).all()
        ok.close(); failing.close()
    finally:
        doors.close()


def test_pinned_host_output(mic, volumes):
    vols, files = _listed(volumes)
    xyzv = [(0, 0, 4, 1), (3, -2, 1, 2), (0, 0, 0, 6), (10, 10, 8, 0)]
    cw, ch, cd = 150, 70, 3
    buf = mic.host_alloc(len(xyzv) * cd * ch * cw * 2)
    try:
        buf[:] = 0xA5
        st, bad, stats = mic.mic2_multi_read_crops(files, xyzv, cw, ch, cd, buf.ctypes.data, buf.size)
        assert (st == 0).all() and stats["slabs"] == 1 and stats["volumes_read"] == 4
        assert np.array_equal(buf.view("<u2").reshape(len(xyzv), cd, ch, cw), M.expected_multi(vols, xyzv, cw, ch, cd))
    finally:
        mic.host_free(buf)


def test_argument_errors_come_back_before_any_launch(mic, volumes):
    vols, files = _listed(volumes)
    files = files[:3]
    cw, ch, cd = 48, 40, 3
    xyzv = [(0, 0, 0, 0), (10, 10, 2, 1), (5, 5, 1, 2)]
    want = M.expected_multi(vols[:3], xyzv, cw, ch, cd)
    t = _tensor(3, cd, ch, cw)
    cap = 3 * cd * ch * cw * 2
    pageable = np.zeros(cap, dtype=np.uint8)
    many = [(0, 0, 0, 0)] * 64                                            # 64 whole volumes: far past the allocation t lies in
    doors = _Doors(mic, files)
    a = np.asarray(xyzv, dtype=np.int32)
    far = np.asarray(xyzv[:2] + [(5, 5, 1, 3)], dtype=np.int32)           # a volume index outside the list ...
    neg = np.asarray(xyzv[:2] + [(5, 5, 1, -1)], dtype=np.int32)
    st3, bad3 = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
    L = mic.lib()
    _, fptrs, flens = mic._volume_table(files)
    _, hptrs, hlens = mic._volume_table(doors.heads)
    dptrs, dlens = np.asarray(doors.ptrs, dtype=np.uintp), np.asarray(doors.lens, dtype=np.uintp)
    rptrs = np.asarray([r._h.value for r in doors.rds], dtype=np.uintp)
    tail = lambda xy, nn, d, c: (xy.ctypes.data if xy is not None else None, nn, cw, ch, cd, d, c, st3.ctypes.data, bad3.ctypes.data, None)
    raw = [lambda xy, nn, d=t.data_ptr(), c=cap, nf=3, f=fptrs.ctypes.data: L.mic_hip_mic2_multi_read_crops(f, flens.ctypes.data, nf, *tail(xy, nn, d, c)),
           lambda xy, nn, d=t.data_ptr(), c=cap, nf=3, f=rptrs.ctypes.data: L.mic_hip_mic2_readers_read_crops(f, nf, *tail(xy, nn, d, c)),
           lambda xy, nn, d=t.data_ptr(), c=cap, nf=3, f=hptrs.ctypes.data: L.mic_hip_session_mic2_multi_read_crops(
               doors.sess._h, f, hlens.ctypes.data, dptrs.ctypes.data, dlens.ctypes.data, nf, *tail(xy, nn, d, c))]
    try:
        for (door, call), raw_call in zip(doors.all, raw):
            for args, code in [((xyzv, 0, ch, cd, t.data_ptr(), cap), mic.MIC_ERR_ARGS), ((xyzv, cw, 0, cd, t.data_ptr(), cap), mic.MIC_ERR_ARGS),
                               ((xyzv, cw, ch, -1, t.data_ptr(), cap), mic.MIC_ERR_ARGS), ((xyzv, cw, ch, cd, t.data_ptr(), cap - 1), mic.MIC_ERR_CAPACITY),
                               ((far, cw, ch, cd, t.data_ptr(), cap), mic.MIC_ERR_ARGS), ((neg, cw, ch, cd, t.data_ptr(), cap), mic.MIC_ERR_ARGS),
                               ((far, cw, ch, cd, t.data_ptr(), cap - 1), mic.MIC_ERR_CAPACITY),      # ... comes behind the capacity
                               ((xyzv, cw, ch, cd, 0, cap), mic.MIC_ERR_ARGS),
                               ((xyzv, cw, ch, cd, pageable.ctypes.data, cap), mic.MIC_ERR_ARGS),
                               ((far, cw, ch, cd, pageable.ctypes.data, cap), mic.MIC_ERR_ARGS),
                               ((many, 150, 70, 11, t.data_ptr(), 64 * 11 * 70 * 150 * 2), mic.MIC_ERR_ARGS)]:
                with pytest.raises(mic.MicError) as e:
                    call(*args)
                assert e.value.code == code, (door, args)
            assert raw_call(a, -1) == mic.MIC_ERR_ARGS, door              # n = -1
            assert raw_call(a, 3, nf=-1) == mic.MIC_ERR_ARGS, door        # nfiles = -1
            assert raw_call(None, 3) == mic.MIC_ERR_ARGS, door            # a NULL array that is needed
            assert raw_call(a, 3, f=None) == mic.MIC_ERR_ARGS, door
            assert raw_call(a, 3, c=cap - 1, f=None) == mic.MIC_ERR_ARGS, door     # ... comes before the capacity
            assert (t.cpu().numpy() == 0xA5).all() and not pageable.any(), door     # none of the refused calls wrote a byte
            assert raw_call(a, 3) == mic.MIC_OK, door                     # (the same call with good arguments)
            assert np.array_equal(t.cpu().numpy().view("<u2")[..., 0], want) and (st3 == 0).all() and (bad3 == -1).all(), door
            t.fill_(0xA5)
            st, bad, stats = call([], cw, ch, cd, t.data_ptr(), 0)        # n = 0: nothing to do, and that is no error
            assert st.size == 0 and stats == dict(frames_decoded=0, pieces=0, slabs=0, volumes_read=0)
            assert raw_call(None, 0, d=None, c=0, nf=0, f=None) == mic.MIC_OK, door
            assert (t.cpu().numpy() == 0xA5).all()
    finally:
        doors.close()


def test_both_kernels_are_timed_under_their_names(mic, volumes):
    vols, files = _listed(volumes)
    doors = _Doors(mic, files)
    try:
        doors.sess.set_timing(True)
        xyzv = [(0, 0, 0, 0), (5, 5, 3, 1), (0, 0, 1, 4), (2, 2, 0, 3)]
        got, st, bad, stats = _read(doors.session, xyzv, 48, 40, 3)
        assert np.array_equal(got, M.expected_multi(vols, xyzv, 48, 40, 3)) and stats["slabs"] == 1
        names = dict(doors.sess.last_timings())
        assert "k_mic2_gather_crops" in names and "k_mic2_accumulate_crops" in names, names
    finally:
        doors.close()


def test_sub_batch_seams_under_a_small_workspace():
    """tests/mic2_multi_chunking_check.py in a fresh process with a 7 MiB workspace ceiling.  A sub-batch holds
    budget / (unit_ws_bytes(mp) + 2 mp) units, mp its largest frame (the arithmetic of
    test_gpu_mic2_crops.py::test_sub_batch_seams_under_a_small_workspace): 150 x 70 = 10500 pixels are 2264704 + 21000 = 2285704
    bytes a unit, 7 MiB = 7340032 bytes hold three of them; 160 x 96 = 15360 pixels are 2459712 + 30720 = 2490432 bytes, two of them;
    33 x 9 and 7 x 35 pixels are 1.86 MB (the tables), three of them.  So a sub-batch holds two or three frames, and the script's
    volumes are ordered so that the cuts fall inside temporal volumes, behind a frame 0 and around an independent volume."""
    env = dict(os.environ, MIC_HIP_WS_BUDGET_MB="7")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mic2_multi_chunking_check.py")], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "mic2 multi crop seams ok" in r.stdout, r.stdout + r.stderr
