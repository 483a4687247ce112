"""Many crops of many single-frame RGB files per call into a device tensor (csrc/mic_rgb_crops.hip: mic_hip_rgb_read_crops,
mic_hip_session_rgb_read_crops and their _as twins; the mode-aware gather of csrc/mic_gather.hip).  The codec is lossless, so the
expected value of every crop is the source image cropped in numpy, zero (or pad) outside (rgb_crop_files.expected) -- never anything
the code under test returned.  The files are the CPU oracle's blobs and MICR files of tests/test_gpu_rgb_batch.py's plane-mode set and
two blobs assembled by hand with raw planes 70 samples wide; each is decoded once with mic_hip_rgb_decompress_batch first."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import out_spec_ref as R
import rgb_crop_files as F

pytestmark = pytest.mark.gpu


def _whole(mic, entries):
    """[(status, failed plane, pixels)] of mic_hip_rgb_decompress_batch over blob / MICR entries"""
    got = mic.decompress_rgb_batch([e if isinstance(e, bytes) else e[0] for e in entries],
                                   [None if isinstance(e, bytes) else (e[1], e[2]) for e in entries])
    return [(st, fp, px) for (st, px), fp in zip(got, mic.decompress_rgb_batch.failed_planes)]


@pytest.fixture(scope="module")
def files(mic, mico, synth, gpu_ready):
    """[(image, file entry, plane modes)]; every file decodes to its source through the whole-image door, and is never written to"""
    out = F.build(synth, mico)
    for (im, _, _), (st, fp, px) in zip(out, _whole(mic, [f for _, f, _ in out])):
        assert st == mic.MIC_OK and fp == -1 and np.array_equal(px, im)
    for (_, _, m), want in zip(out, F.WANT_MODES):
        assert want is None or m == want
    assert 2 in out[8][2][1:]
    return out


def _tensor(n, ch, cw):
    import torch
    return torch.full((max(n, 1), ch, cw, 3), 0xA5, dtype=torch.uint8, device="cuda")    # (every byte must be overwritten)


def _read(call, xyf, cw, ch):
    """call(xyf, cw, ch, d_out, out_cap) -> (status, failed plane, stats); the crops as (n, ch, cw, 3) u8"""
    t = _tensor(len(xyf), ch, cw)
    st, bad, stats = call(xyf, cw, ch, t.data_ptr(), len(xyf) * ch * cw * 3)
    return t.cpu().numpy()[: len(xyf)], st, bad, stats


class _Doors:
    """the two entry points on one list of files: .file and .session, each call(xyf, cw, ch, d_out, out_cap, spec=None).  The
    session form reads blobs that lie back to back in device memory: a MICR file gives its blob and its header's size."""

    def __init__(self, mic, entries):
        import torch
        blobs, self.images = [], []
        for e in entries:
            if isinstance(e, bytes):
                w, h = struct.unpack("<II", e[4:12])
                blobs.append(e[12:]); self.images.append((0, w, h))
            else:
                blobs.append(e[0]); self.images.append((0, e[1], e[2]))
        self.offs = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
        self.d_blobs = torch.from_numpy(np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()).cuda()
        self.sess = mic.Session(4, 64 * 64)
        self.file = lambda xyf, cw, ch, d, cap, spec=None: mic.rgb_read_crops(entries, xyf, cw, ch, d, cap, spec=spec)
        self.session = lambda xyf, cw, ch, d, cap, spec=None: self.sess.rgb_read_crops(self.d_blobs.data_ptr(), self.offs, self.images,
                                                                                       xyf, cw, ch, d, cap, spec=spec)
        self.all = [("file", self.file), ("session", self.session)]

    def close(self):
        self.sess.close()


def test_the_placement_meets_every_alignment(files):
    """pieces start at odd and at even columns of their image, and every alignment mod 4 of the first destination byte occurs"""
    for cw, ch in F.SHAPES:
        xyf = F.origins(files, cw, ch)
        src, dst = set(), set()
        for i, (x, y, f) in enumerate(xyf):
            o = F.overlap(files[f][0], x, y, cw, ch)
            if o:
                src.add(o[0] % 2)
                dst.add((((i * ch + o[2] - y) * cw + o[0] - x) * 3) % 4)
        assert src == {0, 1} and dst == {0, 1, 2, 3}, (cw, ch, src, dst)


@pytest.mark.parametrize("shape", F.SHAPES)
def test_crops_equal_the_sources(mic, files, shape):
    cw, ch = shape
    entries = [f for _, f, _ in files]
    xyf = F.origins(files, cw, ch, skip=(2,))                                # file 2 is named by no crop
    want = F.expected(files, xyf, cw, ch)
    file_of, planes, pieces, fs = mic.rgb_crop_plan(entries, xyf, cw, ch)
    assert (file_of.tolist(), planes, pieces) == F.brute_plan(files, xyf, cw, ch) and 2 not in file_of
    doors = _Doors(mic, entries)
    try:
        for door, call in doors.all:
            got, st, bad, stats = _read(call, xyf, cw, ch)
            for i in range(len(xyf)):
                assert np.array_equal(got[i], want[i]), (door, shape, xyf[i])
            assert (st == mic.MIC_OK).all() and (bad == -1).all(), (door, st, bad)
            assert stats == dict(planes_decoded=planes, planes_total=3 * len(file_of), pieces=pieces, slabs=1), (door, stats)
        outside = [(files[f][0].shape[1], 0, f) for f in range(len(files))] + [(0, 320, 9), (-cw, 0, 7), (3, -ch, 5)]
        for door, call in doors.all:
            got, st, bad, stats = _read(call, outside, cw, ch)
            assert not got.any() and (st == 0).all() and (bad == -1).all(), door
            assert stats == dict(planes_decoded=0, planes_total=0, pieces=0, slabs=0), (door, stats)
        raw_only = [(0, 0, 10), (0, 0, 3), (1, 0, 4), (0, 0, 1), (0, 0, 0)]     # raw and constant planes alone: no decode chain at all
        for door, call in doors.all:
            got, st, bad, stats = _read(call, raw_only, cw, ch)
            assert np.array_equal(got, F.expected(files, raw_only, cw, ch)) and (st == 0).all(), door
            assert stats == dict(planes_decoded=0, planes_total=15, pieces=5, slabs=0), (door, stats)
    finally:
        doors.close()


def test_the_same_call_twice_gives_identical_bytes(mic, files):
    entries = [f for _, f, _ in files]
    xyf = F.origins(files, 65, 6)
    doors = _Doors(mic, entries)
    try:
        for door, call in doors.all:
            a = _read(call, xyf, 65, 6)
            b = _read(call, xyf, 65, 6)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3], door
            assert np.array_equal(a[0], F.expected(files, xyf, 65, 6)), door
    finally:
        doors.close()


def test_session_blobs_from_rgb_encode_and_pinned_output(mic, files):
    """blobs as Session.rgb_encode leaves them, read where they lie; d_out a torch tensor and pinned host memory; the host form's bytes"""
    import torch
    sub = [files[k] for k in (9, 7, 5, 8, 6, 4)]
    imgs = [im for im, _, _ in sub]
    flat = np.concatenate([im.reshape(-1) for im in imgs])
    table, off = [], 0
    for im in imgs:
        table.append((off, im.shape[1], im.shape[0])); off += im.size
    d_rgb = torch.from_numpy(flat).cuda()
    cw, ch = 63, 9
    xyf = F.origins(sub, cw, ch)
    want = F.expected(sub, xyf, cw, ch)
    nbytes = len(xyf) * ch * cw * 3
    enc, rd = mic.Session(4, 64 * 64), mic.Session(4, 64 * 64)
    pin = mic.host_alloc(nbytes)
    try:
        d_blobs, offs, st, fp = enc.rgb_encode(d_rgb.data_ptr(), table)
        assert (st == 0).all() and (fp == -1).all()
        host_blobs = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda")
        mic.device_copy(host_blobs.data_ptr(), d_blobs, int(offs[-1]))
        hb = host_blobs.cpu().numpy()
        entries = [(hb[int(offs[i]): int(offs[i + 1])].tobytes(), im.shape[1], im.shape[0]) for i, im in enumerate(imgs)]
        t = _tensor(len(xyf), ch, cw)
        st_h, bad_h, stats_h = mic.rgb_read_crops(entries, xyf, cw, ch, t.data_ptr(), nbytes)
        host_form = t.cpu().numpy()
        assert np.array_equal(host_form, want) and (st_h == 0).all()
        # the blobs where rgb_encode left them (another session reads them: the encoder's buffers stay as they are)
        t2 = _tensor(len(xyf), ch, cw)
        st_s, bad_s, stats_s = rd.rgb_read_crops(d_blobs, offs, table, xyf, cw, ch, t2.data_ptr(), nbytes)
        assert np.array_equal(t2.cpu().numpy(), host_form) and (st_s == 0).all() and (bad_s == -1).all() and stats_s == stats_h
        # ... and the encoding session itself, into pinned host memory
        pin[:] = 0xA5
        st_p, bad_p, stats_p = enc.rgb_read_crops(d_blobs, offs, table, xyf, cw, ch, pin.ctypes.data, nbytes)
        assert np.array_equal(pin.reshape(want.shape), host_form) and (st_p == 0).all() and stats_p == stats_h
        pin[:] = 0xA5
        st_p, bad_p, stats_p = mic.rgb_read_crops(entries, xyf, cw, ch, pin.ctypes.data, nbytes)
        assert np.array_equal(pin.reshape(want.shape), host_form) and (st_p == 0).all()
    finally:
        mic.host_free(pin)
        enc.close(); rd.close()


def test_a_file_fails_alone(mic, mico, synth, files):
    """tests/test_gpu_rgb_batch.py's test_a_job_fails_alone_on_decode, read through the crop doors: every file carries the code and
    plane mic_hip_rgb_decompress_batch gives it, refused files' crops are zero, the good files' crops exact"""
    a, b = synth.wsi_like(67, 65, seed=3), F.noise(synth, 64, 64, 5)
    fa, fb = mico.wsi_compress_tile(a)[1], mico.wsi_compress_tile(b)[1]
    ma = mico.micr_write(a)[1]
    assert F.modes(fb) == [2, 2, 2]
    long_co = fa[:4] + (int.from_bytes(fa[4:8], "little") + len(fa)).to_bytes(4, "little") + fa[8:]
    l0, l1 = int.from_bytes(fb[0:4], "little"), int.from_bytes(fb[4:8], "little")
    flipped = None
    for k in range(2, min(l1, 40)):                                          # a flipped byte inside the Co stream for which the oracle's decoder fails too
        cand = bytearray(fb); cand[12 + l0 + k] ^= 0xFF
        if mico.wsi_decompress_tile(bytes(cand), 64, 64)[0] != 0:
            flipped = bytes(cand)
            break
    assert flipped is not None
    entries = [(fa, 67, 65), (fb[:-1], 64, 64), (fb, 64, 64), (long_co, 67, 65), b"MICX" + ma[4:], ma, (ma, 66, 65, 1), (flipped, 64, 64), (fa, 67, 65)]
    imgs = [a, b, b, a, a, a, a, b, a]
    lst = [(im, e, None) for im, e in zip(imgs, entries)]
    # what the whole-image door says of each (the mismatching MICR dims go through the raw job table)
    n = len(entries)
    jobs = (mic.RgbDecJob * n)()
    keep = []
    for i, e in enumerate(entries):
        data, w, h, c = (e, 0, 0, 1) if isinstance(e, bytes) else (e[0], e[1], e[2], e[3] if len(e) > 3 else 0)
        cbuf = np.frombuffer(data, np.uint8); out = np.zeros(67 * 65 * 3, np.uint8)
        keep.append((cbuf, out))
        jobs[i].compressed = cbuf.ctypes.data; jobs[i].compressed_len = cbuf.size; jobs[i].rgb_out = out.ctypes.data; jobs[i].out_cap = out.size
        jobs[i].container = c; jobs[i].width, jobs[i].height = w, h
    assert mic.lib().mic_hip_rgb_decompress_batch(jobs, n) == mic.MIC_OK
    door = [(j.status, j.failed_plane) for j in jobs]
    assert [d[0] == 0 for d in door] == [True, False, True, False, False, True, False, False, True]
    assert door[1] == door[3] == door[4] == (mic.MIC_ERR_CORRUPT, -1) and door[6] == (mic.MIC_ERR_ARGS, -1)
    assert door[7][0] != 0 and door[7][1] == 1                               # "Co plane: %w"
    cw, ch = 17, 5
    xyf = F.origins(lst, cw, ch)
    want = F.expected(lst, xyf, cw, ch)
    file_of, planes, pieces, fs = mic.rgb_crop_plan(entries, xyf, cw, ch)
    assert fs.tolist() == [d[0] if k != 7 else 0 for k, d in enumerate(door)]  # (a damaged stream is no header's business)
    assert file_of.tolist() == [0, 2, 5, 7, 8]

    def check(call, which, label):
        got, st, bad, stats = _read(call, [xyf[i] for i in which], cw, ch)
        for j, i in enumerate(which):
            f = xyf[i][2]
            named = F.overlap(imgs[f], xyf[i][0], xyf[i][1], cw, ch) is not None
            if f == 7:                                                       # the unit codec's code, for the crops that need the plane
                assert (st[j], bad[j]) == (door[7] if named else (0, -1)), (label, xyf[i])
                if not named:
                    assert not got[j].any()
            elif door[f][0] != 0:
                assert (st[j], bad[j]) == door[f] and not got[j].any(), (label, xyf[i], st[j], bad[j])
            else:
                assert (st[j], bad[j]) == (0, -1) and np.array_equal(got[j], want[i]), (label, xyf[i])
        return stats
    stats = check(lambda *a: mic.rgb_read_crops(entries, *a), list(range(len(xyf))), "file")
    assert stats["planes_total"] == 15 and stats["planes_decoded"] == 3 * F.modes(fa).count(2) + 6 == planes and stats["slabs"] == 1
    # the session form takes blobs: the six blob entries
    blobs_only = [k for k, e in enumerate(entries) if isinstance(e, tuple) and len(e) == 3]
    doors = _Doors(mic, [entries[k] for k in blobs_only])
    try:
        which = [i for i, o in enumerate(xyf) if o[2] in blobs_only]
        remap = {k: j for j, k in enumerate(blobs_only)}
        check(lambda xs, *a: doors.session([(x, y, remap[f]) for x, y, f in xs], *a), which, "session")
    finally:
        doors.close()


def _pairs(nfiles):
    """one exact pair per (file, channel), all different"""
    pairs = [((1 + k) / 1024.0, -0.25 * (k % 7)) for k in range(3 * nfiles)]
    assert all(R.exact_pair(*p) for p in pairs) and len(set(pairs)) == len(pairs)
    return pairs


def _typed_want(files, xyf, cw, ch, dtype, pairs=None, clamp=None, pad=0.0, channels_first=False, refused=()):
    x = F.expected(files, xyf, cw, ch)
    outside = R.outside_mask(xyf, lambda i: files[xyf[i][2]][0].shape[1], lambda i: files[xyf[i][2]][0].shape[0], cw, ch)[..., None]
    outside = np.broadcast_to(outside, x.shape).copy()
    for i, o in enumerate(xyf):
        if o[2] in refused:
            outside[i] = True
    if pairs is None:
        a, b = 1.0, 0.0
    else:
        ab = np.asarray([[pairs[3 * o[2] + c] for c in range(3)] for o in xyf], dtype=np.float64)    # (n, 3, 2)
        a, b = ab[:, None, None, :, 0], ab[:, None, None, :, 1]
    want = R.convert(x, dtype, a, b, clamp=clamp, pad=pad, outside=outside)
    R.assert_no_subnormals(want, dtype)
    return np.ascontiguousarray(want.transpose(0, 3, 1, 2)) if channels_first else want


def test_typed_doors(mic, files):
    entries = [f for _, f, _ in files]
    cw, ch = 65, 6
    xyf = F.origins(files, cw, ch)
    count = len(xyf) * ch * cw * 3
    pairs = _pairs(len(files))
    doors = _Doors(mic, entries)
    try:
        for door, call in doors.all:
            # bf16, channels first, one pair per (file, channel)
            spec = mic.OutSpec("bf16", channels_first=True, affine=pairs)
            buf = R.Buffer(count, "bf16")
            st, bad, stats = call(xyf, cw, ch, buf.ptr, buf.nbytes, spec)
            want = _typed_want(files, xyf, cw, ch, "bf16", pairs, channels_first=True)
            assert np.array_equal(buf.bits().reshape(want.shape), want) and (st == 0).all(), door
            # u8, interleaved, one pair and a clamp, at an odd address
            spec = mic.OutSpec("u8", affine=[(0.5, 3.0)], clamp=(20.0, 100.0))
            buf = R.Buffer(count, "u8", skew=1)
            st, bad, stats = call(xyf, cw, ch, buf.ptr, buf.nbytes, spec)
            want = _typed_want(files, xyf, cw, ch, "u8", [(0.5, 3.0)] * (3 * len(files)), clamp=(20.0, 100.0))
            assert np.array_equal(buf.bits().reshape(want.shape), want) and (st == 0).all(), door
            # f32 with pad -1: overhanging and outside crops
            spec = mic.OutSpec("f32", pad=-1.0)
            buf = R.Buffer(count, "f32")
            st, bad, stats = call(xyf, cw, ch, buf.ptr, buf.nbytes, spec)
            want = _typed_want(files, xyf, cw, ch, "f32", pad=-1.0)
            assert (want.view(np.float32) == -1.0).any() and np.array_equal(buf.bits().reshape(want.shape), want) and (st == 0).all(), door
            # the NATIVE spec is the native door byte for byte
            native = _read(call, xyf, cw, ch)
            t = _tensor(len(xyf), ch, cw)
            st, bad, stats = call(xyf, cw, ch, t.data_ptr(), count, mic.OutSpec("native"))
            assert np.array_equal(t.cpu().numpy(), native[0]) and np.array_equal(st, native[1]) and stats == native[3], door
            # a typed tensor is judged like the native one: alignment and capacity before any launch
            for ptr, cap, code in ((buf.ptr + 2, buf.nbytes, mic.MIC_ERR_ARGS), (buf.ptr, buf.nbytes - 1, mic.MIC_ERR_CAPACITY)):
                with pytest.raises(mic.MicError) as e:
                    call(xyf, cw, ch, ptr, cap, mic.OutSpec("f32"))
                assert e.value.code == code, door
    finally:
        doors.close()
    # a refused file's crops are pad
    bad_entries = list(entries)
    bad_entries[7] = (entries[7][0][:-1], entries[7][1], entries[7][2])
    buf = R.Buffer(count, "f32")
    st, bad, stats = mic.rgb_read_crops(bad_entries, xyf, cw, ch, buf.ptr, buf.nbytes, spec=mic.OutSpec("f32", pad=-1.0))
    want = _typed_want(files, xyf, cw, ch, "f32", pad=-1.0, refused=(7,))
    assert np.array_equal(buf.bits().reshape(want.shape), want)
    assert all(s == (mic.MIC_ERR_CORRUPT if o[2] == 7 else 0) for s, o in zip(st, xyf))


def test_argument_errors_come_back_before_any_launch(mic, files):
    entries = [f for _, f, _ in files]
    cw, ch = 32, 16
    xyf = [(0, 0, 9), (10, 10, 7)]
    t = _tensor(2, ch, cw)
    cap = 2 * ch * cw * 3
    pageable = np.zeros(cap, dtype=np.uint8)
    many = [(0, 0, 9)] * 16384                                               # 24 MiB of crops: far past the allocation t lies in
    doors = _Doors(mic, entries)
    try:
        for door, call in doors.all:
            for args, want in [(([(0, 0, 0), (0, 0, len(files))], cw, ch, t.data_ptr(), cap), mic.MIC_ERR_ARGS),
                               (([(0, 0, 0), (0, 0, -1)], cw, ch, t.data_ptr(), cap), mic.MIC_ERR_ARGS),
                               ((xyf, 0, ch, t.data_ptr(), cap), mic.MIC_ERR_ARGS), ((xyf, cw, -2, t.data_ptr(), cap), mic.MIC_ERR_ARGS),
                               ((xyf, cw, ch, t.data_ptr(), cap - 1), mic.MIC_ERR_CAPACITY),
                               ((xyf, cw, ch, pageable.ctypes.data, cap), mic.MIC_ERR_ARGS),
                               ((many, cw, ch, t.data_ptr(), 16384 * ch * cw * 3), mic.MIC_ERR_ARGS)]:
                with pytest.raises(mic.MicError) as e:
                    call(*args)
                assert e.value.code == want, (door, args[1:], want)
            st, bad, stats = call([], cw, ch, t.data_ptr(), 0)               # n = 0: nothing to do, and that is no error
            assert st.size == 0 and stats == dict(planes_decoded=0, planes_total=0, pieces=0, slabs=0)
            assert (t.cpu().numpy() == 0xA5).all() and not pageable.any()    # none of the refused calls wrote a byte
            got, st, bad, stats = _read(call, xyf, cw, ch)
            assert np.array_equal(got, F.expected(files, xyf, cw, ch)) and (st == 0).all(), door
        doors.sess.set_timing(True)
        _read(doors.session, xyf, cw, ch)
        assert "k_rgb_gather_crops" in dict(doors.sess.last_timings())
    finally:
        doors.close()


def test_sub_batch_seams_in_a_child_process():
    """tests/rgb_crops_chunking_check.py in a fresh process with a 4 MiB workspace ceiling, as tests/test_gpu_rgb_batch.py's
    test_sub_batch_seams_in_a_child_process sets it.  A sub-batch takes coded planes while their number times
    (unit_ws_bytes(px) + 2 px), px the largest of them, stays under the ceiling; the tier-2 slabs of a plane of 80 x 60 = 4800 pixels
    are 4 * (4 px + 16) + 131104 + 2 * (4 px + 16) + 8 * (2 px + 8) + px / 8 + 26 * 65536 + 8192 = 2035992 bytes (the arithmetic
    of tests/test_gpu_strip_crops.py), 2045592 with its pixels: 4 MiB hold two planes and not three.  Six full-colour frames, three
    coded planes each, then go one frame a chain (a file is never cut): six chains; six grey frames, one coded plane each, two a
    chain: three.  Both calls are exact; the check asserts slabs(colour) >= 2 and slabs(grey) < slabs(colour)."""
    env = dict(os.environ, MIC_HIP_WS_BUDGET_MB="4")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rgb_crops_chunking_check.py")], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "rgb crop seams ok" in r.stdout, r.stdout + r.stderr
