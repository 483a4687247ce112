"""MIC2 whole-volume batches on the GPU: mic_hip_mic2_compress_batch / _decompress_batch and mic_hip_session_mic2_encode / _decode
against the single calls (and through them the oracle): every file byte for byte, every volume sample for sample, a volume that
fails alone, the files closed into a loop on the device, and the fan-out over device lists."""
import struct

import numpy as np
import pytest
import torch

import mic2_batch_volumes as B
import mic2_crop_volumes as V
import mic2_multi_volumes as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(mic, mico, synth, gpu_ready):
    """the volumes, and the single calls' files of the eight jobs -- computed once, never written to"""
    vols = B.volumes(synth)
    jobs = [(vols[k][0], vols[k][1], t) for k, t in B.JOBS]
    files = []
    for vol, maxv, t in jobs:
        code, f = B.single_encode(mic, vol, maxv, t)
        assert code == 0
        rc, o = mico.mic2_compress(vol, maxv, temporal=t)
        assert rc == 0 and o == f                                                           # the single call is the oracle's file
        files.append(f)
    return dict(vols=vols, jobs=jobs, files=files)


def _encode(mic, jobs, **kw):
    return mic.compress_multi_frame_batch([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs], **kw)


def _device_volumes(jobs):
    """the volumes back to back in one device tensor: (tensor, [(px_off, w, h, n, max_value, temporal)])"""
    flat = np.concatenate([j[0].reshape(-1) for j in jobs])
    off, desc = 0, []
    for vol, maxv, t in jobs:
        desc.append((off, vol.shape[2], vol.shape[1], vol.shape[0], maxv, t))
        off += vol.size
    return torch.from_numpy(flat.view(np.int16)).cuda(), desc


def _fetch(mic, d_ptr, nbytes):
    t = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    mic.device_copy(t.data_ptr(), d_ptr, nbytes)
    return t.cpu().numpy()[:nbytes].tobytes()


def test_every_file_equals_the_single_call(mic, ref):
    jobs, files = ref["jobs"], ref["files"]
    res, stats = _encode(mic, jobs)
    for (st, bad, f), want in zip(res, files):
        assert (st, bad) == (0, -1) and f == want
    assert stats == dict(units=sum(j[0].shape[0] for j in jobs), slabs=1, volumes_done=len(jobs))
    cuts, nunits = mic.mic2_batch_plan([(j[0].shape[2], j[0].shape[1], j[0].shape[0]) for j in jobs])
    assert len(cuts) - 1 == stats["slabs"] and nunits == stats["units"]
    # the same volumes from device memory: the files back to back on the device, their heads on the host
    d_px, desc = _device_volumes(jobs)
    sess = mic.Session(4, 160 * 96)
    d_files, offs, heads, st, bad, sstats = sess.mic2_encode(d_px.data_ptr(), desc)
    assert (st == 0).all() and (bad == -1).all() and sstats == stats
    assert offs.tolist() == np.cumsum([0] + [len(f) for f in files]).tolist()
    assert _fetch(mic, d_files, int(offs[-1])) == b"".join(files)
    assert heads == [B.Mic2File(f).head() for f in files]
    sess.close()


def test_both_decode_doors_write_every_sample(mic, ref):
    jobs, files = ref["jobs"], ref["files"]
    outs = [np.full(j[0].size, 0xA5A5, dtype=np.uint16) for j in jobs]
    res, stats = mic.decompress_multi_frame_batch(files, outs=outs)
    assert stats == dict(units=sum(j[0].shape[0] for j in jobs), slabs=1, volumes_done=len(jobs))
    for (st, bad, dims, px), (vol, maxv, t), out in zip(res, jobs, outs):
        assert (st, bad) == (0, -1) and dims == (vol.shape[2], vol.shape[1], vol.shape[0], int(t))
        assert np.array_equal(px, vol) and np.array_equal(out.reshape(vol.shape), vol)
    # the files on the device, back to back: every one but the first starts at whatever byte the one before it leaves
    blob = b"\x00" + b"".join(files)
    starts = np.cumsum([1] + [len(f) for f in files])[:-1]
    assert any(s % 4 for s in starts) and any(s % 2 for s in starts)
    d_blob = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    px_off = np.cumsum([0] + [j[0].size for j in jobs])
    d_out = torch.full((int(px_off[-1]) * 2,), 0xA5, dtype=torch.uint8, device="cuda")
    sess = mic.Session(4, 160 * 96)
    st, bad, sstats = sess.mic2_decode([B.Mic2File(f).head() for f in files], [d_blob.data_ptr() + int(s) for s in starts],
                                       [len(f) for f in files], d_out.data_ptr(), px_off[:-1], int(px_off[-1]))
    assert (st == 0).all() and (bad == -1).all() and sstats == stats
    got = d_out.cpu().numpy().view("<u2")
    assert np.array_equal(got, np.concatenate([j[0].reshape(-1) for j in jobs]))
    sess.close()


def test_the_loop_closes_on_the_device(mic, ref):
    """Session.mic2_encode's files, heads and offsets go unchanged into Session.mic2_decode and Session.mic2_multi_read_crops"""
    jobs = ref["jobs"]
    d_px, desc = _device_volumes(jobs)
    enc, dec = mic.Session(4, 160 * 96), mic.Session(4, 160 * 96)                           # (the files live until the ENCODING session's next call)
    d_files, offs, heads, st, bad, _ = enc.mic2_encode(d_px.data_ptr(), desc)
    assert (st == 0).all()
    ptrs = [d_files + int(o) for o in offs[:-1]]
    lens = [int(b - a) for a, b in zip(offs, offs[1:])]
    px_off = [d[0] for d in desc]
    d_out = torch.full((d_px.numel() * 2,), 0xA5, dtype=torch.uint8, device="cuda")
    st, bad, stats = dec.mic2_decode(heads, ptrs, lens, d_out.data_ptr(), px_off, d_px.numel())
    assert (st == 0).all() and stats["slabs"] == 1 and stats["volumes_done"] == len(jobs)
    assert torch.equal(d_out.view(torch.int16), d_px)
    cw, ch, cd = V.SHAPES[0]
    per = [V.origins(j[0].shape[2], j[0].shape[1], j[0].shape[0], cw, ch, cd)[:6] for j in jobs]
    xyzv = M.interleave(per)
    t = torch.full((len(xyzv), cd, ch, cw, 2), 0xA5, dtype=torch.uint8, device="cuda")
    cst, cbad, _ = dec.mic2_multi_read_crops(heads, ptrs, lens, xyzv, cw, ch, cd, t.data_ptr(), t.numel())
    assert (cst == 0).all()
    assert np.array_equal(t.cpu().numpy().view("<u2")[..., 0], M.expected_multi([j[0] for j in jobs], xyzv, cw, ch, cd))
    enc.close(); dec.close()


def test_a_volume_fails_alone_on_encode(mic, ref):
    vols, jobs, files = ref["vols"], ref["jobs"], ref["files"]
    refused = [("still", True), ("col", False), ("col", True), ("row", False)]
    extra, want = [], []
    for k, t in refused:
        vol, maxv = vols[k]
        code, _ = B.single_encode(mic, vol, maxv, t)
        assert code != 0, k                                                                 # (the single call refuses each of them: an all-zero residual, frames that code larger than raw)
        extra.append((vol, maxv, t))
        want.append((code, B.first_refused_frame(mic, vol, maxv, t)))
    assert want[0][1] == 1                                                                  # "still": the first all-zero residual
    batch = jobs[:3] + extra[:2] + jobs[3:6] + extra[2:] + jobs[6:]
    where = [3, 4, 8, 9]
    res, stats = _encode(mic, batch)
    good = [i for i in range(len(batch)) if i not in where]
    for i, w in zip(where, want):
        assert res[i][:2] == w and res[i][2] is None, (i, res[i][:2], w)
    for i, f in zip(good, files):
        assert res[i][:2] == (0, -1) and res[i][2] == f, i
    assert stats["volumes_done"] == len(jobs) and stats["units"] == sum(b[0].shape[0] for b in batch)
    # the same on the device: a refused volume's range is empty, the files around it are exact
    d_px, desc = _device_volumes(batch)
    sess = mic.Session(4, 160 * 96)
    d_files, offs, heads, st, bad, _ = sess.mic2_encode(d_px.data_ptr(), desc)
    for i, w in zip(where, want):
        assert (st[i], bad[i]) == w and offs[i + 1] == offs[i] and heads[i] is None
    assert _fetch(mic, d_files, int(offs[-1])) == b"".join(files)
    assert [int(offs[i + 1] - offs[i]) for i in good] == [len(f) for f in files]
    sess.close()
    # a capacity one byte short, a NULL pointer, dimensions of 0: each alone
    caps = [None] * len(jobs)
    caps[2] = len(files[2]) - 1
    caps[4] = 20 + 8 * jobs[4][0].shape[0] - 1                                              # (not even the table)
    res, stats = _encode(mic, jobs, caps=caps)
    for i, f in enumerate(files):
        if i in (2, 4):
            assert res[i] == (mic.MIC_ERR_CAPACITY, -1, None), i
        else:
            assert res[i] == (0, -1, f), i
    res, stats = mic.compress_multi_frame_batch([jobs[0][0], None, jobs[1][0]], [jobs[0][1], 4095, jobs[1][1]], [jobs[0][2], True, jobs[1][2]])
    assert res[0] == (0, -1, files[0]) and res[1] == (mic.MIC_ERR_ARGS, -1, None) and res[2] == (0, -1, files[1])
    assert stats == dict(units=jobs[0][0].shape[0] + jobs[1][0].shape[0], slabs=1, volumes_done=2)
    assert mic.compress_multi_frame_batch([], [], []) == ([], dict(units=0, slabs=0, volumes_done=0))


def test_a_volume_fails_alone_on_decode(mic, ref):
    jobs, files = ref["jobs"], ref["files"]
    damaged = B.damage(files[0], 5)
    code, dec = B.single_decode(mic, damaged)
    truncated = files[3][: len(files[3]) - 10]
    magic = b"MIC3" + files[4][4:]
    past = bytearray(files[6])
    struct.pack_into("<I", past, 20 + 8 * 1 + 4, len(files[6]))                             # frame 1's length points past the end
    empty = bytearray(files[7])
    struct.pack_into("<I", empty, 20 + 8 * 2 + 4, 0)                                        # frame 2's length is 0
    batch = [damaged, files[1], files[2], truncated, magic, files[5], bytes(past), bytes(empty), None, files[3]]
    singles = [B.single_decode(mic, f)[0] if f is not None else mic.MIC_ERR_ARGS for f in batch]
    assert singles[1] == singles[2] == singles[5] == singles[9] == 0 and all(singles[i] != 0 for i in (3, 4, 6, 7))
    res, stats = mic.decompress_multi_frame_batch(batch)
    source = {1: jobs[1][0], 2: jobs[2][0], 5: jobs[5][0], 9: jobs[3][0]}
    for i, (st, bad, dims, px) in enumerate(res):
        assert st == singles[i], (i, st, singles[i])
        if i in source:
            assert bad == -1 and np.array_equal(px, source[i]), i
    if code:
        assert res[0][1] == 5
    else:
        assert np.array_equal(res[0][3], dec)
    assert res[6][1] == 1 and res[7][1] == 2 and res[3][1] >= 0 and res[4][1] == -1 and res[8][1] == -1
    assert stats["volumes_done"] == sum(s == 0 for s in singles)
    # the same files on the device
    ok = [i for i, f in enumerate(batch) if f is not None]
    blobs = [torch.from_numpy(np.frombuffer(batch[i], dtype=np.uint8).copy()).cuda() for i in ok]
    heads = [bytes(batch[i][: 20 + 8 * 16]) for i in ok]                                    # (more than any of these tables: the call takes what it needs)
    sizes = [jobs[k][0].size for k in (0, 1, 2, 3, 4, 5, 6, 7, 3)]
    px_off = np.cumsum([0] + sizes)
    d_out = torch.zeros(int(px_off[-1]), dtype=torch.int16, device="cuda")
    sess = mic.Session(4, 160 * 96)
    st, bad, _ = sess.mic2_decode(heads, [b.data_ptr() for b in blobs], [len(batch[i]) for i in ok], d_out.data_ptr(), px_off[:-1], int(px_off[-1]))
    got = d_out.cpu().numpy().view(np.uint16)
    for k, i in enumerate(ok):
        assert st[k] == singles[i], (i, st[k])
        if i in source:
            assert np.array_equal(got[px_off[k]: px_off[k + 1]], source[i].reshape(-1)), i
    if code:
        assert bad[0] == 5
    else:
        assert np.array_equal(got[: px_off[1]], dec.reshape(-1))
    # a volume that would end behind the output is MIC_ERR_CAPACITY alone
    st, bad, _ = sess.mic2_decode(heads[1:3], [blobs[1].data_ptr(), blobs[2].data_ptr()], [len(batch[1]), len(batch[2])], d_out.data_ptr(),
                                  [0, sizes[1]], sizes[1] + sizes[2] - 1)
    assert st.tolist() == [0, mic.MIC_ERR_CAPACITY]
    sess.close()


@pytest.fixture
def device_lists(mic, gpu_ready):
    yield ([0, 0], [0, 0, 0])
    mic.set_devices([0])


def test_batches_over_device_lists(mic, ref, device_lists):
    """As the other batches are tested: {0, 0} and {0, 0, 0} -- the fan-out with two and three sessions of one device, a shard
    boundary between volumes -- give the one-device files and pixels."""
    jobs, files = ref["jobs"], ref["files"]
    for devs in device_lists:
        mic.set_devices(devs)
        res, stats = _encode(mic, jobs)
        assert [r[2] for r in res] == files, devs
        assert stats["volumes_done"] == len(jobs) and 1 <= stats["slabs"] <= len(devs), devs
        back, stats = mic.decompress_multi_frame_batch(files)
        for (st, bad, dims, px), (vol, _, _) in zip(back, jobs):
            assert st == 0 and np.array_equal(px, vol), devs
        assert 1 <= stats["slabs"] <= len(devs), devs
