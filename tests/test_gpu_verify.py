"""GPU tests of the verified encode, the verify door and the CRC-32 digests (mic_verify.hip; include/mic_hip.h, "verified encode").
Every comparison is exact; the references are zlib.crc32 and numpy, never the code under test."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def _crc(a):
    return zlib.crc32(np.ascontiguousarray(a).astype("<u2").tobytes())


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.int16).copy()).cuda()


def _blobs_to_host(mic, torch, d_blobs, nbytes):
    t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")
    mic.device_copy(t.data_ptr(), d_blobs, int(nbytes))
    return t.cpu().numpy()[: int(nbytes)]


def _lay_out(mic, frames, maxvs, nstates, lead=0):
    """the frames back to back from pixel `lead` on: (flat u16 array, unit table)"""
    flat = np.zeros(lead + sum(f.size for f in frames), dtype=np.uint16)
    units, off = [], lead
    for f, mv, ns in zip(frames, maxvs, nstates):
        h, w = f.shape
        flat[off:off + f.size] = f.reshape(-1)
        units.append((off, w, h, mv, ns))
        off += f.size
    return flat, mic.Session.make_units(units)


def _small(w, h, seed):
    """a small frame with few enough symbols to be coded (tests/test_gpu_host_path.py, _seam_jobs)"""
    rng = np.random.default_rng(seed)
    return ((np.arange(w * h).reshape(h, w) // 3) % 900 + rng.integers(0, 3, (h, w))).astype(np.uint16)


def _geometry_seams(mic):
    lane, wave, group = mic.verify_geometry()
    assert 0 < lane < wave < group
    return lane, wave, group


# ---- 1. digest seams ---------------------------------------------------------------------------------------------------------
def test_digest_equals_zlib_at_every_seam(mic, gpu_ready):
    torch = pytest.importorskip("torch")
    seams = _geometry_seams(mic)
    sizes = [1, 2, 3, 7, 8, 9, 63, 64, 65] + [g + d for g in seams for d in (-1, 0, 1)] + [2 * seams[2] - 1, 2 * seams[2] + 1]
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 65536, (1, n), dtype=np.uint16) for n in sizes]
    frames += [np.zeros((1, seams[1] + 5), np.uint16), np.full((1, seams[1] + 3), 0xFFFF, np.uint16), np.zeros((1, 1), np.uint16), np.full((1, 5), 0xFFFF, np.uint16)]
    # one batch mixing a 640 x 480 frame with one-pixel units
    frames += [rng.integers(0, 65536, (1, 1), dtype=np.uint16), rng.integers(0, 4096, (480, 640), dtype=np.uint16)]
    frames += [rng.integers(0, 65536, (1, 1), dtype=np.uint16) for _ in range(3)]
    seen = set()
    for lead in (0, 1, 3):                                             # (units back to back: every alignment of a unit's first and last byte)
        flat, units = _lay_out(mic, frames, [0] * len(frames), [2] * len(frames), lead)
        seen |= {int(u.px_offset) % 8 for u in units}
        d_px = _dev(torch, flat)
        sess = mic.Session(len(frames), 640 * 480)
        try:
            got = sess.digest(d_px.data_ptr(), units)
            again = sess.digest(d_px.data_ptr(), units)
        finally:
            sess.close()
        want = np.array([_crc(f) for f in frames], dtype=np.uint32)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, [(int(i), frames[i].size, hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]
        assert np.array_equal(got, again)
    assert seen == set(range(8))                                       # px_offset odd, and 1 .. 7 modulo 8


# ---- 2. verified encode agrees with encode -----------------------------------------------------------------------------------
def _flavour_frames(synth):
    ct = np.fromfile(os.path.join(GOLDEN, "CT_512_512_image.bin"), dtype="<u2").reshape(512, 512)
    mr = np.fromfile(os.path.join(GOLDEN, "MR_256_256_image.bin"), dtype="<u2").reshape(256, 256)
    frames = [ct, mr, synth.xr_like(cols=640, rows=480, depth=12, seed=31), synth.xr_like(cols=400, rows=300, depth=16, seed=32),
              synth.xr_like(cols=333, rows=211, depth=12, seed=33), _small(129, 7, 34)]
    maxvs = [int(ct.max()), int(mr.max()), 4095, 65535, 4095, 4095]
    return frames, maxvs


@pytest.mark.parametrize("flavour", ["2", "4", "8", "grad", "gap"])
def test_verified_encode_agrees_with_encode(mic, synth, gpu_ready, flavour):
    torch = pytest.importorskip("torch")
    frames, maxvs = _flavour_frames(synth)
    ns = {"2": 2, "4": 4, "8": 8, "grad": 2 | mic.MIC_HIP_PRED_GRAD, "gap": 2 | mic.MIC_HIP_GAP_REMOVAL}[flavour]
    flat, units = _lay_out(mic, frames, maxvs, [ns] * len(frames), lead=3)
    d_px = _dev(torch, flat)
    sess = mic.Session(len(frames), 512 * 512)
    try:
        d_blobs, offs, st, used = sess.encode(d_px.data_ptr(), units)
        assert not st.any(), st
        plain = _blobs_to_host(mic, torch, d_blobs, offs[-1]).copy()
        d_blobs2, offs2, used2, res = sess.encode_verified(d_px.data_ptr(), units)
        checked = _blobs_to_host(mic, torch, d_blobs2, offs2[-1])
    finally:
        sess.close()
    assert np.array_equal(offs, offs2) and np.array_equal(used, used2) and np.array_equal(plain, checked)
    for f, r in zip(frames, res):
        assert (r.status, r.mismatches, r.first_mismatch) == (mic.MIC_OK, 0, -1), r
        assert r.crc32 == _crc(f)


# ---- 3 / 4. altered samples are found exactly ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoded_batch(mic, synth, gpu_ready):
    """three 300 x 200 frames, encoded once: (frames, flat pixels, units, streams on the host, offsets)"""
    torch = pytest.importorskip("torch")
    frames = [synth.xr_like(cols=300, rows=200, depth=12, seed=50 + i) for i in range(3)]
    flat, units = _lay_out(mic, frames, [4095] * 3, [2] * 3, lead=1)
    sess = mic.Session(3, 300 * 200)
    try:
        d_px = _dev(torch, flat)
        d_blobs, offs, st, _ = sess.encode(d_px.data_ptr(), units)
        assert not st.any()
        blobs = _blobs_to_host(mic, torch, d_blobs, offs[-1]).copy()
    finally:
        sess.close()
    return frames, flat, units, blobs, offs


def _verify(mic, torch, sess, blobs, offs, units, ref_flat):
    d_blobs = torch.from_numpy(np.concatenate([blobs, np.zeros(64, np.uint8)])).cuda()   # (the decoder may read 64 bytes past a stream)
    d_ref = _dev(torch, ref_flat)
    return sess.verify(d_blobs.data_ptr(), offs, units, d_ref.data_ptr())


def test_one_altered_sample_is_found_exactly(mic, gpu_ready, encoded_batch):
    """One sample of the reference altered, at every position the issue names -- 0, 1, 7, 8, w - 1, w, the last pixel, and +-1 around
    every multiple of the kernel's lane, wave and group chunk inside the frame -- and, because the kernel cuts a unit from its END and
    units start at every alignment, at every position of the frame's first and last 200 pixels and +-9 around the wave and group seams
    counted from the end.  Many altered copies of the one frame go through each verify call, an untouched copy at either end."""
    torch = pytest.importorskip("torch")
    frames, flat, units, blobs, offs = encoded_batch
    w, h = 300, 200
    npx = w * h
    lane, wave, group = _geometry_seams(mic)
    positions = {0, 1, 7, 8, w - 1, w, npx - 1} | set(range(200)) | set(range(npx - 200, npx))
    for g in (lane, wave, group):
        for m in range(g, npx, g):
            positions |= {m - 1, m, m + 1}
    for g in (wave, group):
        for m in range(npx - g, 0, -g):
            positions |= set(range(m - 9, m + 10))
    positions = sorted(p for p in positions if 0 <= p < npx)
    frame = frames[1].reshape(-1)
    stream = blobs[int(offs[1]):int(offs[2])]
    want_ok = _crc(frame)
    per_call = 126
    sess = mic.Session(per_call + 2, npx)
    try:
        for i0 in range(0, len(positions), per_call):
            part = positions[i0:i0 + per_call]
            n = len(part) + 2
            unit_at = [1 + k * (npx + 1) for k in range(n)]              # (a stride of npx + 1: the copies start at every alignment)
            ref = np.zeros(unit_at[-1] + npx, dtype=np.uint16)
            for k in range(n):
                ref[unit_at[k]:unit_at[k] + npx] = frame
            for k, p in enumerate(part):
                ref[unit_at[k + 1] + p] ^= 0x0100
            table = mic.Session.make_units([(o, w, h, 4095, 2) for o in unit_at])
            many = np.tile(stream, n)
            many_offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(stream.size)
            res = _verify(mic, torch, sess, many, many_offs, table, ref)
            for k in (0, n - 1):
                assert (res[k].status, res[k].mismatches, res[k].first_mismatch, res[k].crc32) == (mic.MIC_OK, 0, -1, want_ok), (i0, k, res[k])
            for k, p in enumerate(part):
                r = res[k + 1]
                assert (r.status, r.mismatches, r.first_mismatch) == (mic.MIC_ERR_MISMATCH, 1, p), (p, r)
                assert r.crc32 == _crc(ref[unit_at[k + 1]:unit_at[k + 1] + npx]), p
    finally:
        sess.close()


def test_many_differences_are_counted_and_the_first_one_named(mic, synth, gpu_ready, encoded_batch):
    torch = pytest.importorskip("torch")
    frames, flat, units, blobs, offs = encoded_batch
    npx = 300 * 200
    lane, wave, group = _geometry_seams(mic)
    other = synth.xr_like(cols=300, rows=200, depth=12, seed=77)
    base = [int(u.px_offset) for u in units]
    ref = flat.copy()
    ref[base[0]:base[0] + npx] = other.reshape(-1)                      # unit 0: another frame of the same shape
    three = [npx - 1 - 2 * group - 5, npx - 1 - group - 9, npx - 4]     # unit 2: three samples in three different groups
    for p in three:
        ref[base[2] + p] += 1
    sess = mic.Session(3, npx)
    try:
        res = _verify(mic, torch, sess, blobs, offs, units, ref)
    finally:
        sess.close()
    a, b = frames[0].reshape(-1), other.reshape(-1)
    assert np.count_nonzero(a != b) > npx // 2
    assert (res[0].status, res[0].mismatches, res[0].first_mismatch) == (mic.MIC_ERR_MISMATCH, np.count_nonzero(a != b), np.flatnonzero(a != b)[0])
    assert res[0].crc32 == _crc(other)
    assert (res[1].status, res[1].mismatches, res[1].first_mismatch) == (mic.MIC_OK, 0, -1)
    assert (res[2].status, res[2].mismatches, res[2].first_mismatch) == (mic.MIC_ERR_MISMATCH, 3, min(three))


# ---- 5. codec errors are not mismatches --------------------------------------------------------------------------------------
def test_codec_errors_are_not_mismatches(mic, synth, gpu_ready, encoded_batch):
    torch = pytest.importorskip("torch")
    w, h = 300, 200
    plain = [synth.xr_like(cols=w, rows=h, depth=12, seed=60 + i) for i in range(3)]
    const = np.full((h, w), 1234, dtype=np.uint16)
    noise = (synth.hash_u64(w * h, 3) & np.uint64(0xFFFF)).astype(np.uint16).reshape(h, w)
    frames = [plain[0], const, plain[1], noise, plain[2]]
    flat, units = _lay_out(mic, frames, [4095, 4095, 4095, 65535, 4095], [2] * 5)
    d_px = _dev(torch, flat)
    sess = mic.Session(5, w * h)
    try:
        _, offs, st, _ = sess.encode(d_px.data_ptr(), units)
        _, offs2, _, res = sess.encode_verified(d_px.data_ptr(), units)
    finally:
        sess.close()
    assert st[1] != 0 and st[3] != 0 and st[0] == st[2] == st[4] == 0, st   # (the codec refuses the constant frame and the 16-bit noise frame)
    assert np.array_equal(offs, offs2)
    for k, (f, r) in enumerate(zip(frames, res)):
        assert r.status == st[k] and r.status != mic.MIC_ERR_MISMATCH, (k, r)
        assert (r.mismatches, r.first_mismatch, r.crc32) == (0, -1, _crc(f)), (k, r)
    # a truncated stream between two good ones: the decoder's status, nothing compared
    frames3, flat3, units3, blobs, offs = encoded_batch
    o = [int(x) for x in offs]
    cut = (o[2] - o[1]) // 2
    short = np.concatenate([blobs[:o[1] + cut], blobs[o[2]:]])
    offs_short = np.array([o[0], o[1], o[1] + cut, o[1] + cut + o[3] - o[2]], dtype=np.uint64)
    sess = mic.Session(3, w * h)
    try:
        d_blobs = torch.from_numpy(np.concatenate([short, np.zeros(64, np.uint8)])).cuda()
        d_out = torch.zeros(flat3.size, dtype=torch.int16, device="cuda")
        dec_st = sess.decode(d_blobs.data_ptr(), offs_short, units3, d_out.data_ptr())
        res = _verify(mic, torch, sess, short, offs_short, units3, flat3)
    finally:
        sess.close()
    assert dec_st[1] != 0 and dec_st[0] == dec_st[2] == 0, dec_st
    assert (res[1].status, res[1].mismatches, res[1].first_mismatch, res[1].crc32) == (dec_st[1], 0, -1, _crc(frames3[1]))
    for k in (0, 2):
        assert (res[k].status, res[k].mismatches, res[k].crc32) == (mic.MIC_OK, 0, _crc(frames3[k]))


# ---- 6. tier retry -----------------------------------------------------------------------------------------------------------
def test_verified_encode_through_the_tier_retry(mic, synth, gpu_ready):
    torch = pytest.importorskip("torch")
    from test_gpu_workspace_tiers import _escape_frame
    w, h, maxv = 640, 480, 4095
    frames = [synth.xr_like(cols=w, rows=h, depth=12, seed=40), _escape_frame(w, h, maxv), synth.xr_like(cols=w, rows=h, depth=12, seed=41)]
    flat, units = _lay_out(mic, frames, [maxv] * 3, [2] * 3)
    d_px = _dev(torch, flat)
    sess = mic.Session(3, w * h)
    try:
        assert not sess.workspace_bytes()[1]
        runs = []
        for call in range(2):
            d_blobs, offs, used, res = sess.encode_verified(d_px.data_ptr(), units)
            assert sess.workspace_bytes()[1]                            # the escape frame did not fit tier 1: the batch ran again in tier 2
            for f, r in zip(frames, res):
                assert (r.status, r.mismatches, r.first_mismatch, r.crc32) == (mic.MIC_OK, 0, -1, _crc(f)), (call, r)
            runs.append((offs.copy(), used.copy(), _blobs_to_host(mic, torch, d_blobs, offs[-1]).copy()))
        assert all(np.array_equal(x, y) for x, y in zip(runs[0], runs[1]))
        held = sess.workspace_bytes()[0]
        assert held >= flat.nbytes                                      # (the scratch pixels are counted)
    finally:
        sess.close()


# ---- 7. host doors -----------------------------------------------------------------------------------------------------------
def host_door_checks(mic, synth):
    """What test 7 asks of the four host doors; runs in this process, in a child under a small workspace, and over two shards."""
    imgs = [synth.xr_like(cols=322, rows=211, depth=12, seed=200 + i) for i in range(5)] + [_small(129, 77, 9)]
    dims = [(i.shape[1], i.shape[0]) for i in imgs]
    want_crc = [_crc(i) for i in imgs]
    # single frames
    plain = mic.compress_batch(imgs, [4095] * len(imgs), 2)
    checked = mic.compress_batch_verified(imgs, [4095] * len(imgs), 2)
    for (st, blob, used), (st2, blob2, used2, r), c in zip(plain, checked, want_crc):
        assert st == st2 == 0 and blob == blob2 and used == used2
        assert (r.status, r.crc32, r.mismatches, r.first_mismatch) == (0, c, 0, -1)
    blobs = [b for _, b, _ in plain]
    out = mic.decompress_batch_crc(blobs, dims)
    for img, (st, px, crc), c in zip(imgs, out, want_crc):
        assert st == 0 and np.array_equal(px, img) and crc == c
    expect = list(want_crc)
    expect[2] ^= 1
    out = mic.decompress_batch_crc(blobs, dims, expect=expect)
    for k, (img, (st, px, crc)) in enumerate(zip(imgs, out)):
        assert st == (mic.MIC_ERR_MISMATCH if k == 2 else 0) and np.array_equal(px, img) and crc == want_crc[k], k
    # PICS: 211 rows in 1, 3 and 8 strips (8 does not divide them)
    for strips in (1, 3, 8):
        plain = mic.compress_parallel_strips_batch(imgs, 4095, strips, 2)
        checked = mic.pics_compress_batch_verified(imgs, 4095, strips, 2)
        files = []
        for (st, f), (st2, f2, r, bad), c in zip(plain, checked, want_crc):
            assert st == st2 == 0 and f.tobytes() == f2.tobytes() and bad == -1, strips
            assert (r.status, r.crc32, r.mismatches, r.first_mismatch) == (0, c, 0, -1), strips
            files.append(f.tobytes())
        out = mic.pics_decompress_batch_crc(files, dims)
        for img, (st, px, crc), c in zip(imgs, out, want_crc):
            assert st == 0 and np.array_equal(px, img) and crc == c, strips
        expect = list(want_crc)
        expect[4] ^= 0x80000000
        out = mic.pics_decompress_batch_crc(files, dims, expect=expect)
        for k, (img, (st, px, crc)) in enumerate(zip(imgs, out)):
            assert st == (mic.MIC_ERR_MISMATCH if k == 4 else 0) and np.array_equal(px, img) and crc == want_crc[k], (strips, k)


def test_host_doors(mic, synth, gpu_ready):
    host_door_checks(mic, synth)


def test_host_doors_over_two_shards(mic, synth, gpu_ready):
    before = mic.get_devices()
    mic.set_devices([0, 0])
    try:
        host_door_checks(mic, synth)
    finally:
        mic.set_devices(before)


_CHILD = r'''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import __graft_entry__ as e
mic = e.load_package()
import importlib
synth = importlib.import_module("medical_image_codec_amd.synth")
import test_gpu_verify as t
t.host_door_checks(mic, synth)
print("ok")
''' % (ROOT, os.path.join(ROOT, "tests"))


def test_host_doors_under_a_small_workspace(gpu_ready):
    """a child process with a workspace ceiling of 8 MB (read once per process): the verified doors walk several sub-batches --
    MIC_HIP_TRACE=1 names the parts -- and say the same"""
    import re
    env = dict(os.environ, MIC_HIP_WS_BUDGET_MB="8", MIC_HIP_TRACE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    for what in ("encode", "decode"):
        parts = [int(n) for k, n in re.findall(r"\[mic_hip units %s\] part (\d+) of (\d+):" % what, r.stderr) if k == "1"]
        assert parts and min(parts) >= 2, (what, parts)
