"""GPU tests of the host-pointer path (mic_host_io.hip): the batch entry points over ordinary and pinned host memory, the
sub-batch pipeline, and concurrent callers (the header promises what ojph/mic_parallel.h:47-48 promises: any thread, any time).
Everything is compared with the oracle, bit for bit."""
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _images(synth, n, w=322, h=256, depth=12):
    return [synth.xr_like(cols=w, rows=h, depth=depth, seed=100 + i) for i in range(n)]


def test_pics_batch_equals_single_calls_and_the_oracle(mic, mico, synth, gpu_ready):
    # mixed shapes in one call; the last image is one the reference cannot code (a 1290-pixel strip of 10-bit noise has more
    # distinct symbols than table slots: normalizeCount2 spins) -- the job fails, its neighbours do not
    rng = np.random.default_rng(3)
    ramp = ((np.arange(77 * 129).reshape(77, 129) // 3) % 900 + rng.integers(0, 3, (77, 129))).astype(np.uint16)
    imgs = _images(synth, 5) + [ramp, synth.xr_like(cols=257, rows=200, depth=12, seed=9), synth.xr_like(cols=129, rows=77, depth=10, seed=7)]
    maxv = 4095
    res = mic.compress_parallel_strips_batch(imgs, maxv, 8, 2)
    files, good = [], []
    for img, (st, blob) in zip(imgs, res):
        rc, want = mico.pics_compress(img, maxv, 8, 2)
        assert st == rc
        if rc == 0:
            assert blob.tobytes() == want
            assert blob.tobytes() == mic.compress_parallel_strips(img, img.shape[1], img.shape[0], maxv, 8)
            files.append(blob.tobytes()); good.append(img)
    assert len(good) == 7
    out = mic.decompress_parallel_strips_batch(files, [(i.shape[1], i.shape[0]) for i in good])
    for img, (st, px) in zip(good, out):
        assert st == 0 and np.array_equal(px, img)


def test_pics_batch_reports_errors_per_job(mic, mico, synth, gpu_ready):
    imgs = _images(synth, 3)
    rc, good = mico.pics_compress(imgs[0], 4095, 4, 2)
    bad_magic = b"XXXX" + good[4:]
    truncated = good[: len(good) // 2]
    out = mic.decompress_parallel_strips_batch([good, bad_magic, truncated, good], [(322, 256)] * 4)
    assert out[0][0] == 0 and np.array_equal(out[0][1], imgs[0])
    assert out[1][0] == mic.MIC_ERR_CORRUPT and out[2][0] == mic.MIC_ERR_CORRUPT
    assert out[3][0] == 0 and np.array_equal(out[3][1], imgs[0])
    # a too-small output buffer fails that job only
    small = [np.empty(64, dtype=np.uint8), np.empty(mic.pics_bound(322, 256, 8), dtype=np.uint8)]
    res = mic.compress_parallel_strips_batch(imgs[:2], 4095, 8, 2, outs=small)
    assert res[0][0] == mic.MIC_ERR_CAPACITY and res[1][0] == 0
    assert res[1][1].tobytes() == mico.pics_compress(imgs[1], 4095, 8, 2)[1]


def test_pinned_buffers_take_the_direct_path(mic, mico, synth, gpu_ready):
    img = synth.xr_like(cols=640, rows=512, depth=12, seed=3)
    src = mic.host_alloc(img.nbytes, np.uint16).reshape(img.shape)
    src[...] = img
    dst = mic.host_alloc(mic.pics_bound(640, 512, 8))
    try:
        (st, blob), = mic.compress_parallel_strips_batch([src], 4095, 8, 2, outs=[dst])
        assert st == 0 and blob.tobytes() == mico.pics_compress(img, 4095, 8, 2)[1]
        back = mic.host_alloc(img.nbytes, np.uint16)
        (st, px), = mic.decompress_parallel_strips_batch([blob], [(640, 512)], outs=[back])
        assert st == 0 and np.array_equal(px, img)
        mic.host_free(back)
    finally:
        mic.host_free(src[1:, 3:]); mic.host_free(dst)                   # (any view names its allocation: ADVICE r3)
    with pytest.raises(ValueError):
        mic.host_free(src)                                               # freed already
    with pytest.raises(ValueError):
        mic.host_free(np.zeros(16, dtype=np.uint8))                      # never pinned


_CHILD_HEAD = r'''
import sys, numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as e
mic = e.load_package()
import importlib
synth = importlib.import_module("medical_image_codec_amd.synth")
from oracle import mico
''' % ROOT


def _parts_per_call(stderr, what):
    """[the number of parts of each call] from the '[mic_hip units <what>] part k of n: ...' lines of MIC_HIP_TRACE=1"""
    lines = re.findall(r"\[mic_hip units %s\] part (\d+) of (\d+):" % what, stderr)
    return [int(n) for k, n in lines if k == "1"]


WS_BUDGET_MB = 8


def test_sub_batch_pipeline_under_a_small_workspace(mic, mico, synth):
    """A child process with a workspace ceiling of WS_BUDGET_MB: every call walks several sub-batches (both staging halves, the
    packed-buffer swap, the wait for the download of sub-batch k - 2); results must not depend on the cut.  MIC_HIP_TRACE=1 makes the
    library name its parts on stderr: each of the four calls must really have been cut into three parts or more.
    Observed on an MI355X at 8 MB: PICS encode 6 parts, PICS decode 6, frame encode 3, frame decode 3."""
    code = _CHILD_HEAD + r'''
imgs = [synth.xr_like(cols=322, rows=256, depth=12, seed=200 + i) for i in range(9)]
res = mic.compress_parallel_strips_batch(imgs, 4095, 8, 2)
files = []
for img, (st, blob) in zip(imgs, res):
    assert st == 0 and blob.tobytes() == mico.pics_compress(img, 4095, 8, 2)[1]
    files.append(blob.tobytes())
out = mic.decompress_parallel_strips_batch(files, [(322, 256)] * 9)
for img, (st, px) in zip(imgs, out):
    assert st == 0 and np.array_equal(px, img)
jobs = mic.compress_batch(imgs, [4095] * 9, 4)
for img, (st, blob, used) in zip(imgs, jobs):
    rc, want = mico.compress_single_frame(img, 4095, 4)
    assert st == 0 and blob == want
back = mic.decompress_batch([b for _, b, _ in jobs], [(322, 256)] * 9)
for img, (st, px) in zip(imgs, back):
    assert st == 0 and np.array_equal(px, img)
print("ok")
'''
    env = dict(os.environ, MIC_HIP_WS_BUDGET_MB=str(WS_BUDGET_MB), MIC_HIP_TRACE="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    enc, dec = _parts_per_call(r.stderr, "encode"), _parts_per_call(r.stderr, "decode")
    print("parts per call: encode", enc, "decode", dec)
    assert len(enc) == 2 and len(dec) == 2 and min(enc + dec) >= 3, (enc, dec, r.stderr)   # (PICS, frames)


def _seam_jobs(synth):
    """nine jobs of mixed sizes, 8 strips each: with three forced parts the cuts fall after jobs 2 and 5"""
    def small(seed):                                                     # 129 x 77 with few enough symbols per ten-row strip to be coded
        rng = np.random.default_rng(seed)
        return ((np.arange(77 * 129).reshape(77, 129) // 3) % 900 + rng.integers(0, 3, (77, 129))).astype(np.uint16)
    shapes = [(322, 256), (257, 200)]
    imgs = [small(300 + i) if i % 3 == 2 else synth.xr_like(cols=shapes[i % 3][0], rows=shapes[i % 3][1], depth=12, seed=300 + i) for i in range(9)]
    imgs[7] = synth.xr_like(cols=129, rows=77, depth=10, seed=7)         # noise: the reference cannot code it (test_pics_batch_equals_...)
    return imgs


SEAM_SMALL_JOB, SEAM_SMALL_CAP, SEAM_PINNED_JOB = 4, 1024, 0               # job 4's buffer holds its header and no more than a strip: the middle part


def test_three_forced_parts_with_failing_jobs_in_a_child_process(mic, mico, synth, gpu_ready, tmp_path):
    """MIC_HIP_PIPELINE_PARTS=3 (read once: a child process): one PICS batch call over nine jobs of mixed sizes, one of them with
    too small a buffer in the middle part, one that the reference cannot code, one in pinned memory.  Every status and every good
    file equals the oracle's and the uncut call's of this process; the good files come back exact through the batch decoder in the
    same child; MIC_HIP_TRACE=1 shows three parts for both calls."""
    code = _CHILD_HEAD + r'''
sys.path.insert(0, %r)
import test_gpu_host_path as t
imgs = t._seam_jobs(synth)
st, blobs = t._seam_encode(mic, imgs)
np.savez(sys.argv[1], status=np.array(st), **{"f%%d" %% i: b for i, b in enumerate(blobs)})
good = [i for i in range(len(imgs)) if st[i] == 0]
out = mic.decompress_parallel_strips_batch([blobs[i].tobytes() for i in good], [(imgs[i].shape[1], imgs[i].shape[0]) for i in good])
for i, (rc, px) in zip(good, out):
    assert rc == 0 and np.array_equal(px, imgs[i]), i
print("ok")
''' % os.path.join(ROOT, "tests")
    npz = str(tmp_path / "cut.npz")
    env = dict(os.environ, MIC_HIP_PIPELINE_PARTS="3", MIC_HIP_TRACE="1")
    r = subprocess.run([sys.executable, "-c", code, npz], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    assert _parts_per_call(r.stderr, "encode") == [3] and _parts_per_call(r.stderr, "decode") == [3], r.stderr
    cut = np.load(npz)
    imgs = _seam_jobs(synth)
    st, blobs = _seam_encode(mic, imgs)                                   # the uncut call
    for i, img in enumerate(imgs):
        rc, want = mico.pics_compress(img, 4095, 8, 2)
        if i == SEAM_SMALL_JOB:
            assert rc == 0 and len(want) > SEAM_SMALL_CAP
            rc = mic.MIC_ERR_CAPACITY
        assert cut["status"][i] == rc == st[i], i
        if rc == 0:
            assert cut["f%d" % i].tobytes() == want == blobs[i].tobytes(), i
    assert sorted(i for i in range(9) if st[i] != 0) == [SEAM_SMALL_JOB, 7]


def _seam_encode(mic, imgs):
    """the seam jobs through one compress_parallel_strips_batch call: ([status], [file bytes])"""
    imgs = list(imgs)
    outs = [np.empty(SEAM_SMALL_CAP if i == SEAM_SMALL_JOB else mic.pics_bound(a.shape[1], a.shape[0], 8), dtype=np.uint8) for i, a in enumerate(imgs)]
    src = mic.host_alloc(imgs[SEAM_PINNED_JOB].nbytes, np.uint16).reshape(imgs[SEAM_PINNED_JOB].shape)
    dst = mic.host_alloc(outs[SEAM_PINNED_JOB].size)
    try:
        src[...] = imgs[SEAM_PINNED_JOB]
        imgs[SEAM_PINNED_JOB], outs[SEAM_PINNED_JOB] = src, dst
        res = mic.compress_parallel_strips_batch(imgs, 4095, 8, 2, outs=outs)
        return [st for st, _ in res], [blob.copy() for _, blob in res]
    finally:
        mic.host_free(src); mic.host_free(dst)


def test_concurrent_callers_default_pool_and_sessions(mic, mico, synth, gpu_ready):
    """Eight Python threads (ctypes releases the GIL) hammer the host-pointer entry points -- they share the pool of default sessions
    -- while two more drive explicit sessions on the same device; every result is compared with the oracle."""
    import torch
    imgs = _images(synth, 6)
    want_pics = [mico.pics_compress(i, 4095, 8, 2)[1] for i in imgs]
    want_frame = [mico.compress_single_frame(i, 4095, 4)[1] for i in imgs]
    ct = np.fromfile(os.path.join(ROOT, "tests", "golden", "CT_512_512_image.bin"), dtype="<u2").reshape(512, 512)
    want_ct = mico.compress_single_frame(ct, int(ct.max()), 2)[1]
    errors = []

    def host_worker(k):
        try:
            for it in range(6):
                i = (k + it) % len(imgs)
                blob = mic.compress_parallel_strips(imgs[i], 322, 256, 4095, 8)
                assert blob == want_pics[i], "pics bytes"
                px, w, h = mic.decompress_parallel_strips(blob)
                assert np.array_equal(px, imgs[i]), "pics pixels"
                (st, fb, used), = mic.compress_batch([imgs[i]], [4095], 4)
                assert st == 0 and fb == want_frame[i], "frame bytes"
                if it % 3 == 0:
                    assert mic.compress_single_frame(ct, 512, 512, int(ct.max()), 2) == want_ct, "ct bytes"
                res = mic.compress_parallel_strips_batch([imgs[i], imgs[(i + 1) % len(imgs)]], 4095, 8, 2)
                assert res[0][1].tobytes() == want_pics[i] and res[1][1].tobytes() == want_pics[(i + 1) % len(imgs)], "batch bytes"
        except Exception as e:  # noqa: BLE001
            errors.append(f"host {k}: {e!r}")

    def session_worker(k):
        try:
            d_px = torch.from_numpy(np.stack(imgs).view(np.int16)).cuda()
            d_out = torch.empty_like(d_px)
            units = [(f * 322 * 256 + y0 * 322, 322, 32, 4095, 2) for f in range(len(imgs)) for y0 in range(0, 256, 32)]
            sess = mic.Session(len(units), 322 * 32)
            cu = mic.Session.make_units(units)
            for it in range(5):
                sess.encode_enqueue(d_px.data_ptr(), cu)
                d_blobs, offs, st, ns = sess.encode_finish()
                assert (st == 0).all()
                blobs = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda")
                mic.device_copy(blobs.data_ptr(), d_blobs, int(offs[-1]))
                host = blobs.cpu().numpy()
                for f in range(len(imgs)):                                     # strips of frame f = the payload of its PICS-8 file
                    a, b = int(offs[f * 8]), int(offs[f * 8 + 8])
                    assert host[a:b].tobytes() == want_pics[f][20 + 64:], "session bytes"
                sess.decode_enqueue(d_blobs, offs, cu, d_out.data_ptr())
                assert (sess.decode_finish() == 0).all()
                assert torch.equal(d_out, d_px), "session pixels"
            sess.close()
        except Exception as e:  # noqa: BLE001
            errors.append(f"session {k}: {e!r}")

    threads = [threading.Thread(target=host_worker, args=(k,)) for k in range(8)] + \
              [threading.Thread(target=session_worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
