"""WaveletV2 frames of any shapes and level counts in ONE batch call (mic_hip_wavelet_v2_compress_jobs / _decompress_jobs, the mixed
session forms): every launch of csrc/mic_wavelet.hip is driven by a table of the frames.  Every file is the oracle's byte for byte,
every decoded image the oracle's; a reduced level is what the single call wavelet_v2_decompress_level gives for that file."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import wavelet_mixed_frames as F
from conftest import ROOT

pytestmark = pytest.mark.gpu

ONE = dict(sub_batches=1, chains=1)


def _stats(stats, **want):
    assert {k: stats[k] for k in want} == want, stats


def _oracle(mico, jobs):
    """[(rc, file)] of the oracle"""
    return [mico.wavelet_v2_compress(img, mv, lv) for img, mv, lv in jobs]


def _roundtrip(mic, mico, jobs, name, enc_stats=ONE, dec_stats=ONE):
    """one compress call, one decompress call of the oracle's files: bytes and pixels are the oracle's; a frame the oracle refuses
    carries the oracle's code alone"""
    want = _oracle(mico, jobs)
    res, stats = mic.wavelet_v2_compress_jobs([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
    _stats(stats, frames_done=sum(rc == 0 for rc, _ in want), redo_frames=0, **enc_stats)
    for k, ((st, f, applied), (rc, wf)) in enumerate(zip(res, want)):
        assert st == rc, (name, k, st, rc)
        if rc == 0:
            assert f == wf and applied == wf[10], (name, k, jobs[k][0].shape)
    good = [k for k, (rc, _) in enumerate(want) if rc == 0]
    back, stats = mic.wavelet_v2_decompress_jobs([want[k][1] for k in good])
    _stats(stats, frames_done=len(good), redo_frames=0, **dec_stats)
    for k, (st, img, syms) in zip(good, back):
        assert st == 0 and np.array_equal(img, jobs[k][0]), (name, k, jobs[k][0].shape)
    return want


# ---- 1. the tiling list of the seams file as one batch, in the given order and reversed ----------------------------------------------
@pytest.mark.parametrize("order", ["given", "reversed"])
def test_tiling_list_as_one_batch(mic, mico, gpu_ready, order):
    jobs = F.tiling_jobs()
    if order == "reversed":
        jobs = jobs[::-1]
    want = _roundtrip(mic, mico, jobs, order)
    assert [img.shape for (img, _, _), (rc, _) in zip(jobs, want) if rc != 0] == [(3, 3)]
    assert sorted({f[10] for rc, f in want if rc == 0}) == list(range(0, 9))      # level counts 0 (the 1-wide frames), 1 .. 8


# ---- 2. scan seams: a frame's last position group directly in front of the next frame's first ----------------------------------------
def test_scan_seams_in_one_batch(mic, mico, gpu_ready):
    jobs = F.scan_jobs()
    assert sorted(j[0].size for j in jobs[1::2]) == [8191, 8191, 8193, 16383, 16385]
    _roundtrip(mic, mico, jobs, "scan")


# ---- 3. the slow-path hand-over inside a mixed batch -----------------------------------------------------------------------------
def test_one_wide_coefficient_between_other_shapes(mic, mico, gpu_ready):
    _roundtrip(mic, mico, F.wide_jobs(), "wide")


# ---- 4. mixed reduced levels -----------------------------------------------------------------------------------------------------
def test_mixed_reduced_levels(mic, mico, gpu_ready):
    files, levels = [], []
    for (img, mv, lv), (rc, f) in zip(F.level_images(), _oracle(mico, F.level_images())):
        assert rc == 0 and f[10] == lv
        for r in (0, 1, 2, lv, lv + 1):
            files.append(f); levels.append(r)
    res, stats = mic.wavelet_v2_decompress_jobs(files, levels)
    _stats(stats, frames_done=12, redo_frames=0, **ONE)
    for k, (st, img, syms) in enumerate(res):
        f, r = files[k], levels[k]
        if r > f[10]:
            assert st == mic.MIC_ERR_ARGS and img is None, (k, st)
            continue
        assert st == 0 and np.array_equal(img, mic.wavelet_v2_decompress_level(f, r)), (k, r)
        if r == 0:
            assert np.array_equal(img, mico.wavelet_v2_decompress(f)[1]), k
    for base in (0, 5, 10):                                                   # a level-2 job decodes fewer symbols than its level-0 twin
        assert 0 < res[base + 2][2] < res[base][2], (base, res[base][2], res[base + 2][2])
    # a 16-bit escape-heavy frame at level 1 is decoded again whole, in a chain of its own
    esc = F.escape_frame()
    rc, fe = mico.wavelet_v2_compress(esc, 65535, 2)
    assert rc == 0
    res2, stats = mic.wavelet_v2_decompress_jobs(files[:3] + [fe] + files[5:8], levels[:3] + [1] + levels[5:8])
    _stats(stats, sub_batches=1, chains=2, redo_frames=1, frames_done=7)
    assert res2[3][0] == 0 and np.array_equal(res2[3][1], mic.wavelet_v2_decompress_level(fe, 1))
    for k, q in zip((0, 1, 2, 4, 5, 6), (0, 1, 2, 5, 6, 7)):
        assert res2[k][0] == 0 and np.array_equal(res2[k][1], res[q][1]), k


# ---- 5. jobs that fail alone -----------------------------------------------------------------------------------------------------
def test_jobs_that_fail_alone(mic, mico, gpu_ready):
    jobs = [(F.image(97, 301, 12, 5), 4095, 4), (F.image(40, 30, 12, 70), 4095, 3), (F.image(200, 131, 12, 6), 4095, 2),
            (F.image(120, 90, 12, 210), 4095, 5), (F.image(33, 35, 12, 9), 4095, 8)]
    want = [f for rc, f in _oracle(mico, jobs)]
    assert all(want)
    # encode: a null pointer and an out_cap one byte short, each between good jobs
    frames = [jobs[0][0], None, jobs[1][0], jobs[2][0], jobs[3][0]]
    caps = [None, None, None, len(want[2]) - 1, None]
    res, stats = mic.wavelet_v2_compress_jobs(frames, 4095, [4, 3, 3, 2, 5], caps=caps)
    _stats(stats, frames_done=3, **ONE)
    assert [st for st, _, _ in res] == [0, mic.MIC_ERR_ARGS, 0, mic.MIC_ERR_CAPACITY, 0]
    assert [res[0][1], res[2][1], res[4][1]] == [want[0], want[1], want[3]]
    res, _ = mic.wavelet_v2_compress_jobs([jobs[2][0]], 4095, [2], caps=[len(want[2])])      # (the exact capacity holds the file)
    assert res[0][:2] == (0, want[2])
    # decode: a null pointer, a file of 10 bytes, a file whose byte 12 is not 0x04, a truncated stream
    not4 = want[1][:12] + b"\x02" + want[1][13:]
    cut = want[3][: len(want[3]) * 2 // 3]
    files = [want[0], None, want[1], want[2][:10], want[2], not4, want[3], cut, want[4]]
    res, stats = mic.wavelet_v2_decompress_jobs(files)
    _stats(stats, frames_done=5, redo_frames=0, **ONE)
    codes = [st for st, _, _ in res]
    rc10, rc4, rccut = (mico.wavelet_v2_decompress(f)[0] for f in (want[2][:10], not4, cut))
    assert rc10 and rc4 and rccut
    assert codes == [0, mic.MIC_ERR_ARGS, 0, rc10, 0, rc4, 0, rccut, 0], codes
    for k, q in ((0, 0), (2, 1), (4, 2), (6, 3), (8, 4)):
        assert np.array_equal(res[k][1], jobs[q][0]), k


# ---- 6. equal shapes through the new door ------------------------------------------------------------------------------------
def test_equal_shapes_through_the_jobs_door(mic, mico, gpu_ready):
    frames = np.stack([F.image(257, 249, 16, 100 + k) for k in range(3)])
    old = mic.wavelet_v2_compress_batch(frames, 65535, 6)
    res, stats = mic.wavelet_v2_compress_jobs(list(frames), 65535, 6)
    _stats(stats, frames_done=3, **ONE)
    assert [(st, f) for st, f, _ in res] == old and [st for st, _ in old] == [0] * 3
    assert [f for _, f in old] == [mico.wavelet_v2_compress(fr, 65535, 6)[1] for fr in frames]
    files = [f for _, f in old]
    sts, px = mic.wavelet_v2_decompress_batch(files)
    back, stats = mic.wavelet_v2_decompress_jobs(files)
    _stats(stats, frames_done=3, **ONE)
    assert sts == [0] * 3 and [st for st, _, _ in back] == [0] * 3
    assert np.array_equal(np.stack([img for _, img, _ in back]), px) and np.array_equal(px, frames)


# ---- 7. sub-batching -----------------------------------------------------------------------------------------------------------
def test_sub_batches_under_a_small_workspace(mic, gpu_ready):
    """tests/wavelet_mixed_chunking_check.py in a fresh process with a 100 MiB workspace ceiling: the plan cuts the tiling list into at
    least three parts; the calls run exactly the plan's sub-batches and write the oracle's bytes"""
    mb = 100
    cuts = mic.wavelet_v2_batch_plan([(r, c) for r, c, _, _ in F.TILING], mb << 20)
    assert len(cuts) - 1 >= 3 and cuts.tolist() == F.plan([(r, c) for r, c, _, _ in F.TILING], mb << 20)
    env = dict(os.environ, MIC_HIP_WS_BUDGET_MB=str(mb))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wavelet_mixed_chunking_check.py")], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and f"wavelet mixed seams ok: {len(cuts) - 1} sub-batches" in r.stdout, r.stdout + r.stderr


# ---- 8. the session forms: encode -> decode of a mixed table stays on the device ---------------------------------------------------
def test_session_forms_against_the_host_door(mic, mico, gpu_ready):
    torch = pytest.importorskip("torch")
    jobs = [j for j in F.tiling_jobs() if j[0].shape != (3, 3)][:12] + F.wide_jobs()[1:2]
    n = len(jobs)
    host, _ = mic.wavelet_v2_compress_jobs([j[0] for j in jobs], [j[1] for j in jobs], 5)
    assert [st for st, _, _ in host] == [0] * n
    px_off = np.concatenate([[0], np.cumsum([j[0].size for j in jobs])]).astype(np.uint64)
    d_px = torch.from_numpy(np.concatenate([j[0].reshape(-1) for j in jobs]).view(np.int16).copy()).cuda()
    sess = mic.Session(n, 2 * max(j[0].size for j in jobs) + 16, device=0)
    try:
        rcs = [j[0].shape for j in jobs]
        d_streams, offs, st, applied = sess.wavelet_v2_encode_mixed(d_px.data_ptr(), px_off[:-1], rcs, 5)
        assert (st == 0).all() and applied.tolist() == [f[10] for _, f, _ in host]
        packed = torch.empty(int(offs[-1]) + 64, dtype=torch.uint8, device="cuda")
        hip = ctypes.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(ctypes.c_void_p(packed.data_ptr()), ctypes.c_void_p(d_streams), ctypes.c_size_t(int(offs[-1])), 3) == 0
        streams = packed.cpu().numpy()
        for k in range(n):                                                    # the host door's files without their 11-byte headers
            assert streams[int(offs[k]): int(offs[k + 1])].tobytes() == host[k][1][11:], k
        d_out = torch.zeros(int(px_off[-1]), dtype=torch.int16, device="cuda")
        rcl = [(r, c, int(a)) for (r, c), a in zip(rcs, applied)]
        st, syms = sess.wavelet_v2_decode_mixed(packed.data_ptr(), offs, rcl, d_out.data_ptr(), px_off[:-1])
        assert (st == 0).all()
        out = d_out.cpu().numpy().view(np.uint16)
        for k in range(n):
            assert np.array_equal(out[int(px_off[k]): int(px_off[k + 1])].reshape(rcs[k]), jobs[k][0]), k
        # mixed levels, and a frame the argument gate refuses alone
        lv = [min(k % 3, a) for k, (_, _, a) in enumerate(rcl)]
        lv[4] = rcl[4][2] + 1
        dims = [mic.wavelet_v2_level_info(host[k][1], min(lv[k], rcl[k][2])) for k in range(n)]
        out_off = np.concatenate([[0], np.cumsum([r * c for r, c in dims])]).astype(np.uint64)
        d_out.zero_()
        st, syms = sess.wavelet_v2_decode_mixed(packed.data_ptr(), offs, rcl, d_out.data_ptr(), out_off[:-1], level=lv)
        assert st.tolist() == [mic.MIC_ERR_ARGS if k == 4 else 0 for k in range(n)]
        out = d_out.cpu().numpy().view(np.uint16)
        for k in range(n):
            if k != 4:
                want = mic.wavelet_v2_decompress_level(host[k][1], lv[k])
                assert np.array_equal(out[int(out_off[k]): int(out_off[k + 1])].reshape(dims[k]), want), (k, lv[k])
    finally:
        sess.close()


# ---- 9. mic_hip_set_devices ------------------------------------------------------------------------------------------------------
@pytest.fixture
def two_shards(mic, gpu_ready):
    mic.set_devices([0, 0])
    yield
    mic.set_devices([0])


def test_the_same_files_over_two_shards(mic, mico, two_shards):
    jobs = F.tiling_jobs()
    want = _oracle(mico, jobs)
    res, stats = mic.wavelet_v2_compress_jobs([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
    assert stats["sub_batches"] == stats["chains"] == 2 and stats["frames_done"] == len(jobs) - 1, stats
    assert [(st, f) for st, f, _ in res] == [(rc, f) for rc, f in want]
    good = [f for rc, f in want if rc == 0]
    back, stats = mic.wavelet_v2_decompress_jobs(good, 1)
    assert stats["frames_done"] == sum(f[10] >= 1 for f in good), stats
    for f, (st, img, _) in zip(good, back):
        if f[10] >= 1:
            assert st == 0 and np.array_equal(img, mic.wavelet_v2_decompress_level(f, 1))
        else:                                                                 # (the 1-wide frames have no level 1)
            assert st == mic.MIC_ERR_ARGS
