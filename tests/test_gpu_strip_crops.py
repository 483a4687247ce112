"""Many crops of many strip files per call into a device tensor (csrc/mic_strip_crops.hip: mic_hip_strips_read_crops,
mic_hip_session_strips_read_crops).  The codec is lossless, so the expected value of every crop is the source image, padded with zeros
and cropped in numpy (strip_crop_files.expected); the files are written by the device's whole-image encoders and decoded once with
the whole-image decoders, which test_gpu_parity.py pins to the oracle."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import strip_crop_files as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files(mic, synth, gpu_ready):
    """[(name, image, file bytes)]: A, B, D, E PICS, C PICA; each decoded once and compared with its source, never written to"""
    out = F.build(synth, lambda img, maxv, strips, states: mic.compress_parallel_strips(img, img.shape[1], img.shape[0], maxv, strips, states),
                  lambda img, maxv, strips: mic.compress_parallel_strips_adaptive(img, img.shape[1], img.shape[0], maxv, strips))
    for name, img, data in out:
        px = mic.decompress_parallel_strips(data)[0] if F.FILES[name][3] == "PICS" else mic.decompress_parallel_strips_adaptive(data)
        assert np.array_equal(np.asarray(px).reshape(img.shape), img), name
    c = F.StripFile(out[2][2])
    kept = [c.grad(k) for k in range(c.n)]
    assert any(kept) and not all(kept), kept                              # C: some strips kept the gradient predictor, some the average one
    assert out[1][1].min() < 32768 < out[1][1].max()
    return out


def _tensor(n, ch, cw):
    import torch
    return torch.full((max(n, 1), ch, cw, 2), 0xA5, dtype=torch.uint8, device="cuda")   # (every byte must be overwritten)


def _read(call, xyf, cw, ch):
    """call(xyf, cw, ch, d_out, out_cap) -> (status, failed strip, stats); the crops as (n, ch, cw) u16"""
    t = _tensor(len(xyf), ch, cw)
    st, bad, stats = call(xyf, cw, ch, t.data_ptr(), len(xyf) * ch * cw * 2)
    return t.cpu().numpy()[: len(xyf)].view("<u2")[..., 0], st, bad, stats


class _Doors:
    """the two entry points on one list of files: .file and .session, each call(xyf, cw, ch, d_out, out_cap)"""

    def __init__(self, mic, datas):
        import torch
        self.sess = mic.Session(4, 96 * 70)
        self.d_files = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() for d in datas]
        heads = [bytes(d[: F.StripFile(d).body]) if d[:4] in (b"PICS", b"PICA") else bytes(d[:64]) for d in datas]
        ptrs, lens = [t.data_ptr() for t in self.d_files], [len(d) for d in datas]
        self.file = lambda xyf, cw, ch, d, cap: mic.strips_read_crops(datas, xyf, cw, ch, d, cap)
        self.session = lambda xyf, cw, ch, d, cap: self.sess.strips_read_crops(heads, ptrs, lens, xyf, cw, ch, d, cap)
        self.all = [("file", self.file), ("session", self.session)]

    def close(self):
        self.sess.close()


@pytest.mark.parametrize("shape", F.SHAPES)
def test_crops_equal_the_padded_sources(mic, files, shape):
    cw, ch = shape
    datas = [d for _, _, d in files]
    xyf = F.origins(files, cw, ch)
    want = F.expected(files, xyf, cw, ch)
    units, pieces, fs = mic.strips_crop_plan(datas, xyf, cw, ch)
    want_units, want_pieces, _ = F.brute_plan(files, xyf, cw, ch)
    assert [tuple(u) for u in units.tolist()] == want_units and pieces == want_pieces
    total = sum(F.StripFile(d).n for d in datas)
    doors = _Doors(mic, datas)
    try:
        for door, call in doors.all:
            got, st, bad, stats = _read(call, xyf, cw, ch)
            for i in range(len(xyf)):
                assert np.array_equal(got[i], want[i]), (door, shape, xyf[i])
            assert (st == mic.MIC_OK).all() and (bad == -1).all(), (door, st, bad)
            assert stats["strips_decoded"] == len(units) and stats["pieces"] == pieces and stats["slabs"] >= 1, (door, stats)
            assert stats["strips_total"] == total, (door, stats)
        if shape == (32, 16):                                             # a few crops of a file touch a few of its strips
            few = [(5, 2, 0), (40, 5, 2), (500, 9, 3)]
            for door, call in doors.all:
                got, st, bad, stats = _read(call, few, cw, ch)
                assert np.array_equal(got, F.expected(files, few, cw, ch)) and (st == 0).all(), door
                assert stats["strips_decoded"] == 2 + 1 + 2 < stats["strips_total"] == 8 + 6 + 3, (door, stats)
        outside = [(files[f][1].shape[1], 0, f) for f in range(len(files))] + [(0, 70, 0), (-cw, 0, 2), (3, -ch, 3)]
        for door, call in doors.all:
            got, st, bad, stats = _read(call, outside, cw, ch)
            assert not got.any() and (st == 0).all() and (bad == -1).all(), door
            assert stats == dict(strips_decoded=0, strips_total=total, pieces=0, slabs=0), (door, stats)
    finally:
        doors.close()


def test_pinned_host_output(mic, files):
    datas = [d for _, _, d in files]
    xyf = F.origins(files, 33, 9)
    buf = mic.host_alloc(len(xyf) * 9 * 33 * 2)
    try:
        buf[:] = 0xA5
        st, bad, stats = mic.strips_read_crops(datas, xyf, 33, 9, buf.ctypes.data, buf.size)
        assert (st == 0).all() and (bad == -1).all()
        assert np.array_equal(buf.view("<u2").reshape(len(xyf), 9, 33), F.expected(files, xyf, 33, 9))
    finally:
        mic.host_free(buf)


def _damage(mic, data, k):
    """file A with strip k's stream damaged so that the whole-image decoder refuses it: (bytes, that decoder's code).  The first try
    is the flip tests/test_gpu_mic2_crops.py makes; should the flipped stream still decode, coarser damage follows."""
    b, e = F.StripFile(data).span(k)
    mid = (b + e) // 2
    for edit in (lambda d: d.__setitem__(mid, d[mid] ^ 0x5A),
                 lambda d: d.__setitem__(slice(mid - 8, mid + 8), bytes(16)),
                 lambda d: d.__setitem__(slice(b, b + 8), b"\xff" * 8)):
        d = bytearray(data)
        edit(d)
        try:
            mic.decompress_parallel_strips(bytes(d))
        except mic.MicError as err:
            assert err.strip == k and err.code != mic.MIC_OK
            return bytes(d), err.code
    pytest.fail("no damage made the whole-image decoder refuse the strip")


def test_a_damaged_strip_fails_the_crops_on_it_only(mic, files):
    cw, ch = 32, 16
    xyf = F.origins(files, cw, ch) + [(0, 27, 0), (40, 28, 0), (3, 18, 0), (3, 36, 0)]   # A: in and around strip 3 (rows 27 .. 35)
    want = F.expected(files, xyf, cw, ch)
    datas = [d for _, _, d in files]
    datas[0], code = _damage(mic, datas[0], 3)
    doors = _Doors(mic, datas)
    try:
        for door, call in doors.all:
            got, st, bad, stats = _read(call, xyf, cw, ch)
            hit = 0
            for i, o in enumerate(xyf):
                on_it = (0, 3) in F.brute_plan(files, [o], cw, ch)[0]
                hit += on_it
                assert (st[i], bad[i]) == ((code, 3) if on_it else (mic.MIC_OK, -1)), (door, o, st[i], bad[i])
                if not on_it:
                    assert np.array_equal(got[i], want[i]), (door, o)      # A's other strips included
            assert 0 < hit < sum(1 for o in xyf if o[2] == 0)
    finally:
        doors.close()
    # a table entry of B that points outside the file fails B's crops alone, whichever strips they need
    datas = [d for _, _, d in files]
    b = bytearray(datas[1])
    struct.pack_into("<I", b, F.StripFile(datas[1]).entry_at(4), len(b))
    datas[1] = bytes(b)
    with pytest.raises(mic.MicError) as e:
        mic.decompress_parallel_strips(datas[1])
    assert e.value.code == mic.MIC_ERR_CORRUPT
    doors = _Doors(mic, datas)
    try:
        for door, call in doors.all:
            got, st, bad, stats = _read(call, xyf, cw, ch)
            for i, o in enumerate(xyf):
                if o[2] == 1:
                    assert st[i] == mic.MIC_ERR_CORRUPT and bad[i] == -1 and not got[i].any(), (door, o)
                else:
                    assert st[i] == mic.MIC_OK and np.array_equal(got[i], want[i]), (door, o)
            assert stats["strips_total"] == sum(F.StripFile(d).n for k, d in enumerate(datas) if k != 1), (door, stats)
    finally:
        doors.close()


def test_argument_errors_come_back_before_any_launch(mic, files):
    datas = [d for _, _, d in files]
    cw, ch = 32, 16
    xyf = [(0, 0, 0), (10, 10, 2)]
    t = _tensor(2, ch, cw)
    cap = 2 * ch * cw * 2
    pageable = np.zeros(cap, dtype=np.uint8)
    many = [(0, 0, 3)] * 16384                                            # 16 MiB of crops: far past the allocation t lies in
    doors = _Doors(mic, datas)
    try:
        for door, call in doors.all:
            for args, want in [(([(0, 0, 0), (0, 0, 5)], cw, ch, t.data_ptr(), cap), mic.MIC_ERR_ARGS),       # a file index outside the list
                               (([(0, 0, 0), (0, 0, -1)], cw, ch, t.data_ptr(), cap), mic.MIC_ERR_ARGS),
                               ((xyf, 0, ch, t.data_ptr(), cap), mic.MIC_ERR_ARGS), ((xyf, cw, -2, t.data_ptr(), cap), mic.MIC_ERR_ARGS),
                               ((xyf, cw, ch, t.data_ptr(), cap - 1), mic.MIC_ERR_CAPACITY),
                               ((xyf, cw, ch, pageable.ctypes.data, cap), mic.MIC_ERR_ARGS),
                               ((many, cw, ch, t.data_ptr(), 16384 * ch * cw * 2), mic.MIC_ERR_ARGS)]:
                with pytest.raises(mic.MicError) as e:
                    call(*args)
                assert e.value.code == want, (door, args[1:], want)
            st, bad, stats = call([], cw, ch, t.data_ptr(), 0)             # n = 0: nothing to do, and that is no error
            assert st.size == 0 and stats == dict(strips_decoded=0, strips_total=0, pieces=0, slabs=0)
            assert (t.cpu().numpy() == 0xA5).all() and not pageable.any()  # none of the refused calls wrote a byte
            got, st, bad, stats = _read(call, xyf, cw, ch)                 # (the same call with good arguments runs)
            assert np.array_equal(got, F.expected(files, xyf, cw, ch)) and (st == 0).all(), door
    finally:
        doors.close()


def test_the_gather_kernel_is_timed_under_its_name(mic, files):
    datas = [d for _, _, d in files]
    doors = _Doors(mic, datas)
    try:
        doors.sess.set_timing(True)
        _read(doors.session, [(0, 0, 0), (5, 5, 3)], 32, 16)
        assert "k_strips_gather_crops" in dict(doors.sess.last_timings())
    finally:
        doors.close()


def test_a_tall_piece_is_cut_over_grid_y(mic, synth, gpu_ready):
    """A piece of 128 x 72: lanes are 64 wide, a block pass takes 4 rows, so the piece is 2 column passes x 18 row passes = 36 passes
    and row_chunks cuts it over grid y = 2 -- which no piece of the shared files reaches.  One PICS file of one strip, 130 x 72 at 12
    bits (file A's recipe).  The crop at (1, -4) starts one sample into every strip row: 130 samples a row are a multiple of four
    bytes, so each of its rows is 2-byte-aligned only and moves as u16; the rows of the crop at (0, 0) move as dwords."""
    w, h, cw, ch = 130, 72, 128, 80
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    img = np.clip(np.rint(900 + 5 * x + 11 * y + 2.0 * synth.approx_gauss(h * w, 11).reshape(h, w)), 0, 65535).astype(np.uint16)
    data = bytes(mic.compress_parallel_strips(img, w, h, 4095, 1, 2))
    assert F.StripFile(data).n == 1 and np.array_equal(np.asarray(mic.decompress_parallel_strips(data)[0]).reshape(h, w), img)
    tall = [("tall", img, data)]
    xyf = [(1, -4, 0), (0, 0, 0)]
    want = F.expected(tall, xyf, cw, ch)
    assert np.array_equal(want[0, 4:76], img[:, 1:129]) and not want[0, :4].any() and not want[0, 76:].any()
    doors = _Doors(mic, [data])
    try:
        for door, call in doors.all:
            got, st, bad, stats = _read(call, xyf, cw, ch)
            assert np.array_equal(got, want), door
            assert (st == mic.MIC_OK).all() and (bad == -1).all(), (door, st, bad)
            assert stats == dict(strips_decoded=1, strips_total=1, pieces=2, slabs=1), (door, stats)
    finally:
        doors.close()


def test_sub_batch_seams_under_a_small_workspace():
    """tests/strip_crops_chunking_check.py in a fresh process with a 5 MiB workspace ceiling.  A sub-batch takes units while their
    number times (unit_ws_bytes(px) + 2 px), px the largest of them, stays under the ceiling (next_strip_cut).  The tier-2 slabs of a
    unit are 4 * (4 px + 16) (tokens, symbols) + 131104 + 2 * (4 px + 16) (blob) + 8 * (2 px + 8) (segments) + px / 8 (flags) +
    26 * 65536 (tables) + 8192.  The smallest strip of the five files, E's 40 x 8 = 320 pixels, comes to 1856872 with its pixels; the
    largest, D's 1040 x 8 = 8320, to 4 * 33296 + 197696 + 133184 + 1040 + 1703936 + 8192 + 16640 = 2193872.  5 MiB = 5242880 bytes hold
    two of the largest (4387744) and not three of the smallest (5570616): every sub-batch holds exactly two strips, whatever their
    sizes, and a call that needs n strips runs ceil(n / 2) decode chains (1 MiB steps are fine enough: 4 MiB would leave D's strips
    alone, 6 MiB would take three small ones)."""
    env = dict(os.environ, MIC_HIP_WS_BUDGET_MB="5")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "strip_crops_chunking_check.py")], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "strip crop seams ok" in r.stdout, r.stdout + r.stderr
