"""GPU tests of the gap-removal codec (mic_hip_compress_frame_gap & co., MIC_HIP_GAP_REMOVAL units): device bytes against the
restatement in tests/gap_ref.py, decode of every map form, the batch and session paths, corrupt input and capacity."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import gap_ref
from conftest import GOLDEN
from test_gap_removal_ref import near_constant

pytestmark = pytest.mark.gpu


def _ct():
    return np.fromfile(os.path.join(GOLDEN, "CT_512_512_image.bin"), dtype="<u2").reshape(512, 512)


def _mr():
    return np.fromfile(os.path.join(GOLDEN, "MR_256_256_image.bin"), dtype="<u2").reshape(256, 256)


def _frames(synth):
    mr = _mr()
    return [
        ("ct", _ct(), 65535),
        ("mr", mr, int(mr.max())),
        ("xr12", synth.xr_like(cols=300, rows=200, depth=12, seed=4), 4095),
        ("xr16", synth.xr_like(cols=256, rows=192, depth=16, seed=5), 65535),
        ("odd", synth.xr_like(cols=333, rows=211, depth=16, seed=6), 65535),
        ("odd12", synth.xr_like(cols=129, rows=7, depth=12, seed=8), 4095),
        ("near_constant", near_constant(), 65535),
    ]


def _compress(mic, px, max_value, nstates=2):
    h, w = px.shape
    try:
        return 0, mic.compress_single_frame_gap_removal(px, w, h, max_value, nstates)
    except mic.MicError as e:
        return e.code, b""


def _decompress(mic, c, w, h):
    try:
        return 0, mic.decompress_single_frame_gap_removal(c, w, h)
    except mic.MicError as e:
        return e.code, None


def test_single_frame_matches_reference(gpu_ready, mic, mico, synth):
    modes = set()
    for name, px, mv in _frames(synth):
        rc, want, info = gap_ref.compress(mico, px, mv)
        assert rc == 0, name
        modes.add(info["mode"])
        got = mic.compress_single_frame_gap_removal(px, px.shape[1], px.shape[0], mv)
        assert got == want, (name, len(got), len(want))
        out = mic.decompress_single_frame_gap_removal(got, px.shape[1], px.shape[0])
        assert np.array_equal(out, px), name
    assert {gap_ref.MODE_NONE, gap_ref.MODE_RAW, gap_ref.MODE_DELTA} <= modes


def test_tiny_frames_fallback_and_sentinels(gpu_ready, mic, mico):
    rng = np.random.default_rng(11)
    seen = set()
    for w, h in [(1, 1), (2, 1), (3, 2), (5, 5), (8, 3), (16, 16), (4, 9)]:
        for kind in range(3):
            if kind == 0:
                px = np.full((h, w), 7, dtype=np.uint16)
            elif kind == 1:
                px = rng.integers(0, 65536, size=(h, w)).astype(np.uint16)
            else:
                px = rng.integers(0, 4096, size=(h, w)).astype(np.uint16)
            mv = 65535 if kind == 1 else 4095
            rc, want, _ = gap_ref.compress(mico, px, mv)
            rc2, got = _compress(mic, px, mv)
            assert rc2 == rc, (w, h, kind, rc, rc2)
            assert got == want, (w, h, kind)
            seen.add(rc)
            if rc == 0:
                assert np.array_equal(mic.decompress_single_frame_gap_removal(got, w, h), px)
    assert seen & {mic.MIC_ERR_USE_RLE, mic.MIC_ERR_INCOMPRESSIBLE}, seen


def _crafted(mico):
    """map forms the encoder never writes, around the CT frame's compact FSE stream"""
    ct = _ct()
    rc, blob, info = gap_ref.compress(mico, ct, 65535)
    e, fse = info["expand_map"], info["fse"]
    return ct, {
        "raw": b"\x01" + gap_ref.raw_map(e) + fse,
        "bitmap": b"\x02" + gap_ref.bitmap_map(e, int(e[-1])) + fse,
        "delta_escaped": b"\x03" + gap_ref.delta_map(e, escape_all=True) + fse,
        "delta": blob,
    }


def _wrapping(mico):
    px = near_constant()
    tokens = mico.delta_rle_compress(px, 65535)
    e = gap_ref.used_values(tokens)
    rot = list(e[1:]) + [e[0]]
    hdr = bytearray(struct.pack("<HH", len(rot), int(rot[0])))
    for i in range(1, len(rot)):
        hdr += b"\xff" + struct.pack("<H", (int(rot[i]) - int(rot[i - 1]) - 1) & 0xFFFF)
    lut = np.zeros(65536, dtype=np.uint16)
    lut[np.asarray(rot, dtype=np.int64)] = np.arange(len(rot), dtype=np.uint16)
    rc, fse = gap_ref.fse_chain(mico, lut[tokens])
    assert rc == 0
    return px, b"\x03" + bytes(hdr) + fse


def test_decode_every_map_form(gpu_ready, mic, mico):
    ct, forms = _crafted(mico)
    for name, c in forms.items():
        assert gap_ref.decompress(mico, c, 512, 512)[0] == 0, name
        out = mic.decompress_single_frame_gap_removal(c, 512, 512)
        assert np.array_equal(out, ct), name
    px, c = _wrapping(mico)
    out = mic.decompress_single_frame_gap_removal(c, px.shape[1], px.shape[0])
    assert np.array_equal(out, px)
    # a bitmap whose last byte has bits set past maxSym: those are no symbols (the reference reads bits 0 .. maxSym)
    px = np.full((20, 30), 100, dtype=np.uint16)
    px[7, 11] = 3000
    tokens = mico.delta_rle_compress(px, 4095)
    e = gap_ref.used_values(tokens)
    lut = np.zeros(65536, dtype=np.uint16)
    lut[e] = np.arange(len(e), dtype=np.uint16)
    rc, fse = gap_ref.fse_chain(mico, lut[tokens])
    assert rc == 0
    max_sym = int(e[-1]) + (1 if int(e[-1]) % 8 == 7 else 0)          # (a value whose byte has bits above it)
    bm = bytearray(gap_ref.bitmap_map(e, max_sym))
    bm[-1] |= 0x80
    c = b"\x02" + bytes(bm) + fse
    h, w = px.shape
    assert gap_ref.decompress(mico, c, w, h)[0] == 0
    assert np.array_equal(mic.decompress_single_frame_gap_removal(c, w, h), px)


@pytest.mark.parametrize("nstates", [4, 8])
def test_more_states_round_trip(gpu_ready, mic, mico, synth, nstates):
    for name, px, mv in _frames(synth):
        h, w = px.shape
        got = mic.compress_single_frame_gap_removal(px, w, h, mv, nstates)
        assert np.array_equal(mic.decompress_single_frame_gap_removal(got, w, h), px), name
        parsed = gap_ref.parse_map(got)
        e, hs = parsed
        rc, payload = mico.fse_decompress_auto(got[hs:], 4 * w * h + 64)
        assert rc == 0, name
        tokens = mico.delta_rle_compress(px, mv)
        expanded = payload if e is None else np.asarray(e, dtype=np.uint16)[payload]
        assert np.array_equal(expanded, tokens), name
        rc, back = gap_ref.decompress(mico, got, w, h)
        assert rc == 0 and np.array_equal(back, px), name


def test_batch_matches_single_frames(gpu_ready, mic, synth):
    frames = [f for _, f, _ in _frames(synth)] + [synth.xr_like(cols=200, rows=100, depth=12, seed=s) for s in range(3)]
    mvs = [mv for _, _, mv in _frames(synth)] + [4095] * 3
    res = mic.compress_batch_gap_removal(frames, mvs)
    modes = set()
    for f, mv, (st, blob, ns) in zip(frames, mvs, res):
        assert st == 0 and ns in (1, 2)
        assert blob == mic.compress_single_frame_gap_removal(f, f.shape[1], f.shape[0], mv)
        modes.add(blob[0])
    assert {0, 1, 3} <= modes
    dims = [(f.shape[1], f.shape[0]) for f in frames]
    blobs = [b for _, b, _ in res]
    bad = b"\x04" + blobs[0][1:]
    dec = mic.decompress_batch_gap_removal(blobs + [bad], dims + [dims[0]])
    for f, (st, px) in zip(frames, dec[:-1]):
        assert st == 0 and np.array_equal(px, f)
    assert dec[-1][0] == mic.MIC_ERR_CORRUPT
    # a job with bad arguments fails alone
    jobs = (mic.EncJob * 2)()
    out = np.empty(mic._gap_frame_bound(frames[2].size), dtype=np.uint8)
    for j in jobs:
        j.pixels = frames[2].ctypes.data; j.width = frames[2].shape[1]; j.height = frames[2].shape[0]
        j.max_value = 4095; j.nstates = 2; j.out = out.ctypes.data; j.out_cap = out.size
    jobs[1].nstates = 3
    assert mic.lib().mic_hip_compress_batch_gap(jobs, 2) == 0
    assert jobs[0].status == 0 and jobs[1].status == mic.MIC_ERR_ARGS


def test_batch_pinned_buffers(gpu_ready, mic):
    ct = _ct()
    src = mic.host_alloc(ct.nbytes, np.uint16)
    dst = mic.host_alloc(mic._gap_frame_bound(ct.size))
    back = mic.host_alloc(ct.nbytes, np.uint16)
    try:
        src[:] = ct.reshape(-1)
        jobs = (mic.EncJob * 1)()
        jobs[0].pixels = src.ctypes.data; jobs[0].width = 512; jobs[0].height = 512; jobs[0].max_value = 65535; jobs[0].nstates = 2
        jobs[0].out = dst.ctypes.data; jobs[0].out_cap = dst.size
        assert mic.lib().mic_hip_compress_batch_gap(jobs, 1) == 0 and jobs[0].status == 0
        n = jobs[0].out_len
        assert dst[:n].tobytes() == mic.compress_single_frame_gap_removal(ct, 512, 512, 65535)
        dj = (mic.DecJob * 1)()
        dj[0].compressed = dst.ctypes.data; dj[0].compressed_len = n; dj[0].pixels_out = back.ctypes.data
        dj[0].width = 512; dj[0].height = 512
        assert mic.lib().mic_hip_decompress_batch_gap(dj, 1) == 0 and dj[0].status == 0
        assert np.array_equal(back.reshape(512, 512), ct)
    finally:
        for a in (src, dst, back):
            mic.host_free(a)


def test_session_mixed_units(gpu_ready, mic, synth):
    import torch
    ct = _ct()
    xr = synth.xr_like(cols=512, rows=512, depth=12, seed=9)
    frames = [ct, xr, ct, xr]
    flags = [mic.MIC_HIP_GAP_REMOVAL, 0, 0, mic.MIC_HIP_GAP_REMOVAL]
    mvs = [65535, 4095, 65535, 4095]
    px = torch.from_numpy(np.stack(frames).astype(np.int16).view(np.int16)).to("cuda")
    npx = 512 * 512
    units = mic.Session.make_units([(i * npx, 512, 512, mvs[i], 2 | flags[i]) for i in range(4)])
    s = mic.Session(4, npx)
    try:
        s.encode_enqueue(px.data_ptr(), units)
        d, offs, st, ns = s.encode_finish()
        assert list(st) == [0] * 4
        dev = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda")
        mic.device_copy(dev.data_ptr(), d, int(offs[-1]))
        host = dev.cpu().numpy()
        got = [host[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(4)]
        assert got[0] == mic.compress_single_frame_gap_removal(ct, 512, 512, 65535)
        assert got[3] == mic.compress_single_frame_gap_removal(xr, 512, 512, 4095)
        assert got[1] == mic.compress_single_frame(xr, 512, 512, 4095)
        assert got[2] == mic.compress_single_frame(ct, 512, 512, 65535)
        # the plain units' blobs equal a batch without gap units
        px2 = torch.from_numpy(np.stack([xr, ct]).astype(np.int16).view(np.int16)).to("cuda")
        s2 = mic.Session(2, npx)
        try:
            s2.encode_enqueue(px2.data_ptr(), mic.Session.make_units([(0, 512, 512, 4095, 2), (npx, 512, 512, 65535, 2)]))
            d2, offs2, st2, _ = s2.encode_finish()
            dev2 = torch.empty(int(offs2[-1]), dtype=torch.uint8, device="cuda")
            mic.device_copy(dev2.data_ptr(), d2, int(offs2[-1]))
            h2 = dev2.cpu().numpy()
            assert h2[int(offs2[0]):int(offs2[1])].tobytes() == got[1]
            assert h2[int(offs2[1]):int(offs2[2])].tobytes() == got[2]
        finally:
            s2.close()
        # one decode with both kinds side by side
        out = torch.zeros(4 * npx, dtype=torch.int16, device="cuda")
        s.decode_enqueue(dev.data_ptr(), offs, units, out.data_ptr())
        st = s.decode_finish()
        assert list(st) == [0] * 4
        res = out.cpu().numpy().view(np.uint16).reshape(4, 512, 512)
        for i in range(4):
            assert np.array_equal(res[i], frames[i]), i
        # gap + gradient predictor: no such codec
        bad = mic.Session.make_units([(0, 512, 512, 65535, 2 | mic.MIC_HIP_GAP_REMOVAL | mic.MIC_HIP_PRED_GRAD)])
        rc = mic.lib().mic_hip_session_encode_enqueue(s._h, px.data_ptr(), bad, 1)
        assert rc == mic.MIC_ERR_ARGS
        rc = mic.lib().mic_hip_session_decode_enqueue(s._h, dev.data_ptr(), offs.ctypes.data_as(C.POINTER(C.c_uint64)), bad, 1,
                                                      out.data_ptr())
        assert rc == mic.MIC_ERR_ARGS
        # 0x400 is still an unknown flag
        unk = mic.Session.make_units([(0, 512, 512, 65535, 2 | 0x400)])
        assert mic.lib().mic_hip_session_encode_enqueue(s._h, px.data_ptr(), unk, 1) == mic.MIC_ERR_ARGS
    finally:
        s.close()


def test_corrupt_inputs(gpu_ready, mic, mico):
    px = near_constant()
    h, w = px.shape
    rc, good, info = gap_ref.compress(mico, px, 65535)
    cases = [b"", b"\x04" + good[1:], b"\x01", b"\x01\x05", b"\x01\x05\x00\x01\x00", b"\x02\x08", b"\x02\x10\x00\x00",
             b"\x03\x01\x00", b"\x03\x03\x00\x05\x00\x01", b"\x03\x02\x00\x05\x00\xff\x01"]
    # a payload that emits compact symbols >= numSymbols: tokens coded against a map one entry too short
    e = info["expand_map"]
    assert info["mode"] == gap_ref.MODE_RAW and len(e) >= 2
    lut = np.zeros(65536, dtype=np.uint16)
    lut[e] = np.arange(len(e), dtype=np.uint16)
    rc, fse = gap_ref.fse_chain(mico, lut[info["tokens"]])
    assert rc == 0
    cases.append(b"\x01" + gap_ref.raw_map(e[:-1]) + fse)
    # mode 3 with numSymbols = 0: every symbol is out of range
    cases.append(b"\x03\x00\x00\x00\x00" + fse)
    for c in cases:
        assert gap_ref.decompress(mico, c, w, h)[0] == gap_ref.ERR_CORRUPT, c[:8]
        assert _decompress(mic, c, w, h)[0] == mic.MIC_ERR_CORRUPT, c[:8]


def test_capacity(gpu_ready, mic, mico):
    # every pixel an escape: a checkerboard of values near 0 and near the maximum (two tokens per pixel)
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:128, 0:128]
    for mv in (4095, 65535):
        lo = rng.integers(0, mv // 40, size=(128, 128))
        hi = rng.integers(mv - mv // 40, mv + 1, size=(128, 128))
        px = np.where(((x + y) & 1).astype(bool), hi, lo).astype(np.uint16)
        assert len(mico.delta_rle_compress(px, mv)) >= 2 * px.size
        out = np.empty(mic._gap_frame_bound(px.size), dtype=np.uint8)
        n = C.c_size_t(0)
        rc = mic.lib().mic_hip_compress_frame_gap(px.ctypes.data, 128, 128, mv, 2, out.ctypes.data, out.size, C.byref(n))
        rc_ref, want, _ = gap_ref.compress(mico, px, mv)
        assert rc == rc_ref == 0 and out[: n.value].tobytes() == want
    ct = _ct()
    blob = mic.compress_single_frame_gap_removal(ct, 512, 512, 65535)
    out = np.empty(len(blob), dtype=np.uint8)
    rc = mic.lib().mic_hip_compress_frame_gap(ct.ctypes.data, 512, 512, 65535, 2, out.ctypes.data, len(blob), C.byref(n))
    assert rc == 0 and n.value == len(blob)
    rc = mic.lib().mic_hip_compress_frame_gap(ct.ctypes.data, 512, 512, 65535, 2, out.ctypes.data, len(blob) - 1, C.byref(n))
    assert rc == mic.MIC_ERR_CAPACITY
    assert mic.lib().mic_hip_compress_frame_gap(ct.ctypes.data, 512, 512, 65535, 3, out.ctypes.data, out.size, C.byref(n)) == mic.MIC_ERR_ARGS


def _weighted_unused(mico, px, max_value, nstates):
    """a gap stream whose NCount weights compact symbol numSymbols, which the payload never emits: the compact tokens plus one
    such symbol at the end are coded, then the 6-byte prefix's count drops that last symbol"""
    rc, _, info = gap_ref.compress(mico, px, max_value)
    tokens = info["tokens"]
    e = gap_ref.used_values(tokens)
    lut = np.zeros(65536, dtype=np.uint16)
    lut[e] = np.arange(len(e), dtype=np.uint16)
    compact = lut[tokens]
    rc, fse = mico.fse_compress(np.concatenate([compact, [len(e)]]).astype(np.uint16), nstates)
    assert rc == 0 and fse[0] == 0xFF
    fse = bytearray(fse)
    struct.pack_into("<I", fse, 2, len(compact))
    return b"\x01" + gap_ref.raw_map(e) + bytes(fse), compact, bytes(fse)


@pytest.mark.parametrize("nstates", [2, 4])
def test_weighted_but_unemitted_symbol_decodes(gpu_ready, mic, mico, nstates):
    """gapremovalcompressu16.go:270-273 errors on an out-of-range compact symbol only when one is emitted"""
    for px, mv in [(near_constant(), 65535), (_ct(), 65535)]:
        h, w = px.shape
        c, compact, fse = _weighted_unused(mico, px, mv, nstates)
        rc, payload = mico.fse_decompress_auto(fse, 4 * w * h + 64)
        assert rc == 0 and np.array_equal(payload, compact)
        rc, want = gap_ref.decompress(mico, c, w, h)
        assert rc == 0 and np.array_equal(want, px)
        assert np.array_equal(mic.decompress_single_frame_gap_removal(c, w, h), px)
        # the same stream with the symbol emitted (count restored) is corrupt
        full = bytearray(c)
        hs = gap_ref.parse_map(c)[1]
        struct.pack_into("<I", full, hs + 2, len(compact) + 1)
        assert gap_ref.decompress(mico, bytes(full), w, h)[0] == gap_ref.ERR_CORRUPT
        assert _decompress(mic, bytes(full), w, h)[0] == mic.MIC_ERR_CORRUPT
    # side by side with ordinary gap streams in one batch
    ct = _ct()
    c, _, _ = _weighted_unused(mico, ct, 65535, nstates)
    good = mic.compress_single_frame_gap_removal(ct, 512, 512, 65535)
    res = mic.decompress_batch_gap_removal([good, c, good], [(512, 512)] * 3)
    assert all(st == 0 and np.array_equal(p, ct) for st, p in res)
