"""CPU tests of the gap-removal codec's restatement (tests/gap_ref.py) against what the reference publishes and what its code
implies (gapremovalcompressu16.go), and of the library's exports of the four gap entry points."""
import ctypes
import os
import struct

import numpy as np

import gap_ref
from conftest import GOLDEN


def _ct():
    return np.fromfile(os.path.join(GOLDEN, "CT_512_512_image.bin"), dtype="<u2").reshape(512, 512)


def _mr():
    return np.fromfile(os.path.join(GOLDEN, "MR_256_256_image.bin"), dtype="<u2").reshape(256, 256)


def near_constant(seed=7, w=34, h=26):
    rng = np.random.default_rng(seed)
    px = np.full((h, w), 1000, dtype=np.uint16)
    px[rng.integers(h), rng.integers(w)] = int(rng.integers(20000, 65535))
    return px


def _table_log(fse: bytes) -> int:
    off = 6 if fse[0] == 0xFF else 0                                   # N-state streams carry a 6-byte prefix
    return (fse[off] & 0xF) + 5


def test_ct_delta_map(mico):
    rc, blob, info = gap_ref.compress(mico, _ct(), 65535)
    assert rc == 0
    assert info["mode"] == gap_ref.MODE_DELTA and len(info["expand_map"]) == 1782
    assert info["header_len"] == 1800                                   # (docs/compression-results.md says 1798: the code writes 1800)
    assert len(blob) == 233285
    assert _table_log(info["fse"]) == 13


def test_ct_without_gap_removal(mico):
    rc, blob = mico.compress_single_frame(_ct(), 65535)
    assert rc == 0 and len(blob) == 234337 and _table_log(blob) == 16


def test_mr_is_mode_0(mico):
    mr = _mr()
    rc, blob, info = gap_ref.compress(mico, mr, int(mr.max()))
    rc2, plain = mico.compress_single_frame(mr, int(mr.max()))
    assert rc == 0 and rc2 == 0 and info["mode"] == gap_ref.MODE_NONE and blob == b"\x00" + plain


def test_near_constant_frame_is_raw(mico):
    rc, blob, info = gap_ref.compress(mico, near_constant(), 65535)
    assert rc == 0 and info["mode"] == gap_ref.MODE_RAW and blob[0] == 1


def test_bitmap_is_never_chosen_and_applied():
    rng = np.random.default_rng(3)
    for trial in range(400):
        max_sym = int(rng.integers(1, 65536))
        k = int(rng.integers(1, min(max_sym + 1, 3000) + 1))
        vals = np.unique(np.concatenate([rng.integers(0, max_sym + 1, size=k), [max_sym]])).astype(np.uint16)
        apply, mode, _, _ = gap_ref.choose(vals)
        assert not (apply and mode == gap_ref.MODE_BITMAP), (trial, max_sym, k)


def test_reference_decoder_round_trips_every_mode(mico):
    ct = _ct()
    rc, blob, info = gap_ref.compress(mico, ct, 65535)
    e, fse = info["expand_map"], info["fse"]
    max_sym = int(e[-1])
    forms = {
        "delta": blob,
        "raw": b"\x01" + gap_ref.raw_map(e) + fse,
        "bitmap": b"\x02" + gap_ref.bitmap_map(e, max_sym) + fse,
        "delta_escaped": b"\x03" + gap_ref.delta_map(e, escape_all=True) + fse,
    }
    for name, c in forms.items():
        rc, px = gap_ref.decompress(mico, c, 512, 512)
        assert rc == 0 and np.array_equal(px, ct), name
    mr = _mr()
    rc, blob, _ = gap_ref.compress(mico, mr, int(mr.max()))
    rc, px = gap_ref.decompress(mico, blob, 256, 256)
    assert rc == 0 and np.array_equal(px, mr)


def test_wrapping_delta_map(mico):
    """expandMap[i] = expandMap[i-1] + gap + 1 in uint16: a map may wrap past 65535 and the decoder expands it as Go does"""
    px = near_constant()
    tokens = mico.delta_rle_compress(px, 65535)
    e = gap_ref.used_values(tokens)
    # the same values listed from e[1] upwards, then wrapping to e[0]: the compact indices are rotated by one
    rot = list(e[1:]) + [e[0]]
    hdr = bytearray(struct.pack("<HH", len(rot), int(rot[0])))
    for i in range(1, len(rot)):
        g = (int(rot[i]) - int(rot[i - 1]) - 1) & 0xFFFF
        hdr += b"\xff" + struct.pack("<H", g)
    lut = np.zeros(65536, dtype=np.uint16)
    lut[np.asarray(rot, dtype=np.int64)] = np.arange(len(rot), dtype=np.uint16)
    rc, fse = gap_ref.fse_chain(mico, lut[tokens])
    assert rc == 0
    stream = b"\x03" + bytes(hdr) + fse
    assert gap_ref.parse_map(stream)[0] == [int(v) for v in rot]
    rc, out = gap_ref.decompress(mico, stream, px.shape[1], px.shape[0])
    assert rc == 0 and np.array_equal(out, px)


def test_reference_decoder_errors(mico):
    for c in [b"", b"\x04", b"\x01\x00", b"\x01\x02\x00\x01\x00", b"\x02\x08", b"\x02\x10\x00\x00", b"\x03\x01\x00\x00",
              b"\x03\x03\x00\x05\x00\x01", b"\x03\x02\x00\x05\x00\xff\x01"]:
        assert gap_ref.decompress(mico, c, 4, 4)[0] == gap_ref.ERR_CORRUPT, c


def test_library_exports_gap_entry_points(mic):
    L = ctypes.CDLL(mic.LIB_PATH)
    for name in ("mic_hip_compress_frame_gap", "mic_hip_decompress_frame_gap", "mic_hip_compress_batch_gap",
                 "mic_hip_decompress_batch_gap"):
        assert hasattr(L, name), name
    assert mic.MIC_HIP_GAP_REMOVAL == 0x800
    for name in ("compress_single_frame_gap_removal", "decompress_single_frame_gap_removal", "compress_batch_gap_removal",
                 "decompress_batch_gap_removal"):
        assert callable(getattr(mic, name)), name
