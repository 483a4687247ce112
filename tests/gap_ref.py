"""Plain-Python restatement of CompressSingleFrameGapRemoval / DecompressSingleFrameGapRemoval
(gapremovalcompressu16.go:52-282) on top of the oracle's pieces: mico.delta_rle_compress, mico.fse_compress (two states, then
one) and mico.fse_decompress_auto.  The map logic is here, in numpy.  Test infrastructure only."""
from __future__ import annotations

import struct

import numpy as np

MODE_NONE, MODE_RAW, MODE_BITMAP, MODE_DELTA = 0x00, 0x01, 0x02, 0x03
ERR_CORRUPT = -6


def fse_chain(mico, tokens: np.ndarray, nstates: int = 2):
    """compressRLEWithFSE (:328-339) for nstates = 2; the CompressSingleFrame4State / 8State chains (multiframecompress.go:38-95)
    for 4 / 8.  Returns (rc, bytes): rc is the last attempt's error when every flavour fails."""
    chain = {2: [2, 1], 4: [4, 2, 1], 8: [8, 4, 2, 1]}[nstates]
    rc, b = -1, b""
    for ns in chain:
        rc, b = mico.fse_compress(tokens, ns)
        if rc == 0:
            return 0, b
    return rc, b""


def used_values(tokens: np.ndarray) -> np.ndarray:
    """expandMap: the sorted distinct token values"""
    return np.unique(np.asarray(tokens, dtype=np.uint16)).astype(np.int64)


def delta_map_size(e: np.ndarray) -> int:
    """computeDeltaMapSize (:286-303), the mode byte included"""
    if len(e) == 0:
        return 4
    gaps = np.diff(e) - 1
    return 4 + int(np.where(gaps >= 255, 3, 1).sum()) + 1


def choose(tokens: np.ndarray):
    """(apply, mode, overhead, expand_map) as :64-111 decide them"""
    e = used_values(tokens)
    max_sym = int(e[-1]) if len(e) else 0
    sym_len = max_sym + 1
    n = len(e)
    raw = 3 + 2 * n
    bitmap = 3 + (max_sym + 8) // 8
    delta = delta_map_size(e)
    best, mode = raw, MODE_RAW
    if bitmap < best:
        best, mode = bitmap, MODE_BITMAP
    if delta < best:
        best, mode = delta, MODE_DELTA
    apply = n > 1 and n < sym_len // 2 and best * 8 < sym_len - n
    return apply, mode, best, e


def raw_map(e) -> bytes:
    return struct.pack("<H", len(e)) + b"".join(struct.pack("<H", int(v)) for v in e)


def bitmap_map(e, max_sym: int) -> bytes:
    bm = bytearray((max_sym + 8) // 8)
    for v in e:
        bm[int(v) // 8] |= 1 << (int(v) % 8)
    return struct.pack("<H", max_sym) + bytes(bm)


def delta_map(e, escape_all: bool = False) -> bytes:
    """buildDeltaMapHeader (:306-326); escape_all writes every gap in the 3-byte form (a non-minimal map the decoder must read)"""
    out = bytearray(struct.pack("<H", len(e)))
    if len(e) == 0:
        return bytes(out)
    out += struct.pack("<H", int(e[0]))
    for i in range(1, len(e)):
        g = int(e[i]) - int(e[i - 1]) - 1
        if g >= 255 or escape_all:
            out += b"\xff" + struct.pack("<H", g & 0xFFFF)
        else:
            out.append(g)
    return bytes(out)


def compress(mico, px: np.ndarray, max_value: int, nstates: int = 2):
    """-> (rc, bytes, info) with info = {mode, header_len, tokens, expand_map, fse}"""
    tokens = mico.delta_rle_compress(px, max_value)
    apply, mode, best, e = choose(tokens)
    if not apply:
        rc, fse = fse_chain(mico, tokens, nstates)
        info = dict(mode=MODE_NONE, header_len=1, tokens=tokens, expand_map=None, fse=fse)
        return rc, (b"\x00" + fse if rc == 0 else b""), info
    assert mode != MODE_BITMAP, "the encoder never chooses a bitmap it then applies"
    lut = np.zeros(65536, dtype=np.uint16)
    lut[e] = np.arange(len(e), dtype=np.uint16)
    remapped = lut[tokens]
    rc, fse = fse_chain(mico, remapped, nstates)
    hdr = bytes([mode]) + (raw_map(e) if mode == MODE_RAW else delta_map(e))
    assert len(hdr) == best
    info = dict(mode=mode, header_len=len(hdr), tokens=tokens, expand_map=e, fse=fse)
    return rc, (hdr + fse if rc == 0 else b""), info


def parse_map(c: bytes):
    """:178-256 -> (expand_map as a list of u16, header length), or None where the reference errors"""
    if len(c) < 1:
        return None
    mode = c[0]
    if mode == MODE_NONE:
        return None, 1
    if mode == MODE_RAW:
        if len(c) < 3:
            return None
        n = struct.unpack_from("<H", c, 1)[0]
        hs = 3 + 2 * n
        if len(c) < hs:
            return None
        return [struct.unpack_from("<H", c, 3 + 2 * i)[0] for i in range(n)], hs
    if mode == MODE_BITMAP:
        if len(c) < 3:
            return None
        max_sym = struct.unpack_from("<H", c, 1)[0]
        hs = 3 + (max_sym + 8) // 8
        if len(c) < hs:
            return None
        return [s for s in range(max_sym + 1) if c[3 + s // 8] & (1 << (s % 8))], hs
    if mode == MODE_DELTA:
        if len(c) < 5:
            return None
        n = struct.unpack_from("<H", c, 1)[0]
        if n == 0:
            return [], 5
        e = [struct.unpack_from("<H", c, 3)[0]]
        p = 5
        for _ in range(1, n):
            if p >= len(c):
                return None
            b = c[p]
            p += 1
            if b == 0xFF:
                if p + 2 > len(c):
                    return None
                g = struct.unpack_from("<H", c, p)[0]
                p += 2
            else:
                g = b
            e.append((e[-1] + g + 1) & 0xFFFF)            # Go uint16 arithmetic
        return e, p
    return None


def delta_rle_decompress(mico, tokens: np.ndarray, w: int, h: int):
    """DeltaRleDecompressU16.Decompress through the oracle's mico_delta_rle_decompress -> (rc, pixels)"""
    import ctypes as C
    tok = np.ascontiguousarray(tokens, dtype=np.uint16)
    out = np.empty((h, w), dtype=np.uint16)
    rc = mico.lib().mico_delta_rle_decompress(C.c_void_p(tok.ctypes.data), C.c_size_t(tok.size), w, h, C.c_void_p(out.ctypes.data))
    return rc, (out if rc == 0 else None)


def decompress(mico, c: bytes, w: int, h: int):
    """-> (rc, pixels): the map, mico.fse_decompress_auto, the expansion, the Delta+RLE decoder."""
    c = bytes(c)
    parsed = parse_map(c)
    if parsed is None:
        return ERR_CORRUPT, None
    e, hs = parsed
    if e is None:
        return mico.decompress_single_frame(c[1:], w, h)
    rc, compact = mico.fse_decompress_auto(c[hs:], 4 * w * h + 64)
    if rc:
        return rc, None
    if len(compact) and int(compact.max()) >= len(e):
        return ERR_CORRUPT, None
    tokens = np.asarray(e, dtype=np.uint16)[compact] if len(compact) else np.zeros(0, dtype=np.uint16)
    return delta_rle_decompress(mico, tokens, w, h)
