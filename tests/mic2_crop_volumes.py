"""Volumes, crop origins and numpy expectations shared by the MIC2 crop tests (test_mic2_crop_plan_cpu.py, test_mic2_reader_cpu.py,
test_gpu_mic2_crops.py, mic2_crops_chunking_check.py).  Nothing here calls the code under test."""
import struct

import numpy as np

# (cw, ch, cd): a crop that straddles dword-aligned and 2-byte-aligned rows, one narrower than a wave (rows side by side), one
# sample, and the whole 150 x 70 x 11 volume
SHAPES = [(48, 40, 3), (17, 5, 4), (1, 1, 1), (150, 70, 11)]


def volume_12bit(synth):
    """11 frames of 150 x 70 at 12 bits: a cut of an XR-like image, rolled from frame to frame (tests/chunking_check.py).  The odd
    width makes every second row of a frame 2-byte-aligned only."""
    img = synth.xr_like(cols=300, rows=640, depth=12, seed=17)[:70, :150]
    return np.stack([np.roll(img, 3 * k, axis=1) for k in range(11)]), 4095


def volume_16bit(synth):
    """6 frames of 160 x 96 with max_value 65535: a 14-bit image plus 30000 per frame mod 2^16, so that consecutive frames differ
    by more than 2^15 in places and the temporal sums wrap (full-range 16-bit noise is incompressible to the reference's encoder)"""
    img = synth.xr_like(cols=320, rows=200, depth=14, seed=5)[:96, :160].astype(np.uint32)
    return np.stack([((np.roll(img, 2 * k, axis=0) + 30000 * k) & 0xFFFF).astype(np.uint16) for k in range(6)]), 65535


def origins(w, h, n, cw, ch, cd):
    """(x, y, z) origins of cw x ch x cd crops in a w x h x n volume: inside; straddling each of the six faces; wholly outside in
    x, y and z (below 0, at and past the end); z = -2; a crop twice; crops that overlap in every axis and share frames"""
    return [(20, 10, 2), (0, 0, 0),
            (-5, 10, 2), (w - cw // 2 - 1, 10, 2), (20, -3, 2), (20, h - ch // 2 - 1, 2), (20, 10, -1), (20, 10, n - 1),
            (w, 0, 0), (-cw, 0, 0), (w + 7, 0, 0), (0, h, 0), (0, -ch, 1), (0, 0, n), (0, 0, n + 3), (0, 0, -cd),
            (7, 3, -2),
            (33, 21, 4), (33, 21, 4),
            (25, 12, 3), (30, 15, 1), (-3, -2, n - 2)]


def expected(vol, xyz, cw, ch, cd):
    """the crops of the zero-padded volume: (len(xyz), cd, ch, cw)"""
    n, h, w = vol.shape
    pad = np.zeros((n + 2 * cd, h + 2 * ch, w + 2 * cw), dtype=vol.dtype)
    pad[cd: cd + n, ch: ch + h, cw: cw + w] = vol
    out = np.zeros((len(xyz), cd, ch, cw), dtype=vol.dtype)
    for i, (x, y, z) in enumerate(xyz):
        x, y, z = min(max(x, -cw), w) + cw, min(max(y, -ch), h) + ch, min(max(z, -cd), n) + cd   # (farther out is as empty)
        out[i] = pad[z: z + cd, y: y + ch, x: x + cw]
    return out


def brute_plan(w, h, n, temporal, xyz, cw, ch, cd):
    """(frames to entropy-decode, number of (crop, frame) pairs with a non-empty overlap), by enumerating every crop's coordinates"""
    frames, pieces = set(), 0
    for x, y, z in xyz:
        xs, ys, zs = np.arange(x, x + cw), np.arange(y, y + ch), np.arange(z, z + cd)
        area = int(((xs >= 0) & (xs < w)).sum()) * int(((ys >= 0) & (ys < h)).sum())
        inside = [int(f) for f in zs if 0 <= f < n]
        if area:
            pieces += len(inside)
            frames.update(inside)
    if temporal and frames:
        frames = set(range(max(frames) + 1))
    return sorted(frames), pieces


class Mic2File:
    """a MIC2 file taken apart (multiframe.go:49-91): 20-byte header, 8 bytes (offset, length) per frame, the streams"""

    def __init__(self, data):
        self.data = bytearray(data)
        assert self.data[:4] == b"MIC2"
        self.w, self.h, self.n = struct.unpack_from("<III", self.data, 4)
        self.temporal = bool(self.data[16] & 2)
        self.body = 20 + 8 * self.n

    def span(self, f):
        """[begin, end) of frame f's stream in the file"""
        off, ln = struct.unpack_from("<II", self.data, 20 + 8 * f)
        return self.body + off, self.body + off + ln

    def head(self):
        return bytes(self.data[: self.body])


class RecordingSource:
    """a reader's source that notes every (offset, length) it is asked for"""

    def __init__(self, data):
        self.data, self.reads = bytes(data), []

    def __call__(self, off, n):
        self.reads.append((off, n))
        return self.data[off: off + n]

    def coverage(self):
        c = np.zeros(len(self.data), dtype=np.int32)
        for off, n in self.reads:
            c[off: off + n] += 1
        return c
