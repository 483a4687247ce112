"""Volumes, crop lists and numpy expectations shared by the tests of the MIC2 crop calls over many volumes
(test_mic2_multi_plan_cpu.py, test_gpu_mic2_multi_crops.py, mic2_multi_chunking_check.py).  Nothing here calls the code under test."""
import struct

import numpy as np

import mic2_crop_volumes as V
from mic2_crop_volumes import volume_12bit, volume_16bit, expected, Mic2File, RecordingSource, SHAPES   # noqa: F401  (shared as they are)


def _sparse(rng, shape, base):
    """a few small values sprinkled over `base`: what the encoder still accepts at these sizes -- a cut of an XR-like image of
    33 x 9 is MIC_ERR_INTERNAL / MIC_ERR_INCOMPRESSIBLE to it and to the oracle, its coded frame would be larger than the raw one"""
    return np.where(rng.random(shape) < 0.6, base, base + rng.integers(-4, 5, shape))


def volume_narrow(synth):
    """3 frames of 33 x 9 at 12 bits: rows narrower than a wave, and 33 columns go one past the 32-lane layout of a piece"""
    rng = np.random.default_rng(0)
    frames = [_sparse(rng, (9, 33), 1000)]
    for _ in range(2):
        frames.append(_sparse(rng, (9, 33), frames[-1]))
    return np.stack(frames).astype(np.uint16), 4095


def volume_tiny(synth):
    """one frame of 7 x 35: for a temporal file that is frame 0 and no residual.  (No frame of 7 x 5 can be coded: at 35 pixels
    every coded frame is larger than the raw one, MIC_ERR_INCOMPRESSIBLE, here and in the oracle; 35 rows are the fewest of 7
    columns that this content codes at.)"""
    rng = np.random.default_rng(1)
    return np.where(rng.random((1, 35, 7)) < 0.6, 1000, 1000 + rng.integers(1, 5, (1, 35, 7))).astype(np.uint16), 4095


def hand_file(w, h, n, temporal, lens=None, magic=b"MIC2"):
    """a MIC2 file made of its header and frame table alone (multiframe.go:49-91), the streams all zero bytes: what a planner reads"""
    lens = [16] * n if lens is None else list(lens)
    out = bytearray(magic + struct.pack("<III", w, h, n) + bytes([3 if temporal else 1, 0, 0, 0]))
    off = 0
    for ln in lens:
        out += struct.pack("<II", off, ln)
        off += ln
    return bytes(out) + bytes(off)


def interleave(per_volume):
    """per_volume[v] = the (x, y, z) origins of volume v (None: no crops) -> (x, y, z, v) round robin over the volumes, so that
    consecutive crops name different volumes"""
    out, k = [], 0
    while any(p is not None and k < len(p) for p in per_volume):
        out += [tuple(p[k]) + (v,) for v, p in enumerate(per_volume) if p is not None and k < len(p)]
        k += 1
    return out


def crops_of(xyzv, v):
    """(indices into xyzv, (x, y, z) origins) of the crops that name volume v"""
    idx = [i for i, c in enumerate(xyzv) if c[3] == v]
    return idx, [tuple(xyzv[i][:3]) for i in idx]


def brute_multi_plan(dims, xyzv, cw, ch, cd):
    """dims[v] = (w, h, n, temporal) or None (a volume that yields no units) -> ([(volume, frame)] ascending, pieces), volume by
    volume through mic2_crop_volumes.brute_plan"""
    units, pieces = [], 0
    for v, d in enumerate(dims):
        _, xyz = crops_of(xyzv, v)
        if d is None or not xyz:
            continue
        frames, p = V.brute_plan(d[0], d[1], d[2], d[3], xyz, cw, ch, cd)
        units += [(v, f) for f in frames]
        pieces += p
    return units, pieces


def expected_multi(vols, xyzv, cw, ch, cd):
    """the crops of the zero-padded volumes: (len(xyzv), cd, ch, cw); vols[v] None: zeros"""
    out = np.zeros((len(xyzv), cd, ch, cw), dtype=np.uint16)
    for v, vol in enumerate(vols):
        idx, xyz = crops_of(xyzv, v)
        if vol is not None and idx:
            out[idx] = V.expected(vol, xyz, cw, ch, cd)
    return out


def unit_ws_bytes(px):
    """the tier-2 slabs of a unit of px pixels (unit_ws_bytes, csrc/mic_api.hip; the arithmetic of
    test_gpu_mic2_crops.py::test_sub_batch_seams_under_a_small_workspace): tokens and symbols, blob, segments, flags, tables"""
    tokc = 4 * px + 16
    return 4 * tokc + (8 + 131080 + 2 * tokc + 16) + 8 * (2 * px + 8) + px // 8 + 26 * 65536 + 8192


def cuts_of(px, budget):
    """the cut rule of the many-volume core restated: a sub-batch takes units while their number stays within
    budget / (unit_ws_bytes(mp) + 2 mp), mp its largest frame, and within 65535; at least one.  -> [0, ..., len(px)]"""
    cuts = [0]
    while cuts[-1] < len(px):
        i0 = i1 = cuts[-1]
        mp = 0
        while i1 < len(px):
            m = max(mp, px[i1])
            if i1 > i0 and (i1 - i0 + 1 > budget // (unit_ws_bytes(m) + 2 * m) or i1 - i0 >= 65535):
                break
            mp, i1 = m, i1 + 1
        cuts.append(i1)
    return cuts
