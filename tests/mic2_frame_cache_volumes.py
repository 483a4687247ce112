"""Volumes, crop lists and helpers shared by the frame-cache tests of the MIC2 crop readers (test_gpu_mic2_frame_cache.py,
mic2_frame_cache_chunking_check.py).  Nothing here calls the code under test.

The frames are the smallest at which the whole-frame kernel can still go wrong: 37 x 19 = 703 pixels is no multiple of 8 (a peeled
tail of 7) or of 256; 64 x 33 = 2112 pixels is 264 groups of eight, four waves and a part of a fifth, and one block of 2048 pixels
and a part of a second; 8 x 35 = 280 pixels is groups of eight and nothing else, in less than one wave.  (The issue asks for one
frame of exactly 8 x 1.  No such frame can be coded: at 8 pixels every coded frame is larger than the raw one and the encoder, like
the reference's, answers MIC_ERR_INCOMPRESSIBLE -- as it does up to 8 x 24.  8 x 35 is the smallest frame of width 8 this content
codes at, and it keeps what the 8 x 1 frame was for: full groups, no tail.)"""
import struct

import numpy as np

import mic2_crop_volumes as V

SIZES = {"odd": (37, 19, 13), "wave": (64, 33, 16), "eight": (8, 35, 12)}     # (width, height, frames)
MAXV = 4095


def volume(name):
    """a few small values sprinkled over the frame before (mic2_multi_volumes._sparse: what the encoder still accepts at these sizes)"""
    w, h, n = SIZES[name]
    rng = np.random.default_rng(sorted(SIZES).index(name) + 3)
    frames = [np.where(rng.random((h, w)) < 0.6, 1000, 1000 + rng.integers(-4, 5, (h, w)))]
    for _ in range(n - 1):
        frames.append(np.where(rng.random((h, w)) < 0.6, frames[-1], frames[-1] + rng.integers(-4, 5, (h, w))))
    return np.stack(frames).astype(np.uint16)


def make_files(mic, name):
    vol = volume(name)
    n, h, w = vol.shape
    files = {}
    for temporal in (False, True):
        data = mic.compress_multi_frame(vol, w, h, MAXV, temporal=temporal)
        assert np.array_equal(mic.decompress_multi_frame(data), vol) and V.Mic2File(data).temporal == temporal
        files[temporal] = data
    vol.setflags(write=False)
    return dict(vol=vol, files=files)


def named_frames(w, h, n, xyz, cw, ch, cd):
    """the frames some crop overlaps, ascending: a frame cache's keys of the call"""
    return V.brute_plan(w, h, n, False, xyz, cw, ch, cd)[0]


def at_frames(frames, x=2, y=3):
    """one crop of depth 1 per frame: a call that names exactly these frames"""
    return [(x, y, int(f)) for f in frames]


def outside(vol, xyz, cw, ch, cd):
    """(len(xyz), cd, ch, cw) bool: the sample lies outside the volume"""
    n, h, w = vol.shape
    out = np.zeros((len(xyz), cd, ch, cw), dtype=bool)
    for i, (x, y, z) in enumerate(xyz):
        xs, ys, zs = np.arange(x, x + cw), np.arange(y, y + ch), np.arange(z, z + cd)
        out[i] = ((zs < 0) | (zs >= n))[:, None, None] | ((ys < 0) | (ys >= h))[None, :, None] | ((xs < 0) | (xs >= w))[None, None, :]
    return out


def read_native(call, xyz, cw, ch, cd):
    """call(xyz, cw, ch, cd, d_out, out_cap) -> whatever the door returns; the crops as (n, cd, ch, cw) u16 in front of it"""
    import torch
    t = torch.full((max(len(xyz), 1), cd, ch, cw, 2), 0xA5, dtype=torch.uint8, device="cuda")   # (every byte must be overwritten)
    ret = call(xyz, cw, ch, cd, t.data_ptr(), len(xyz) * cd * ch * cw * 2)
    return (t.cpu().numpy()[: len(xyz)].view("<u2")[..., 0],) + tuple(ret)


def damaged(mic, name, temporal, frame):
    """the file of volume `name` with `frame`'s table entry pointing at a well-formed stream of a frame one row shorter, appended to
    the file: a residual then expands to the wrong number of symbols (multiframecompress.go:170-172), a spatial frame runs out of
    tokens"""
    vol = volume(name)
    n, h, w = vol.shape
    good = V.Mic2File(mic.compress_multi_frame(vol, w, h, MAXV, temporal=temporal))
    short = V.Mic2File(mic.compress_multi_frame(np.ascontiguousarray(vol[:, : h - 1]), w, h - 1, MAXV, temporal=temporal))
    b, e = short.span(frame)
    struct.pack_into("<II", good.data, 20 + 8 * frame, len(good.data) - good.body, e - b)
    return bytes(good.data + short.data[b:e])
