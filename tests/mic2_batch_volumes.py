"""Volumes, job lists and reference results shared by the tests of the MIC2 whole-volume batches (test_mic2_batch_plan_cpu.py,
test_gpu_mic2_batch.py, mic2_batch_chunking_check.py).  The references are the single calls; nothing here calls the batch doors."""
import numpy as np

import mic2_multi_volumes as M
from mic2_multi_volumes import Mic2File, cuts_of   # noqa: F401  (shared as they are)

# the batch of the byte-identity tests: (volume, temporal), in this order
JOBS = [("xr12", True), ("tiny", False), ("narrow", True), ("wrap16", True), ("xr12", False), ("one", True), ("two", True), ("wrap16", False)]


def volumes(synth):
    """name -> (frames (n, h, w) uint16, max_value).  Beside the four of mic2_multi_volumes: "one" and "two", the first frame(s) of
    the 12-bit volume -- a temporal file of frame 0 alone, and of one residual --; "still", frames [0, 0, 1, 1, 1] of it -- as a
    temporal volume its residuals 1, 3 and 4 are all zero, which the encoder refuses --; "col" and "row", its first four frames cut to
    one column and to one row, which no pipeline codes (every coded frame is larger than the raw one)."""
    xr, xmax = M.volume_12bit(synth)
    out = dict(xr12=(xr, xmax), wrap16=M.volume_16bit(synth), narrow=M.volume_narrow(synth), tiny=M.volume_tiny(synth))
    out["one"] = (np.ascontiguousarray(xr[:1]), xmax)
    out["two"] = (np.ascontiguousarray(xr[:2]), xmax)
    out["still"] = (np.ascontiguousarray(xr[[0, 0, 1, 1, 1]]), xmax)
    out["col"] = (np.ascontiguousarray(xr[:4, :, :1]), xmax)
    out["row"] = (np.ascontiguousarray(xr[:4, :1, :]), xmax)
    return out


def single_encode(mic, vol, maxv, temporal):
    """(code, file or None) of the single call for that volume alone"""
    try:
        return mic.MIC_OK, mic.compress_multi_frame(vol, vol.shape[2], vol.shape[1], maxv, temporal=temporal)
    except mic.MicError as e:
        return e.code, None


def single_decode(mic, data):
    """(code, frames or None) of the single call for that file alone"""
    try:
        return mic.MIC_OK, np.asarray(mic.decompress_multi_frame(data))
    except mic.MicError as e:
        return e.code, None


def first_refused_frame(mic, vol, maxv, temporal):
    """the first frame, in frame order, that the unit codec refuses of a volume the single call refuses: a spatial frame is judged
    by the single-frame call; a temporal volume's residual i by the temporal single call on frames i - 1 .. i (frame i - 1 spatial,
    which codes if it did as a frame of its own)"""
    n, h, w = vol.shape
    for f in range(n):
        if not temporal or f == 0:
            try:
                mic.compress_single_frame(vol[f], w, h, maxv)
            except mic.MicError:
                return f
        else:
            try:
                mic.compress_single_frame(vol[f - 1], w, h, maxv)
            except mic.MicError:
                continue                                   # (cannot be told apart this way; frames before it decide)
            if single_encode(mic, np.ascontiguousarray(vol[f - 1: f + 1]), maxv, True)[0] != mic.MIC_OK:
                return f
    return -1


def units_px(vols):
    """pixels of every unit of the volumes, volume by volume and frame by frame: what the cut rule is stated over"""
    return [v.shape[1] * v.shape[2] for v in vols for _ in range(v.shape[0])]


def unit_names(vols):
    """(volume, frame) of every unit"""
    return [(i, f) for i, v in enumerate(vols) for f in range(v.shape[0])]


def damage(data, frame):
    """the file with a byte flipped in the middle of that frame's stream (mic2_multi_chunking_check.py)"""
    m = Mic2File(data)
    b, e = m.span(frame)
    m.data[(b + e) // 2] ^= 0x5A
    return bytes(m.data)
