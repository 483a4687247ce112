"""The host reference of the scaled MIC3 patch readers (the _scaled doors, include/mic_hip.h), shared by test_wsi_scaled_cpu.py,
test_gpu_wsi_scaled.py and wsi_scaled_chunking_check.py.  Nothing here calls the code under test.

A call has one scale num / den (reduced).  In units of 1 / den of a level pixel, measured from the patch origin, output pixel j covers
[j * num, (j + 1) * num) and level pixel k covers [k * den, (k + 1) * den); the weight of (j, k) is the length of the overlap.  Per
channel S = sum_l wy(r, l) * sum_k wx(j, k) * p(x + k, y + l) over the zero-extended level and v = (S + num^2 // 2) // num^2, all in
Python / int64 integers (S stays below 2^36)."""
import math

import numpy as np


def reduce(num, den):
    g = math.gcd(num, den)
    return num // g, den // g


def accepted(num, den):
    """the doors' judgement of a scale"""
    if num <= 0 or den <= 0:
        return False
    num, den = reduce(num, den)
    return den <= num <= 16 * den and num <= 1024


def extent(pw, ph, num, den):
    """the source rectangle of a pw x ph patch: ceil(pw * num / den) x ceil(ph * num / den) level pixels"""
    return -(-pw * num // den), -(-ph * num // den)


def weights(count, num, den):
    """(count, ceil(count * num / den)) int64: the overlap of output pixel j with source pixel k"""
    n_src = -(-count * num // den)
    j = np.arange(count, dtype=np.int64)[:, None]
    k = np.arange(n_src, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((j + 1) * num, (k + 1) * den) - np.maximum(j * num, k * den))


def source_rect(level_img, x, y, sw, sh):
    """the sw x sh level pixels at (x, y), zero outside the level, and the mask of those inside it"""
    lh, lw = level_img.shape[:2]
    out = np.zeros((sh, sw) + level_img.shape[2:], dtype=np.int64)
    inside = np.zeros((sh, sw), dtype=bool)
    x0, x1, y0, y1 = max(x, 0), min(x + sw, lw), max(y, 0), min(y + sh, lh)
    if x0 < x1 and y0 < y1:
        out[y0 - y: y1 - y, x0 - x: x1 - x] = level_img[y0:y1, x0:x1]
        inside[y0 - y: y1 - y, x0 - x: x1 - x] = True
    return out, inside


def resample(level_img, xy, pw, ph, num, den):
    """-> (samples (n, ph, pw[, C]) of the level's dtype, outside (n, ph, pw) bool: the pixel's footprint lies wholly outside the level)"""
    num, den = reduce(num, den)
    sw, sh = extent(pw, ph, num, den)
    wx, wy = weights(pw, num, den), weights(ph, num, den)
    out = np.zeros((len(xy), ph, pw) + level_img.shape[2:], dtype=level_img.dtype)
    outside = np.ones((len(xy), ph, pw), dtype=bool)
    for i, (x, y) in enumerate(xy):
        src, inside = source_rect(level_img, int(x), int(y), sw, sh)
        rows = np.tensordot(wy, src, axes=([1], [0]))                     # (ph, sw[, C])
        s = np.tensordot(wx, rows, axes=([1], [1]))                       # (pw, ph[, C])
        s = np.swapaxes(s, 0, 1)
        assert s.max(initial=0) < 2 ** 36
        out[i] = ((s + num * num // 2) // (num * num)).astype(level_img.dtype)
        touched = (wy @ inside.astype(np.int64)) @ wx.T                    # (ph, pw): the footprint's area inside the level
        outside[i] = touched == 0
    return out, outside


def pyramid_2x(img):
    """the rule the pyramid is built by (wsipyramid.go:27,51): (a + b + c + d + 2) / 4 over whole 2 x 2 blocks, odd trailing pixels dropped"""
    h, w = img.shape[0] // 2, img.shape[1] // 2
    v = img[: 2 * h, : 2 * w].astype(np.int64)
    return ((v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) // 4).astype(img.dtype)
