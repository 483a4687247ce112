"""The frame lists of tests/test_gpu_wavelet_mixed.py, shared with tests/test_wavelet_mixed_cpu.py (which asks the oracle, without a
device, that every frame of them compresses except the 3 x 3 one), and the cut rule of mic_hip_wavelet_v2_batch_plan restated."""
import numpy as np


def image(rows, cols, depth, seed):
    """a ramp with a little noise: few distinct symbols, so that the 4-state FSE stage takes even small and thin frames
    (tests/test_gpu_wavelet_seams.py's _image, restated)"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    px = (y * 7 + x * 3) % 97 + rng.integers(0, 3, (rows, cols))
    if depth == 16:
        px = px * 613 + rng.integers(0, 2, (rows, cols))
    return px.astype(np.uint16)


def escape_frame(rows=512, cols=512, seed=7):
    """16-bit, LL mean above 32767: every LL coefficient is a three-word escape, so P words never cover P coefficients"""
    rng = np.random.default_rng(seed)
    return (40000 + rng.integers(0, 64, (rows, cols))).astype(np.uint16)


# (rows, cols, levels, depth): the tiling list of the seams file -- one block beside many, level counts 0 (the 1-wide frames) and 1 .. 8,
# odd widths at whatever offset the neighbours leave
TILING = [(125, 122, 1, 12), (128, 124, 2, 12), (129, 125, 3, 12), (254, 246, 4, 16), (256, 248, 5, 12), (257, 249, 6, 16),
          (515, 494, 7, 12), (129, 496, 8, 16), (254, 497, 1, 16), (125, 990, 2, 12), (257, 1985, 3, 16), (515, 990, 8, 16),
          (1, 700, 5, 12), (700, 1, 5, 12), (2, 333, 4, 12), (3, 3, 8, 16), (2, 2, 1, 12), (64, 1985, 6, 12)]
# n = 8191, 8191, 8193, 16383, 16385 (WS_T = 8192 positions per group), each between two frames of other sizes
SCAN = [(33, 35), (1, 8191), (61, 67), (8191, 1), (21, 29), (3, 2731), (17, 47), (129, 127), (13, 43), (145, 113), (5, 9)]


def tiling_jobs():
    """[(image, max_value, levels)] of TILING"""
    return [(image(r, c, d, r * 3 + c), (1 << d) - 1, lv) for r, c, lv, d in TILING]


def scan_jobs():
    return [(image(r, c, 12, r * c), 4095, 8) for r, c in SCAN]


def wide_jobs():
    """the "one wide coefficient" frame (160 x 210, one value 65535: exactly one coefficient outside +-32767) between two frames of
    other shapes"""
    mid = image(160, 210, 12, 42) // 16
    mid[81, 101] = 65535
    return [(image(97, 301, 12, 5), 4095, 4), (mid, 65535, 3), (image(200, 131, 12, 6), 4095, 2)]


LEVEL_SHAPES = [(257, 249, 6), (129, 496, 4), (300, 200, 3)]


def level_images():
    return [(image(r, c, 12, r + c), 4095, lv) for r, c, lv in LEVEL_SHAPES]


# ---- the cut rule, restated -------------------------------------------------------------------------------------------------------
def unit_ws_bytes(px):
    """what a unit of px pixels takes of the workspace (the tier-2 slabs)"""
    tokc, ts = 4 * px + 16, 65536
    return tokc * 4 + (8 + 131080 + 2 * tokc + 16) + (2 * px + 8) * 8 + px // 8 + ts * 4 * 6 + ts * 2 + 8192


def per_frame(mp):
    """bytes a frame takes in a sub-batch whose largest frame has mp pixels"""
    return unit_ws_bytes(2 * mp + 16) + 8 * mp


def plan(rc, budget, limit=65535, px_target=1 << 30):
    """frames in order while they stay within budget // per_frame(largest so far), `limit` frames and px_target pixels; the first joins"""
    px = [int(r) * int(c) for r, c in rc]
    cuts, i = [0], 0
    while i < len(px):
        i0, mp, total = i, 0, 0
        while i < len(px):
            mp = max(mp, px[i])
            cnt = i - i0
            if cnt > 0 and (cnt + 1 > max(1, budget // per_frame(mp)) or cnt >= limit or total >= px_target):
                break
            total += px[i]
            i += 1
        cuts.append(i)
    return cuts
