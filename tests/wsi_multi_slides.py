"""Slides and patch lists for tests/test_wsi_multi_plan_cpu.py and tests/test_gpu_wsi_multi_patches.py (no test in here; the GPU
test's child process imports it too).  Built on wsi_patch_slides: slide A is its slide, with the raw-plane, white and black tiles.

    A  200 x 150, tiles 64 x 64, 3 levels
    B   90 x  70, tiles 32 x 48, 2 levels   (non-square tiles, another size than A's)
    C   41 x  33, tiles 16 x 16, 3 levels   (odd width: odd row starts for the 16-bit gather)

B holds a ramp plus 2-bit noise, C a ramp alone -- narrower than wsi_patch_slides.slide's noise, whose docstring says why wider noise
will not do: their planes are smaller still, and the reference's CompressWSI refuses C's 256-pixel planes with any noise at all
(tests/test_wsi_multi_plan_cpu.py checks that the oracle encodes every slide here)."""
import numpy as np

import wsi_patch_slides as S

NAMES = ("A", "B", "C")
GEOMETRY = {"A": (S.W, S.H, S.TILE, S.TILE, S.LEVELS), "B": (90, 70, 32, 48, 2), "C": (41, 33, 16, 16, 3)}   # w, h, tile_w, tile_h, levels
PATCHES = [(24, 20), (71, 37), (1, 1)]
OTHER_FORMAT = {"rgb": "grey8", "grey8": "grey16", "grey16": "grey8"}      # slide D of a call: slide B in this format


def image(name, fmt):
    if name == "A":
        return S.slide(fmt)
    w, h = GEOMETRY[name][:2]
    rng = np.random.default_rng(11 if name == "B" else 12)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = (3 * xx + 2 * yy) // 2 + (rng.integers(0, 4, (h, w)) if name == "B" else 0)
    if fmt == "rgb":
        return np.stack([ramp % 256, (ramp // 2 + 40) % 256, (255 - ramp) % 256], -1).astype(np.uint8)
    if fmt == "grey8":
        return (ramp % 256).astype(np.uint8)
    return (ramp * 13 + 100).astype(np.uint16)                              # 12-bit range


def oracle_file(mico, name, fmt):
    """the slide through the oracle's CompressWSI -> (rc, file); A with its noise tile rewritten raw, as S.make_file does"""
    img = image(name, fmt)
    _, _, tw, th, levels = GEOMETRY[name]
    rc, data = (mico.wsi_compress(img, tw, th, levels) if fmt == "rgb" else mico.wsi_compress_grey(img, tw, th, levels))
    if rc == 0 and name == "A":
        data = S.raw_plane_file(fmt, img, data)
    return rc, data


def device_file(mic, name, fmt):
    """the slide through the library's own encoder"""
    if name == "A":
        return S.make_file(mic, fmt)[1]
    w, h, tw, th, levels = GEOMETRY[name]
    return mic.compress_wsi(image(name, fmt), w, h, tile_w=tw, tile_h=th, levels=levels, **S.fmt_args(fmt))


def groups(parsed, pw, ph, slides=None):
    """[(slide, level, [(x, y)])]: S.origins of every level of every slide; parsed: [Mic3File]"""
    out = []
    for s, f in enumerate(parsed):
        if slides is not None and s not in slides:
            continue
        for level, (lw, lh, _, _, _) in enumerate(f.levels):
            tw, th = (int.from_bytes(f.head[16 + 4 * k: 20 + 4 * k], "little") for k in range(2))
            out.append((s, level, S.origins(lw, lh, tw, th, pw, ph)))
    return out


def patch_list(parsed, pw, ph, slides=None, seed=7):
    """(x, y, slide, level) of every group, concatenated and shuffled: neighbours of the call belong to different slides and levels"""
    q = [(x, y, s, level) for s, level, xy in groups(parsed, pw, ph, slides) for x, y in xy]
    order = np.random.default_rng(seed).permutation(len(q))
    return [q[i] for i in order]


def tile_size(f):
    return tuple(int.from_bytes(f.head[16 + 4 * k: 20 + 4 * k], "little") for k in range(2))
