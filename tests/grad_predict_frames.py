"""Frames, token streams and PICA images aimed at the seams of k_dec_predict_grad (csrc/mic_decode_px.hip), made on the CPU:
tests/test_gpu_grad_predict.py runs them through the device, tests/test_grad_predict_cpu.py shows without one that every case
reaches the seam it is named for.  Nothing here calls the code under test; the oracle (mico) only makes tokens and streams.

The kernel's seams: 64-row bands (lane r owns row 64 b + r; lane 63 hands its row to lane 0 of the next band through LDS),
four-pixel groups (N / NW by DPP from the lane above, NE of a group's column 3 handed over inside the step; at the right edge
NE = NW, decided apart for columns 0..2 and column 3 of a group, so W mod 4 are four code paths), 8-byte symbol loads with a
sample-by-sample tail for the frame's last group, four escape-flag bits per group cut out of two flag words (a group at
p mod 32 in 29..31 straddles them; a frame of a multiple of 32 pixels reads the slab's spare word), three row-buffer classes by
width (W <= 4088, <= 8184, <= 32768; wider frames take the row above from the output frame) and 16-bit wrap-around of the
predicted pixel.

A forced escape is a pixel set to 0 or to the maximum value, whichever lies further from its prediction: that is at least half the
range away and so at least thr = 2^(depth-1) - 1: an escape whatever the neighbourhood holds."""
import functools
from collections import namedtuple

import numpy as np

from tokeniser_streams import grad_predict

# aim: {"esc": pixels (y, x) that must be escapes, "plain": pixels that must not be, "props": names of frame properties}
Case = namedtuple("Case", "name img maxv aim")

SEAM_ROWS = (62, 63, 64, 65, 127, 128)


def predict_at(img, y, x):
    """the reference's prediction of pixel (y, x) from the pixels above and left of it (deltagradrlecompressu16.go:79-121)"""
    h, w = img.shape
    if y == 0:
        return int(img[0, x - 1]) if x else 0
    if x == 0:
        return int(img[y - 1, 0])
    nw = int(img[y - 1, x - 1])
    return grad_predict(int(img[y, x - 1]), int(img[y - 1, x]), nw, int(img[y - 1, x + 1]) if x + 1 < w else nw)


def force(img, maxv, pixels):
    """the pixels, in raster order, set to 0 or maxv against their prediction"""
    half = (int(maxv) + 1) // 2
    for y, x in sorted(set(pixels)):
        img[y, x] = 0 if predict_at(img, y, x) >= half else maxv
    return img


def seam_pixels(w, h, variant):
    """(0, 0), the end of row 0, the frame's last pixel; in the rows around the band seams column 0, columns 1..5 and the last five
    columns -- every other column of every other of these rows: the four variants take the four quarters, so that plain pixels
    stay beside, above and below the escapes (at 8 bits a pixel under AND right of a forced one would escape too, and a row of
    escapes checks no prediction); the pairs "column 4 q + 3 of row y / column 4 q + 4 of row y - 1": both
    escapes (rows 20 and 64) and the upper one alone (rows 40 and 128)"""
    esc = {(0, 0), (0, w - 1), (h - 1, w - 1)}
    plain = set()
    cols = sorted({c for c in list(range(6)) + list(range(w - 5, w)) if 0 <= c < w})
    for n, y in enumerate(SEAM_ROWS):
        if y < h and (n + variant) % 2 == 0:
            esc |= {(y, c) for c in cols if (c + (variant >> 1)) % 2 == 0}
    q = 1 if w < 64 else 5
    if 4 * q + 4 < w:
        for y, both in ((20, True), (64, True), (40, False), (128, False)):
            if y < h:
                esc.add((y - 1, 4 * q + 4))
                if both:
                    esc.add((y, 4 * q + 3))
                else:
                    esc.discard((y, 4 * q + 3)); plain.add((y, 4 * q + 3))
    return esc, plain - esc


def _props(w, h, esc):
    """straddle: an escape e of a group that starts at pixel p with (p mod 32) + (e - p) >= 32 -- its flag bit comes from the
    second word of the funnel shift (counted at odd widths, where the groups take every phase); spare: the pixel count is a
    multiple of 32 and the last pixel an escape -- the group of the last pixel reads the word behind the flags"""
    props = set()
    for y, x in esc:
        p = y * w + (x & ~3)
        if w % 2 and (p % 32) + (x & 3) >= 32:
            props.add("straddle")
    if (w * h) % 32 == 0 and (h - 1, w - 1) in esc:
        props.add("spare")
    return props


def seam_case(name, img, maxv, variant):
    h, w = img.shape
    esc, plain = seam_pixels(w, h, variant)
    force(img, maxv, esc)
    return Case(name, img, maxv, {"esc": sorted(esc), "plain": sorted(plain), "props": _props(w, h, esc)})


def tiny_pattern(synth, w, h, maxv=255):
    """low amplitude around mid level: codable at 8 bits down to one column (at 12 bits the narrow ones are incompressible)"""
    y, x = np.mgrid[0:h, 0:w]
    noise = (synth.hash_u64(w * h, 7 * w + h) % np.uint64(3)).astype(np.int64).reshape(h, w)
    return (maxv // 2 + y % 5 + x % 3 + noise).astype(np.uint16)


def ramp(synth, w, h, mod=4096):
    """the ramp of test_gpu_predict_rows._wave2_ramp"""
    noise = (synth.hash_u64(w * h, w + h) % np.uint64(5)).astype(np.int64).reshape(h, w)
    return ((np.add.outer(np.arange(h) * 7, np.arange(w) // 8) + noise) % mod).astype(np.uint16)


def tiny_cases(synth):
    return [seam_case(f"tiny-{w}x{h}-v{v}", tiny_pattern(synth, w, h), 255, v)
            for w in range(1, 10) for h in (63, 64, 65, 128, 129) for v in range(4)]


def band_cases(synth):
    return [seam_case(f"band-{w}x{h}-v{v}", ramp(synth, w, h), 4095, v)
            for w in (63, 64, 65, 255, 257) for h in (63, 64, 65, 128, 129, 193) for v in range(4)]


CLASS_WIDTHS = (4087, 4088, 4089, 8128, 8129, 8184, 8185, 32767, 32768)


def class_cases(synth):
    """both sides of every row-buffer class and of mic_pred_bit's 8128 / 8129, one row, two rows, a band and a row"""
    return [seam_case(f"class-{w}x{h}", ramp(synth, w, h), 4095, (n + k) % 4)
            for n, w in enumerate(CLASS_WIDTHS) for k, h in enumerate((1, 2, 65))]


def deep_cases(synth):
    """16 bits: every fifth pixel of every third row has bit 15 set against a neighbourhood that has not"""
    out = []
    for w, h in ((258, 66), (4089, 65)):
        img = ramp(synth, w, h, 65536)
        img[::3, ::5] ^= 0x8000
        esc = [(0, 0), (0, 5 * ((w - 1) // 5)), (3, 5), (63, 255), (63, 0), (63, 5 * ((w - 1) // 5))]
        out.append(Case(f"deep-{w}x{h}", img, 65535, {"esc": sorted(set(esc)), "plain": [(1, 1), (64, 1)], "props": set()}))
    return out


FAMILIES = {"tiny": tiny_cases, "band": band_cases, "class": class_cases, "deep": deep_cases}


@functools.lru_cache(maxsize=None)
def family(synth, name):
    """the cases of one family, built once"""
    return tuple(FAMILIES[name](synth))


@functools.lru_cache(maxsize=None)
def oracle_streams(mico, synth, name):
    """the oracle's CompressSingleFrameGrad stream of every case of a family (b"" where it refuses the frame)"""
    return tuple(mico.compress_single_frame_grad(cs.img, cs.maxv)[1] for cs in family(synth, name))


# ---- streams no encoder writes ----------------------------------------------------------------------------------------------
Stream = namedtuple("Stream", "name stream w h maxv k tok structural")

WRAP_FRAMES = ((70, 258, 12), (66, 4089, 12), (130, 61, 12), (65, 8185, 12), (129, 1023, 16))
DAMAGE_FRAMES = ((3, 2.0, (70, 258)), (4, 60.0, (66, 4089)), (5, 10.0, (130, 61)), (6, 167.0, (9, 8185)), (7, 4.0, (65, 1009)))


def header_positions(tok):
    """indices of the run / chunk headers of a token stream (rledecompressu16.go:59-85)"""
    mid = (1 << (int(tok[0]).bit_length() - 1)) - 1
    pos, i = set(), 1
    while i < tok.size:
        pos.add(i)
        c = int(tok[i])
        i += 2 if c <= mid else 1 + c - mid
    return pos


@functools.lru_cache(maxsize=None)
def wrapping_streams(mico, synth):
    """The gradient tokens of XR-like frames with 1..39 literal symbols replaced by arbitrary values below the delimiter (the
    recipe of test_rows_predictor_wrapping_streams_agree_with_the_oracle) and coded again: pixels leave 0..maxv and wrap around
    16 bits, and the wrapped value is W / N / NW / NE of the pixels behind it.  k = 0 is the clean stream.  structural: a
    replaced token was a header, so the stream's layout changed too."""
    rng = np.random.default_rng(21)
    out = []
    for seed, (h, w, depth) in enumerate(WRAP_FRAMES, 1):
        img = synth.xr_like(cols=w, rows=h, depth=depth, seed=seed, noise=8.0)
        maxv = (1 << depth) - 1
        tok = mico.grad_delta_rle_compress(img, maxv)
        heads = header_positions(tok)
        for k in range(14):
            t = tok.copy()
            structural = False
            if k:
                mid = (1 << (int(t[0]).bit_length() - 1)) - 1
                cand = np.nonzero((t[4:] > 8) & (t[4:] < mid))[0] + 4
                pick = rng.choice(cand, size=min(cand.size, int(rng.integers(1, 40))), replace=False)
                t[pick] = rng.integers(0, max(int(t[0]) - 1, 2), pick.size).astype(np.uint16)
                structural = any(int(i) in heads for i in pick)
            rc, stream = mico.fse_compress(t, 2)
            if rc == 0:
                out.append(Stream(f"wrap-{w}x{h}-{k}", stream, w, h, maxv, k, t, structural))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def damaged_streams(mico, synth):
    """The recipe of test_wide_frames_with_damaged_tokens_agree_with_the_oracle on gradient tokens: zero counts, headers that
    point past the end or into a chunk, streams that stop early -- coded again so that the entropy stage accepts them."""
    rng = np.random.default_rng(17)
    out = []
    for seed, noise, (h, w) in DAMAGE_FRAMES:
        img = synth.xr_like(cols=w, rows=h, depth=12, seed=seed, noise=noise)
        tok = mico.grad_delta_rle_compress(img, 4095)
        for k in range(48):
            t = tok.copy()
            for _ in range(int(rng.integers(1, 5))):
                i = int(rng.integers(1, t.size))
                t[i] = (0, 1, 2, int(t[0]), int(t[0]) // 2 + 1, int(rng.integers(0, int(t[0]) + 1)))[int(rng.integers(0, 6))]
            if k % 8 == 2:
                t = t[: int(rng.integers(3, t.size))]
            rc, stream = mico.fse_compress(t, 2)
            if rc == 0:
                out.append(Stream(f"damaged-{w}x{h}-{k}", stream, w, h, 4095, k, t, True))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_decodes(mico, synth, which):
    """[(rc, pixels or None)] of the oracle's own decoder for wrapping_streams / damaged_streams"""
    streams = wrapping_streams(mico, synth) if which == "wrapping" else damaged_streams(mico, synth)
    return tuple(mico.decompress_single_frame_grad(s.stream, s.w, s.h) for s in streams)


def stream_counts(streams, results):
    """what the floors of both tests are counted from.  results: [(rc, pixels)] per stream"""
    clean = {(s.w, s.h): px for s, (rc, px) in zip(streams, results) if s.k == 0 and rc == 0}
    ok = [(s, px) for s, (rc, px) in zip(streams, results) if rc == 0]
    return {"coded": len(streams), "decodable": len(ok), "refused": len(streams) - len(ok),
            "differing": sum(1 for s, px in ok if s.k and (s.w, s.h) in clean and not np.array_equal(px, clean[(s.w, s.h)])),
            "above_maxv": sum(1 for s, px in ok if int(px.max()) > s.maxv)}


WRAP_FLOORS = {"decodable": 50, "differing": 40, "above_maxv": 30}
DAMAGE_FLOORS = {"coded": 150, "decodable": 60, "refused": 40}


# ---- PICA ---------------------------------------------------------------------------------------------------------------------
PICA_SHAPES = ((4089, 260, 4), (8185, 200, 3), (258, 517, 8), (4088, 130, 2), (32768, 130, 2))
WIDEST = 32768                                              # the widest frame the gradient row buffer holds (PR_MAX_W)


def wave_image(synth, w, h, kind):
    """a diagonal wave: along (x + y) / 23 every strip picks the gradient predictor, along (x - y) / 11 the avg predictor"""
    y, x = np.mgrid[0:h, 0:w]
    noise = (synth.hash_u64(w * h, w + 3 * h) % np.uint64(7)).astype(np.int64).reshape(h, w) - 3
    arg = (x + y) / 23.0 if kind == "grad" else (x - y) / 11.0
    return (2000 + np.rint(1500 * np.sin(arg)).astype(np.int64) + noise).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def pica_images(synth):
    """(name, image, strips, kind)"""
    return tuple((f"pica-{kind}-{w}x{h}", wave_image(synth, w, h, kind), n, kind) for w, h, n in PICA_SHAPES for kind in ("grad", "avg"))


def pica_flags(blob):
    """the predictor flag of every strip, from the file's 16-byte entries (parallelstripsadaptive.go:118-128)"""
    n = int.from_bytes(blob[12:16], "little")
    return [int.from_bytes(blob[16 + 16 * s + 12: 32 + 16 * s], "little") for s in range(n)]


def pica_starts(blob):
    n = int.from_bytes(blob[12:16], "little")
    return [int.from_bytes(blob[16 + 16 * s: 20 + 16 * s], "little") for s in range(n)]
