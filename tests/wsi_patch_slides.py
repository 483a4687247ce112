"""Slides and MIC3 file surgery for tests/test_gpu_wsi_patches.py (no test in here; its child process imports it too)."""
import numpy as np

W, H, TILE, LEVELS = 200, 150, 64, 3
FORMATS = ("rgb", "grey8", "grey16")
NOISE_TILE = 1          # level-0 tile (1, 0): whole-tile noise; raw_plane_file stores it raw
WHITE_TILE, BLACK_TILE = 6, 4   # level-0 tiles (2, 1) and (0, 1): constant planes


def fmt_args(fmt):
    return dict(channels=3, bits_per_sample=8) if fmt == "rgb" else dict(channels=1, bits_per_sample=16 if fmt == "grey16" else 8)


def slide(fmt):
    """A smooth ramp; uniform noise over the whole tile (1, 0); white over the whole tile (2, 1); black over (0, 1).
    The noise is 7 bits wide (6 in the 16-bit slide): wider noise has more distinct residuals than the reference's
    normaliser takes in a 4096-pixel plane, and CompressWSI then fails."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = (xx + 2 * yy) // 3
    if fmt == "rgb":
        img = np.stack([ramp % 256, (ramp // 2) % 256, (255 - ramp) % 256], -1).astype(np.uint8)
        noise, white = rng.integers(0, 128, (H, W, 3)).astype(np.uint8), 255
    elif fmt == "grey8":
        img, noise, white = (ramp % 256).astype(np.uint8), rng.integers(0, 128, (H, W)).astype(np.uint8), 255
    else:
        img, noise, white = (ramp * 19).astype(np.uint16), (2000 + rng.integers(0, 64, (H, W))).astype(np.uint16), 4095      # 12-bit range, 6-bit noise
    img[0:64, 64:128] = noise[0:64, 64:128]
    img[64:128, 128:192] = white
    img[64:128, 0:64] = 0
    return img


class Mic3File:
    """header fields, level table and tile blobs of a MIC3 file (wsiformat.go:99-165), and the file again from edited blobs"""

    def __init__(self, data):
        data = bytes(data)
        self.nlev = int.from_bytes(data[28:30], "little")
        self.total = int.from_bytes(data[32:40], "little")
        self.planes = 3 if data[24] == 3 else 1
        self.head = bytearray(data[: 48 + 20 * self.nlev])
        idx = 48 + 20 * self.nlev
        body = idx + 16 * self.total
        self.levels = []            # (w, h, tiles_x, tiles_y, first)
        for i in range(self.nlev):
            self.levels.append(tuple(int.from_bytes(data[48 + 20 * i + 4 * k: 52 + 20 * i + 4 * k], "little") for k in range(5)))
        self.blobs = []
        for t in range(self.total):
            off = int.from_bytes(data[idx + 16 * t: idx + 16 * t + 8], "little")
            n = int.from_bytes(data[idx + 16 * t + 8: idx + 16 * t + 16], "little")
            self.blobs.append(bytearray(data[body + off: body + off + n]))

    def plane_spans(self, t):
        """[(offset of the plane in blob t, its length)]: RGB = three u32 lengths, then the planes; grey = the blob"""
        b = self.blobs[t]
        if self.planes == 1:
            return [(0, len(b))]
        lens = [int.from_bytes(b[4 * i: 4 * i + 4], "little") for i in range(3)]
        return [(12 + sum(lens[:i]), lens[i]) for i in range(3)]

    def modes(self, t):
        """the mode byte of every plane of tile t"""
        return [self.blobs[t][o] for o, _ in self.plane_spans(t)]

    def bytes(self):
        out, off = bytearray(self.head), 0
        for b in self.blobs:
            out += off.to_bytes(8, "little") + len(b).to_bytes(8, "little")
            off += len(b)
        for b in self.blobs:
            out += b
        return bytes(out)


def tile_planes(fmt, img, tx, ty):
    """the u16 planes compressWSIPlane sees for level-0 tile (tx, ty): zero-padded; RGB through YCoCg-R with Co / Cg zigzagged"""
    t = np.zeros((TILE, TILE) + img.shape[2:], dtype=img.dtype)
    part = img[ty * TILE: (ty + 1) * TILE, tx * TILE: (tx + 1) * TILE]
    t[: part.shape[0], : part.shape[1]] = part
    if fmt != "rgb":
        return [t.astype(np.uint16)]
    r, g, b = (t[:, :, k].astype(np.int32) for k in range(3))
    co = r - b
    tmp = b + (co >> 1)
    cg = g - tmp
    y = tmp + (cg >> 1)
    zz = lambda v: (((v << 1) ^ (v >> 15)) & 0xFFFF)
    return [y.astype(np.uint16), zz(co).astype(np.uint16), zz(cg).astype(np.uint16)]


def raw_plane_file(fmt, img, data):
    """`data` (the MIC3 file of img) with the planes of the noise tile stored raw (planeRaw, wsicompress.go:403-414, :515-523): the
    same pixels.  The reference's encoder takes that branch on ErrIncompressible only, which no 4096-pixel plane it can code at all
    returns (tests/test_oracle_wavelet_wsi.py), so the file is made by hand, as grey_raw_container does there."""
    f = Mic3File(data)
    tx, ty = NOISE_TILE % f.levels[0][2], NOISE_TILE // f.levels[0][2]
    planes = [bytes([3]) + p.astype("<u2").tobytes() for p in tile_planes(fmt, img, tx, ty)]
    f.blobs[NOISE_TILE] = bytearray((b"".join(len(p).to_bytes(4, "little") for p in planes) if f.planes == 3 else b"") + b"".join(planes))
    return f.bytes()


def make_file(mic, fmt):
    img = slide(fmt)
    data = mic.compress_wsi(img, W, H, tile_w=TILE, tile_h=TILE, levels=LEVELS, **fmt_args(fmt))
    return img, raw_plane_file(fmt, img, data)


def origins(lw, lh, tw, th, pw, ph):
    """tile-aligned, straddling four tiles, overhanging each edge, fully outside, negative, repeated"""
    o = [(0, 0), (tw, th), (tw - pw // 2 - 1, th - ph // 2 - 1),
         (-pw // 2, 10), (10, -ph // 2), (lw - pw // 2, 7), (7, lh - ph // 2), (-3, -2), (lw - 1, lh - 1),
         (lw, 0), (0, lh), (-pw, 0), (0, -ph), (lw + 50, lh + 50), (-1000, -1000)]
    return o + [o[2], o[2], o[0]]


def expected(level_img, xy, pw, ph):
    """the patches cut from the level image padded with zeros"""
    lh, lw = level_img.shape[:2]
    out = np.zeros((len(xy), ph, pw) + level_img.shape[2:], dtype=level_img.dtype)
    for i, (x, y) in enumerate(xy):
        x0, x1, y0, y1 = max(x, 0), min(x + pw, lw), max(y, 0), min(y + ph, lh)
        if x0 < x1 and y0 < y1:
            out[i, y0 - y: y1 - y, x0 - x: x1 - x] = level_img[y0:y1, x0:x1]
    return out
