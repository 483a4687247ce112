"""Strip files, crop origins and numpy expectations shared by the strip-file crop tests (test_strip_crop_plan_cpu.py,
test_gpu_strip_crops.py, strip_crops_chunking_check.py).  Nothing here calls the code under test: the files are written by the
encoders the caller hands in (the CPU oracle's, or the device's whole-image ones), and every expected crop is cut from the zero-padded
source pixels.  The images are the smallest at which the crop path can still go wrong, and quiet enough that strips of a few hundred
pixels still have a tANS table (the reference's encoder refuses small noisy inputs)."""
import struct

import numpy as np

# (cw, ch): a crop that straddles dword-aligned and 2-byte-aligned rows, an odd one narrower than a wave (rows side by side), one
# sample, and one larger than four of the five images
SHAPES = [(32, 16), (33, 9), (1, 1), (128, 80)]

# name -> (width, height, max_value, container, strips, states)
FILES = {
    "A": (96, 70, 4095, "PICS", 8, 2),       # strip height 9, the last strip 7 rows
    "B": (97, 53, 4095, "PICS", 5, 4),       # odd width: every second row of a strip is 2-byte-aligned only; values past 32768 and 65535
    "C": (96, 70, 4095, "PICA", 6, 2),       # quiet upper part, textured lower part: uneven boundaries, both predictors
    "D": (1040, 24, 4095, "PICS", 3, 8),     # the width class of the fused row decoder (1009 .. 2688 columns)
    "E": (40, 8, 4095, "PICS", 1, 2),        # a single unit
}
ORDER = ["A", "B", "C", "D", "E"]


def _noise(synth, w, h, seed):
    return synth.approx_gauss(h * w, seed).reshape(h, w)


def image(synth, name):
    """the source pixels of file `name`, (height, width) uint16"""
    w, h = FILES[name][:2]
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    if name == "A":
        img = 900 + 5 * x + 11 * y + 2.0 * _noise(synth, w, h, 11)
    elif name == "B":                        # a ramp of 900 a column, mod 2^16: every row crosses 2^15 and wraps at 2^16.  (max_value stays
        # 4095: it sizes the residual alphabet, and a 16-bit alphabet's table header alone outweighs a strip of a thousand pixels)
        img = np.rint(20 + 900 * x + 3 * y + 2.0 * _noise(synth, w, h, 12)).astype(np.int64) & 0xFFFF
    elif name == "C":                        # noise growing from row 25 on, bars from row 40 on (chosen with the oracle's PICA encoder)
        img = 800 + 3 * x + np.clip((y - 25) * 3 / 15.0, 0.6, 3) * _noise(synth, w, h, 1) + np.where(y >= 40, ((x // 8) % 2) * 40, 0)
    elif name == "D":
        img = 300 + 2 * x + 9 * y + 2.0 * _noise(synth, w, h, 14)
    else:
        img = 100 + 7 * x + 13 * y + 1.5 * _noise(synth, w, h, 15)
    return np.clip(np.rint(img), 0, 65535).astype(np.uint16)


def build(synth, pics, pica):
    """[(name, image, file bytes)] in ORDER.  pics(img, max_value, num_strips, nstates) / pica(img, max_value, num_strips) -> bytes"""
    out = []
    for name in ORDER:
        w, h, maxv, kind, strips, states = FILES[name]
        img = image(synth, name)
        img.setflags(write=False)
        data = pics(img, maxv, strips, states) if kind == "PICS" else pica(img, maxv, strips)
        assert bytes(data[:4]) == kind.encode(), name
        out.append((name, img, bytes(data)))
    return out


def oracle_encoders(mico):
    def pics(img, maxv, strips, states):
        rc, b = mico.pics_compress(img, maxv, strips, states)
        assert rc == 0, rc
        return b

    def pica(img, maxv, strips):
        rc, b = mico.pica_compress(img, maxv, strips)
        assert rc == 0, rc
        return b
    return pics, pica


class StripFile:
    """a PICS (parallelstrips.go) or PICA (parallelstripsadaptive.go) file taken apart: header, table, streams"""

    def __init__(self, data):
        self.data = bytearray(data)
        self.kind = bytes(self.data[:4]).decode()
        assert self.kind in ("PICS", "PICA")
        self.w, self.h, self.n = struct.unpack_from("<III", self.data, 4)
        self.body = 20 + 8 * self.n if self.kind == "PICS" else 16 + 16 * self.n

    def entry_at(self, k):
        """byte position of strip k's table entry"""
        return 20 + 8 * k if self.kind == "PICS" else 16 + 16 * k

    def rows(self, k):
        """[y0, y1) of strip k"""
        if self.kind == "PICS":
            sh, = struct.unpack_from("<I", self.data, 16)
            return k * sh, min(self.h, (k + 1) * sh)
        y0, = struct.unpack_from("<I", self.data, 16 + 16 * k)
        y1 = struct.unpack_from("<I", self.data, 32 + 16 * k)[0] if k + 1 < self.n else self.h
        return y0, y1

    def span(self, k):
        """[begin, end) of strip k's stream in the file"""
        off, ln = struct.unpack_from("<II", self.data, self.entry_at(k) + (0 if self.kind == "PICS" else 4))
        return self.body + off, self.body + off + ln

    def grad(self, k):
        """PICA: strip k kept the gradient predictor"""
        return bool(struct.unpack_from("<I", self.data, 16 + 16 * k + 12)[0] & 1)

    def head(self):
        return bytes(self.data[: self.body])


def _spread(files, cw, ch, seed):
    """a dozen seeded origins over all the files, some of them overhanging"""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(12):
        f = i % len(files)
        w, h = files[f][1].shape[1], files[f][1].shape[0]
        out.append((int(rng.randint(-cw // 2 - 1, w)), int(rng.randint(-ch // 2 - 1, h)), f))
    return out


def origins(files, cw, ch):
    """(x, y, file) triples of cw x ch crops over `files` (build()'s list): per file the four corners, a crop overhanging each
    side, one strictly inside a strip (where the strip is tall enough, else in its first rows), one across a strip seam, one wholly
    outside; then a crop twice and a dozen seeded random origins over all the files"""
    out = []
    for f, (name, img, data) in enumerate(files):
        h, w = img.shape
        m = StripFile(data)
        s = min(1, m.n - 1)                                              # a strip with a seam below it, if there is one
        y0, y1 = m.rows(s)
        out += [(0, 0, f), (w - cw, 0, f), (0, h - ch, f), (w - cw, h - ch, f),
                (-5, 3, f), (w - cw // 2 - 1, 3, f), (7, -3, f), (7, h - ch // 2 - 1, f),
                (9, y0 + 1 if y1 - y0 > ch + 1 else y0, f),
                (11, max(y1 - max(ch // 2, 1), 0) if m.n > 1 else h // 2, f),
                [(w, 0, f), (0, h, f), (-cw, 2, f), (3, -ch, f), (w + 9, h + 9, f)][f % 5]]
    out += [(13, 5, 0), (13, 5, 0)]
    return out + _spread(files, cw, ch, 1000 * cw + ch)


def expected(files, xyf, cw, ch):
    """the crops of the zero-padded sources: (len(xyf), ch, cw)"""
    out = np.zeros((len(xyf), ch, cw), dtype=np.uint16)
    pads = {}
    for i, (x, y, f) in enumerate(xyf):
        img = files[f][1]
        h, w = img.shape
        if f not in pads:
            pads[f] = np.zeros((h + 2 * ch, w + 2 * cw), dtype=np.uint16)
            pads[f][ch: ch + h, cw: cw + w] = img
        x, y = min(max(x, -cw), w) + cw, min(max(y, -ch), h) + ch          # (farther out is as empty)
        out[i] = pads[f][y: y + ch, x: x + cw]
    return out


def brute_plan(files, xyf, cw, ch):
    """(sorted (file, strip) units, number of (crop, strip) pairs with a non-empty overlap, strips of the named files), by
    enumerating every crop's coordinates against every strip's rows"""
    units, pieces = set(), 0
    heads = {f: StripFile(files[f][2]) for f in {f for _, _, f in xyf}}
    for x, y, f in xyf:
        m = heads[f]
        xs, ys = np.arange(x, x + cw), np.arange(y, y + ch)
        cols = int(((xs >= 0) & (xs < m.w)).sum())
        for k in range(m.n):
            y0, y1 = m.rows(k)
            if cols and int(((ys >= y0) & (ys < y1)).sum()):
                pieces += 1
                units.add((f, k))
    return sorted(units), pieces, sum(m.n for m in heads.values())
