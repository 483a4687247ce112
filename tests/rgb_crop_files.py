"""The RGB files the crop tests read (test_rgb_crop_plan_cpu.py, test_gpu_rgb_crops.py): tests/test_gpu_rgb_batch.py's plane-mode set
as the CPU oracle's CompressRGB blobs and MICR files, and two blobs assembled by hand -- the format allows any plane to be raw
([Y_len][Co_len][Cg_len], then per plane a mode byte and its data; decompressWSIPlane, wsicompress.go:487-524).  Nothing here calls
the code under test: the expected crops are cut out of the source arrays with numpy."""
import numpy as np

W70, H33 = 70, 33


def noise(synth, h, w, seed):
    return (synth.hash_u64(h * w * 3, seed) & np.uint64(0xFF)).astype(np.uint8).reshape(h, w, 3)


def modes(blob):
    """the three plane modes of a CompressRGB blob, from its length fields"""
    ls = [int.from_bytes(blob[4 * q: 4 * q + 4], "little") for q in range(3)]
    return [blob[12 + sum(ls[:p])] for p in range(3)]


def planes(img):
    """YCoCgRForward (asm_amd64.go:88-104) and ZigZag of Co and Cg (deltazigzagcompressu16.go:108-111): three (h, w) uint16 planes"""
    r, g, b = (img[..., k].astype(np.int32) for k in range(3))
    co = r - b
    t = b + (co >> 1)
    cg = g - t
    y = t + (cg >> 1)
    zz = lambda v: (((v << 1) ^ (v >> 15)) & 0xFFFF).astype(np.uint16)
    return y.astype(np.uint16), zz(co), zz(cg)


def assemble(bodies):
    """a CompressRGB blob from its three planes' bytes (mode byte included)"""
    return b"".join(len(b).to_bytes(4, "little") for b in bodies) + b"".join(bodies)


def raw_blob(img):
    """three raw planes: modes [3, 3, 3]"""
    return assemble([b"\x03" + p.astype("<u2").tobytes() for p in planes(img)])


def mixed_blob(mico, img):
    """Y raw, Co and Cg coded: modes [3, 2, 2] -- the coded streams lie behind 2 * w * h raw bytes"""
    y, co, cg = planes(img)
    bodies = [b"\x03" + y.astype("<u2").tobytes()]
    for p in (co, cg):
        rc, stream = mico.compress_single_frame(p, max(int(p.max()), 255), 2)
        assert rc == 0
        bodies.append(b"\x02" + stream)
    return assemble(bodies)


def build(synth, mico):
    """[(image (h, w, 3) uint8, file as mic.rgb_files takes it, plane modes)]"""
    ramp = np.repeat((np.arange(300) % 256).astype(np.uint8)[None, :, None], 3, axis=2)
    imgs = [np.zeros((1, 1, 3), np.uint8),                                     # 0, 0, 0
            np.array([[[200, 150, 100]]], np.uint8),                           # 1, 1, 0
            np.tile(np.array([200, 150, 100], np.uint8), (9, 9, 1)),           # 1, 1, 0
            np.array([[[10, 200, 30], [11, 100, 50]]], np.uint8),              # three raw planes of 2 x 1
            ramp,                                                              # raw Y of 300 x 1, Co and Cg constant zero
            noise(synth, 64, 64, 1), noise(synth, 17, 130, 2),                 # three coded planes
            synth.wsi_like(200, 300), synth.us_like(240, 320, 1), synth.us_like(240, 320, 2)]
    micr = (5, 8)                                                              # these two as MICR files
    out = []
    for i, im in enumerate(imgs):
        rc, blob = mico.wsi_compress_tile(im)
        assert rc == 0, i
        if i in micr:
            rc, f = mico.micr_write(im)
            assert rc == 0 and f[12:] == blob
            out.append((im, f, modes(blob)))
        else:
            out.append((im, (blob, im.shape[1], im.shape[0]), modes(blob)))
    hand = noise(synth, H33, W70, 3)                                          # (every plane of it codes under the reference's normaliser)
    for blob in (raw_blob(hand), mixed_blob(mico, hand)):
        out.append((hand, (blob, W70, H33), modes(blob)))
    return out


WANT_MODES = [[0, 0, 0], [1, 1, 0], [1, 1, 0], [3, 3, 3], [3, 0, 0], [2, 2, 2], [2, 2, 2], [2, 2, 2], None, [2, 0, 0], [3, 3, 3], [3, 2, 2]]

SHAPES = [(1, 1), (17, 5), (63, 9), (64, 7), (65, 6), (130, 11)]              # piece_lanes' seams: lw a power of two <= 64, then the x loop


def origins(files, cw, ch, skip=()):
    """(x, y, file) triples over every file but `skip`: inside at even and odd columns, negative, overhanging and wholly outside
    origins, several crops of one file"""
    xyf = []
    for f, (im, _, _) in enumerate(files):
        if f in skip:
            continue
        h, w = im.shape[:2]
        xyf += [(0, 0, f), (-3, -2, f), (1, 0, f), (w - cw // 2 - 1, h - ch // 2 - 1, f), (w, 0, f), (-cw, 0, f), (0, h, f), (-2, -1, f), (-1, 0, f)]
        if w > 40:
            xyf += [(33, min(10, h - 1), f), (34, min(11, h - 1), f), (w - 2, 0, f)]
    return xyf


def overlap(im, x, y, cw, ch):
    """the clipped columns and rows of a crop in its image, or None when they are empty"""
    h, w = im.shape[:2]
    x0, x1, y0, y1 = max(x, 0), min(x + cw, w), max(y, 0), min(y + ch, h)
    return (x0, x1, y0, y1) if x1 > x0 and y1 > y0 else None


def expected(files, xyf, cw, ch):
    """(n, ch, cw, 3) uint8: the crops of the source arrays, zero outside"""
    out = np.zeros((len(xyf), ch, cw, 3), np.uint8)
    for i, (x, y, f) in enumerate(xyf):
        o = overlap(files[f][0], x, y, cw, ch)
        if o:
            x0, x1, y0, y1 = o
            out[i, y0 - y: y1 - y, x0 - x: x1 - x] = files[f][0][y0:y1, x0:x1]
    return out


def brute_plan(files, xyf, cw, ch):
    """(files some crop overlaps with non-empty area, ascending; their mode-2 planes; the crops that overlap)"""
    named = sorted({f for x, y, f in xyf if overlap(files[f][0], x, y, cw, ch)})
    pieces = sum(1 for x, y, f in xyf if overlap(files[f][0], x, y, cw, ch))
    return named, sum(files[f][2].count(2) for f in named), pieces
