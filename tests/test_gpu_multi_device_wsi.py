"""MIC3 slides and WaveletV2 batches over the devices of mic_hip_set_devices (csrc/mic_api_ext.hip: wsi_compress_bands, decode_box;
csrc/mic_host_io.hip: over_devices).  A slide is cut into one band of tile rows per device (mic_hip_wsi_band_plan); each band codes
levels 0..K as a slide of its own, devices[0] codes the top of the pyramid from the bands' gathered rows.  The file must be the
one-device file byte for byte, whatever the list.  The test box has one GPU, so the lists are {0}, {0, 0} and {0, 0, 0}: the same
code path with two and three shards on one device.  Reference fan-out: wsicompress.go:126-145."""
import ctypes as C
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LISTS = ([0], [0, 0], [0, 0, 0])

# (format, width, height, tile_w, tile_h, levels); the plan of each over 2 and 3 shards is checked below to cover K = L - 1 (no
# top of the pyramid to gather), 0 < K < L - 1, K = 0 (with an even and with an odd tile_h), an odd tile_h with K > 0, empty bands
CASES = [
    ("rgb", 2050, 1999, 256, 256, 0),
    ("rgb", 1201, 777, 128, 96, 0),
    ("rgb", 999, 1500, 160, 97, 0),
    ("rgb", 700, 300, 256, 256, 0),
    ("rgb", 3001, 600, 256, 255, 0),
    ("rgb", 1501, 1203, 256, 256, 2),
    ("grey8", 1537, 2305, 256, 256, 3),
    ("grey8", 640, 2600, 200, 100, 2),
    ("grey16", 777, 1999, 100, 100, 4),
    ("grey16", 901, 1203, 256, 256, 0),
]


@pytest.fixture
def device_lists(mic, gpu_ready):
    yield LISTS
    mic.set_devices([0])


def _slide(synth, fmt, w, h, seed):
    if fmt == "rgb":                                  # (grain: small tiles of smooth slides are what the reference's normaliser gives up on)
        grain = np.random.default_rng(seed).integers(-6, 7, (h, w, 3))
        return np.clip(synth.wsi_like(w, h, seed=seed).astype(np.int32) + grain, 0, 255).astype(np.uint8)
    from test_oracle_wavelet_wsi import _grey_slide
    return _grey_slide(synth, w, h, 16 if fmt == "grey16" else 8, seed=seed)


def _oracle(mico, fmt, img, tw, th, levels):
    return mico.wsi_compress(img, tw, th, levels) if fmt == "rgb" else mico.wsi_compress_grey(img, tw, th, levels)


def _compress(mic, fmt, img, w, h, tw, th, levels):
    if fmt == "rgb":
        return mic.compress_wsi(img, w, h, tile_w=tw, tile_h=th, levels=levels)
    return mic.compress_wsi(img, w, h, channels=1, bits_per_sample=16 if fmt == "grey16" else 8, tile_w=tw, tile_h=th, levels=levels)


def test_cases_cover_every_kind_of_plan(mic):
    par = importlib.import_module("medical_image_codec_amd.parallel")
    kinds = set()
    for fmt, w, h, tw, th, lv in CASES:
        L = len(par.wsi_levels(w, h, tw, th, lv))
        for shards in (2, 3):
            k, first = mic.wsi_band_plan(w, h, tw, th, lv, shards)
            bands = sum(b > a for a, b in zip(first, first[1:]))
            if bands < 2:
                continue
            kinds.add("K=L-1" if k == L - 1 else ("K=0" if k == 0 else "0<K<L-1"))
            if k == 0 and k < L - 1:
                kinds.add("K=0 odd tile_h" if th & 1 else "K=0 even tile_h")
            if th & 1 and 0 < k < L - 1:
                kinds.add("odd tile_h gathers level K")
            if bands < shards:
                kinds.add("empty band")
            if fmt != "rgb":
                kinds.add(fmt)
    assert kinds >= {"K=L-1", "0<K<L-1", "K=0", "K=0 odd tile_h", "K=0 even tile_h", "odd tile_h gathers level K", "empty band",
                     "grey8", "grey16"}, kinds


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-t{c[3]}x{c[4]}-l{c[5]}" for c in CASES])
def test_slide_files_and_decodes_equal_one_device(mic, mico, synth, device_lists, case):
    fmt, w, h, tw, th, levels = case
    img = _slide(synth, fmt, w, h, seed=w % 13 + 3)
    rc, want = _oracle(mico, fmt, img, tw, th, levels)
    assert rc == 0
    ref_levels = None
    for devs in device_lists:
        mic.set_devices(devs)
        got = _compress(mic, fmt, img, w, h, tw, th, levels)
        assert got == want, devs
        hdr = mic.read_wsi_header(want)
        pix = [mic.decompress_wsi_level(want, lvl).copy() for lvl in range(len(hdr["levels"]))]
        assert np.array_equal(pix[0], img), devs
        if ref_levels is None:
            ref_levels = pix
        for lvl, (a, b) in enumerate(zip(pix, ref_levels)):
            assert np.array_equal(a, b), (devs, lvl)
        # rectangles across tile-row (and so shard) edges, at levels 0 and 1
        for lvl in range(min(2, len(pix))):
            lh, lw = pix[lvl].shape[:2]
            for f in (1 / 3, 1 / 2, 2 / 3):
                y = max(0, int(round(lh * f / th)) * th - 5)
                for x, rw in ((3, lw - 7), (lw // 3, 50)):
                    rh = 2 * th + 10
                    if x >= lw or y >= lh or rw <= 0:
                        continue
                    reg = mic.decompress_wsi_region(want, lvl, x, y, rw, rh)
                    assert np.array_equal(reg, pix[lvl][y: y + rh, x: x + rw]), (devs, lvl, x, y)
            assert np.array_equal(mic.decompress_wsi_region(want, lvl, 0, 0, lw, lh), pix[lvl]), (devs, lvl)


def test_capacity_error_leaves_the_guard_bytes(mic, mico, synth, device_lists):
    w, h = 1201, 777
    img = _slide(synth, "rgb", w, h, seed=21)
    rc, want = mico.wsi_compress(img, 128, 96, 0)
    assert rc == 0
    hdr_len = 48 + 20 * int.from_bytes(want[28:30], "little") + 16 * int.from_bytes(want[32:40], "little")
    px = np.ascontiguousarray(img).reshape(-1)
    for devs in device_lists:
        mic.set_devices(devs)
        for cap in (10, hdr_len, hdr_len + 100, len(want) - 1, len(want)):
            buf = np.full(cap + 4096, 0xA5, dtype=np.uint8)
            n = C.c_size_t(0)
            rc = mic.lib().mic_hip_wsi_compress_ex(px.ctypes.data, w, h, 3, 8, 128, 96, 0, buf.ctypes.data, cap, C.byref(n))
            assert (buf[cap:] == 0xA5).all(), (devs, cap)
            if cap < len(want):
                assert rc == mic.MIC_ERR_CAPACITY, (devs, cap)
            else:
                assert rc == 0 and n.value == len(want) and buf[: n.value].tobytes() == want, devs


def _damage_tile(blob: bytes, level: int, tx: int, ty: int) -> bytes:
    b = bytearray(blob)
    nlev, total = int.from_bytes(b[28:30], "little"), int.from_bytes(b[32:40], "little")
    ld = 48 + 20 * level
    tiles_x, first = int.from_bytes(b[ld + 8: ld + 12], "little"), int.from_bytes(b[ld + 16: ld + 20], "little")
    e = 48 + 20 * nlev + 16 * (first + ty * tiles_x + tx)
    off = int.from_bytes(b[e: e + 8], "little")
    b[48 + 20 * nlev + 16 * total + off + 12] = 9                     # the first plane's mode byte: no such mode
    return bytes(b)


def test_damaged_tile_in_the_last_band_fails_like_one_device(mic, mico, synth, device_lists):
    w, h = 2050, 1999
    img = _slide(synth, "rgb", w, h, seed=22)
    rc, want = mico.wsi_compress(img, 256, 256, 0)
    assert rc == 0
    hdr = mic.read_wsi_header(want)
    bad = _damage_tile(want, 0, 1, hdr["levels"][0]["tiles_y"] - 1)
    codes = []
    for devs in device_lists:
        mic.set_devices(devs)
        with pytest.raises(mic.MicError) as e:
            mic.decompress_wsi_level(bad, 0)
        codes.append(e.value.code)
        assert np.array_equal(mic.decompress_wsi_level(bad, 1), mic.decompress_wsi_level(want, 1)), devs
    assert codes[0] == mic.MIC_ERR_CORRUPT and codes == [codes[0]] * len(codes), codes


def test_wavelet_v2_batches_over_device_lists(mic, mico, synth, device_lists):
    frames = np.stack([synth.xr_like(cols=96, rows=80, depth=12, seed=700 + i, noise=2.0 + i % 5) for i in range(24)])
    want = [mico.wavelet_v2_compress(f, 4095, 5) for f in frames]
    assert all(rc == 0 for rc, _ in want)
    rc, other = mico.wavelet_v2_compress(synth.xr_like(cols=100, rows=80, depth=12, seed=9, noise=4.0), 4095, 5)
    assert rc == 0
    for devs in device_lists:
        mic.set_devices(devs)
        got = mic.wavelet_v2_compress_batch(frames, 4095, 5)
        for i, ((st, blob), (_, ref)) in enumerate(zip(got, want)):
            assert st == 0 and blob == ref, (devs, i)
        st, px = mic.wavelet_v2_decompress_batch([b for _, b in want])
        assert st == [0] * len(frames) and np.array_equal(px, frames), devs
        # a file of another shape as the FIRST frame of the second shard: compared with the batch's files[0], it fails alone;
        # a damaged file on the last shard fails alone too
        first = mic.shard_plan([96 * 80] * len(frames), len(devs))
        pos = first[1] if len(devs) > 1 else len(frames) // 2
        files = [b for _, b in want]
        files[pos] = other
        files[-1] = files[-1][:11] + b"\x00" + files[-1][12:]
        st, px = mic.wavelet_v2_decompress_batch(files)
        for i in range(len(frames)):
            if i == pos:
                assert st[i] == mic.MIC_ERR_ARGS, (devs, i)
            elif i == len(frames) - 1:
                assert st[i] == mic.MIC_ERR_CORRUPT, (devs, i)
            else:
                assert st[i] == 0 and np.array_equal(px[i], frames[i]), (devs, i)
