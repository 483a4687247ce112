"""MIC3 and WaveletV2 from host buffers over a device list (mic_hip_set_devices): mic_hip_wsi_compress_ex and
mic_hip_wsi_decompress_level(0) on a synthetic RGB slide (synth.wsi_slide, 32768 x 32768 by default), and a WaveletV2 batch
(256 frames of 512 x 512 by default) through mic_hip_wavelet_v2_compress_batch / _decompress_batch.  Wall time per call, median of
--reps after one warm-up call; prints one JSON line.  The file's SHA-256 lets runs with different lists be compared.

    python tools/bench_wsi_devices.py --devices 0
    python tools/bench_wsi_devices.py --devices 0,0

A device may be listed twice (two shards on one GPU): that shows the band path runs and what overlap two shards get on one GPU, not
what N GPUs would give."""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

mic = entry.load_package()
synth = importlib.import_module("medical_image_codec_amd.synth")


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--devices", default="0", help="comma-separated device list for mic_hip_set_devices")
    ap.add_argument("--size", type=int, default=32768, help="slide width = height")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--frame-size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    devs = [int(d) for d in a.devices.split(",")]
    mic.set_devices(devs)
    L = mic.lib()
    res = dict(devices=devs, wsi_size=a.size, reps=a.reps)

    S = a.size
    slide = synth.wsi_slide(S, S)
    px = slide.reshape(-1)
    cap = px.size * 3 + (1 << 20)                      # (np.empty: only the pages the file is written to are touched)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0)

    def compress():
        rc = L.mic_hip_wsi_compress_ex(px.ctypes.data, S, S, 3, 8, 256, 256, 0, out.ctypes.data, cap, C.byref(n))
        assert rc == 0, rc
    res["wsi_compress_ms"], res["wsi_compress_all_ms"] = timed(compress, a.reps)
    blob = out[: n.value]
    res["wsi_bytes"] = int(n.value)
    res["wsi_sha256"] = hashlib.sha256(memoryview(blob)).hexdigest()[:16]
    img = np.empty_like(px)

    def decompress():
        rc = L.mic_hip_wsi_decompress_level(blob.ctypes.data, blob.size, 0, img.ctypes.data, img.size)
        assert rc == 0, rc
    res["wsi_decompress_level0_ms"], res["wsi_decompress_level0_all_ms"] = timed(decompress, a.reps)
    res["wsi_round_trip_ok"] = bool(np.array_equal(img, px))
    del slide, px, out, img, blob

    F, R = a.frames, a.frame_size
    base = [synth.xr_like(cols=R, rows=R, depth=12, seed=40 + i) for i in range(8)]
    frames = np.stack([np.roll(base[i % 8], i // 8, axis=1) for i in range(F)])
    files = []

    def wv_compress():
        got = mic.wavelet_v2_compress_batch(frames, 4095, 5)
        assert all(st == 0 for st, _ in got)
        files[:] = [b for _, b in got]
    res["wavelet_frames"], res["wavelet_frame_size"] = F, R
    res["wavelet_compress_ms"], res["wavelet_compress_all_ms"] = timed(wv_compress, a.reps)
    res["wavelet_bytes"] = sum(len(b) for b in files)
    back = []

    def wv_decompress():
        st, pxs = mic.wavelet_v2_decompress_batch(files)
        assert st == [0] * F
        back[:] = [pxs]
    res["wavelet_decompress_ms"], res["wavelet_decompress_all_ms"] = timed(wv_decompress, a.reps)
    res["wavelet_round_trip_ok"] = bool(np.array_equal(back[0], frames))
    mic.set_devices([0])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
