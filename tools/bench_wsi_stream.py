"""MIC3 streaming against the one-shot call on a synthetic RGB slide (synth.wsi_slide, 32768 x 32768 by default).

One-shot: mic_hip_wsi_compress_ex on the whole slide in one host buffer.  Streaming: WsiWriter with pushes of 512, 2048 and 8192
rows into an in-memory sink; each push's rows come from synth.wsi_slide_band, so the streamed slide is never whole in host memory,
and the band generation is kept out of the streaming time.  For each: wall ms (median of --reps after one warm-up), device_bytes,
peak host bytes the writer held, bands, the band pyramid kernel's device time per band (k_wsi_band_pyramid), and the existing
per-level launches (k_wsi_downsample, one per level) on a device-resident band of the same rows (mic_hip_session_wsi_encode with
timing).  Every streamed file is checked against the one-shot file.  Prints one JSON line.

    python tools/bench_wsi_stream.py [--size 32768] [--reps 3]"""
import argparse
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


class MemSink:
    """in-memory pwrite target, grown as offsets arrive"""
    def __init__(self):
        self.buf = bytearray()

    def __call__(self, off, data):
        end = off + len(data)
        if len(self.buf) < end:
            self.buf.extend(bytes(end - len(self.buf)))
        self.buf[off:end] = data


def stream_once(size, push, seed):
    sink = MemSink()
    t_push = 0.0
    with mic.WsiWriter(sink, size, size) as w:
        for y in range(0, size, push):
            band = synth.wsi_slide_band(size, size, y, min(size, y + push), seed)
            t0 = time.perf_counter()
            w.push(band)
            t_push += time.perf_counter() - t0
        t0 = time.perf_counter()
        n = w.finish()
        t_push += time.perf_counter() - t0
        st = w.stats
        dev = w.device_bytes
    return t_push * 1e3, bytes(sink.buf[:n]), dev, st


def band_downsample_ms(size, rows, seed):
    """k_wsi_downsample over every level of one band of `rows` rows, resident on the device (the one-shot path's launches)"""
    import torch
    band = synth.wsi_slide_band(size, size, 0, rows, seed)
    d = torch.from_numpy(band.reshape(-1)).cuda()
    sess = mic.Session(1, 256 * 256)
    sess.wsi_encode(d.data_ptr(), size, rows)                      # (warm)
    sess.set_timing(2)                                             # (summed over the call's launch chains)
    sess.wsi_encode(d.data_ptr(), size, rows)
    ms = [t for name, t in sess.last_timings() if name == "k_wsi_downsample"]
    sess.close()
    return ms[0] if ms else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pushes", default="512,2048,8192")
    a = ap.parse_args()
    seed = 4
    size = a.size
    img = synth.wsi_slide(size, size, seed=seed)
    px = img.reshape(-1)
    out = np.empty(px.size + (1 << 26), dtype=np.uint8)
    import ctypes as C
    n = C.c_size_t(0)

    def oneshot():
        rc = mic.lib().mic_hip_wsi_compress_ex(px.ctypes.data, size, size, 3, 8, 0, 0, 0, out.ctypes.data, out.size, C.byref(n))
        assert rc == 0, rc
    oneshot()
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        oneshot()
        ts.append((time.perf_counter() - t0) * 1e3)
    want = out[: n.value].tobytes()
    res = dict(size=size, file_bytes=len(want), sha256=hashlib.sha256(want).hexdigest()[:16],
               oneshot_ms=round(statistics.median(ts), 1), oneshot_host_bytes=px.size + len(want), stream={})
    del img, px
    for push in (int(p) for p in a.pushes.split(",")):
        stream_once(size, push, seed)                              # warm-up
        runs = [stream_once(size, push, seed) for _ in range(a.reps)]
        ms = statistics.median(r[0] for r in runs)
        _, got, dev, st = runs[0]
        res["stream"][str(push)] = dict(ms=round(ms, 1), ratio=round(ms / res["oneshot_ms"], 3), equal=got == want, device_bytes=dev,
                                        host_bytes_peak=st["host_bytes_peak"], bands=st["bands"], band_rows=st["band_rows"],
                                        pyramid_ms_per_band=round(st["pyramid_ms"] / max(1, st["bands"]), 4))
    # the band the writer codes: R rows (its device_bytes do not depend on the push size)
    rows = next(iter(res["stream"].values()))["band_rows"]
    res["band_downsample_ms_existing"] = band_downsample_ms(size, rows, seed)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
