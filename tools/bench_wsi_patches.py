#!/usr/bin/env python3
"""512 random 256 x 256 patches of level 0 of an 8192 x 8192 RGB slide (256 x 256 tiles), three ways:
  file    -- one mic_hip_wsi_read_patches call on the MIC3 file in host memory, into a device tensor
  store   -- one Session.wsi_read_patches call on the slide Session.wsi_encode left on the device
  loop    -- what there was before: decompress_wsi_region + torch.from_numpy(...).cuda() per patch
Ten runs each (after one warm-up), min and median wall time, the calls' stats; the record goes to profiles/wsi_patches.json.

  python tools/bench_wsi_patches.py [--size 8192] [--patches 512] [--patch 256] [--runs 10] [--out profiles/wsi_patches.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def timed(fn, runs, sync):
    fn(); sync()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn(); sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(min_ms=min(ts), median_ms=statistics.median(ts), runs_ms=ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--patches", type=int, default=512)
    ap.add_argument("--patch", type=int, default=256)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wsi_patches.json"))
    a = ap.parse_args()
    import torch
    import importlib
    mic = entry.load_package()
    synth = importlib.import_module("medical_image_codec_amd.synth")
    W = H = a.size
    n, p = a.patches, a.patch
    img = np.ascontiguousarray(synth.wsi_like(W, H, seed=11))
    data = mic.compress_wsi(img, W, H)
    rng = np.random.default_rng(1)
    xy = np.stack([rng.integers(0, W - p, n), rng.integers(0, H - p, n)], 1).astype(np.int32)
    out = torch.empty((n, p, p, 3), dtype=torch.uint8, device="cuda")
    sync = torch.cuda.synchronize
    rec = dict(device=mic.device_name(), slide=[W, H], tile=256, patches=n, patch=[p, p], file_bytes=len(data), runs=a.runs)

    stats = {}
    def by_file():
        st, stats["file"] = mic.wsi_read_patches(data, 0, xy, p, p, out.data_ptr(), out.numel())
        assert (st == 0).all()
    rec["file"] = timed(by_file, a.runs, sync)
    ref = out.cpu().numpy().copy()
    for i in (0, n // 2, n - 1):
        assert np.array_equal(ref[i], img[xy[i, 1]: xy[i, 1] + p, xy[i, 0]: xy[i, 0] + p])

    sess = mic.Session(3 * 1024, 256 * 256)
    d_img = torch.from_numpy(img.reshape(-1)).cuda()
    sess.wsi_encode(d_img.data_ptr(), W, H)
    def by_store():
        st, stats["store"] = sess.wsi_read_patches(0, xy, p, p, out.data_ptr(), out.numel())
        assert (st == 0).all()
    rec["store"] = timed(by_store, a.runs, sync)
    assert np.array_equal(out.cpu().numpy(), ref)
    sess.close()

    def by_loop():
        for i in range(n):
            out[i] = torch.from_numpy(mic.decompress_wsi_region(data, 0, int(xy[i, 0]), int(xy[i, 1]), p, p)).cuda()
    rec["loop"] = timed(by_loop, a.runs, sync)
    assert np.array_equal(out.cpu().numpy(), ref)

    rec["stats"] = stats
    rec["loop_over_file_median"] = rec["loop"]["median_ms"] / rec["file"]["median_ms"]
    rec["loop_over_store_median"] = rec["loop"]["median_ms"] / rec["store"]["median_ms"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: (v if not isinstance(v, dict) or "runs_ms" not in v else {"min_ms": round(v["min_ms"], 2), "median_ms": round(v["median_ms"], 2)})
                      for k, v in rec.items()}))


if __name__ == "__main__":
    main()
