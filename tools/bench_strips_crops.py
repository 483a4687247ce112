#!/usr/bin/env python3
"""Times a 2-D training sampler's read of a strip-file dataset: 512 random 512 x 512 crops over 288 XR-shaped 12-bit PICS-8 files
(bench.py's generator and shape), three ways:
  (a) whole_images : decompress_parallel_strips_batch of the files the crops name into buffers kept across runs, numpy crops, one
                     upload per crop (all there was before the crop calls);
  (b) read_crops   : one strips_read_crops call from the files in host memory into a device tensor;
  (c) session      : one Session.strips_read_crops call with the files in device memory.
All three must give the same bytes.  Minimum and median of --runs runs after a warm-up, the device idle at the end of each run;
per-kernel device times of (c) through Session.set_timing.  Writes profiles/strips_crops.json (--out)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry


def timed(fn, runs, sync):
    fn(); sync()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(min_ms=round(min(ts), 3), median_ms=round(statistics.median(ts), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=288)
    ap.add_argument("--cols", type=int, default=2577)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--strips", type=int, default=8)
    ap.add_argument("--crops", type=int, default=512)
    ap.add_argument("--crop", type=int, nargs=2, default=[512, 512], metavar=("CW", "CH"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strips_crops.json"))
    a = ap.parse_args()
    import torch
    mic = entry.load_package()
    synth = importlib.import_module("medical_image_codec_amd.synth")
    n, w, h = a.images, a.cols, a.rows
    cw, ch = a.crop
    d_px = synth.xr_like_batch_torch(n, cols=w, rows=h, depth=12, seed0=1, noise=synth.XR_NOISE_PUBLISHED_RATIO, device="cuda")
    images = d_px.cpu().numpy().view(np.uint16)
    del d_px
    files = []
    for i0 in range(0, n, 48):                                                # (the encoder's out buffers are sized for the worst case)
        for st, f in mic.compress_parallel_strips_batch(list(images[i0: i0 + 48]), 4095, a.strips, 2):
            assert st == 0, st
            files.append(f.copy())
    rng = np.random.default_rng(7)
    xyf = np.stack([rng.integers(0, w - cw + 1, a.crops), rng.integers(0, h - ch + 1, a.crops), rng.integers(0, n, a.crops)], axis=1)
    units, pieces, _ = mic.strips_crop_plan(files, xyf, cw, ch)
    named = sorted({int(f) for f in xyf[:, 2]})
    place = {f: k for k, f in enumerate(named)}
    sync = torch.cuda.synchronize
    keep = {}
    outs = [np.empty(w * h, dtype=np.uint16) for _ in named]

    def whole_images():
        res = mic.decompress_parallel_strips_batch([files[f] for f in named], [(w, h)] * len(named), outs)
        keep["a"] = [torch.from_numpy(np.ascontiguousarray(res[place[int(f)]][1][y: y + ch, x: x + cw]).view(np.int16)).cuda() for x, y, f in xyf]
    t = torch.empty((a.crops, ch, cw), dtype=torch.int16, device="cuda")
    nbytes = t.numel() * 2

    def read_crops():
        keep["st"], keep["bad"], keep["stats"] = mic.strips_read_crops(files, xyf, cw, ch, t.data_ptr(), nbytes)
    sess = mic.Session(8, w * (h // a.strips + 1))
    lens = [f.size for f in files]
    offs = np.concatenate([[0], np.cumsum([(ln + 255) // 256 * 256 for ln in lens])])
    d_all = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda")
    for f, o in zip(files, offs):
        d_all[int(o): int(o) + f.size] = torch.from_numpy(f).cuda()
    ptrs = [d_all.data_ptr() + int(o) for o in offs[:-1]]
    heads = [mic.strips_head(f) for f in files]
    t2 = torch.empty_like(t)

    def session():
        keep["st2"], keep["bad2"], keep["stats2"] = sess.strips_read_crops(heads, ptrs, lens, xyf, cw, ch, t2.data_ptr(), nbytes)
    r = dict(device=mic.device_name(), images=n, shape=[h, w], strips=a.strips, crops=a.crops, crop=[ch, cw], runs=a.runs,
             file_bytes=int(sum(lens)), files_named=len(named))
    r["whole_images"] = timed(whole_images, a.runs, sync)
    r["read_crops"] = timed(read_crops, a.runs, sync)
    r["session"] = timed(session, a.runs, sync)
    want = torch.stack(keep["a"])
    assert torch.equal(want, t) and torch.equal(want, t2), "the three ways disagree"
    assert (keep["st"] == 0).all() and (keep["st2"] == 0).all() and keep["stats"] == keep["stats2"]
    stats = keep["stats"]
    assert stats["strips_decoded"] == len(units) and stats["pieces"] == pieces
    r.update(strips_decoded=int(stats["strips_decoded"]), strips_total=int(stats["strips_total"]), pieces=int(pieces), slabs=int(stats["slabs"]),
             strips_decoded_share=round(stats["strips_decoded"] / stats["strips_total"], 4),
             bytes_uploaded=int(sum(int.from_bytes(bytes(files[f][24 + 8 * k: 28 + 8 * k]), "little") for f, k in units.tolist())))
    for k in ("read_crops", "session"):
        r[k]["speedup_min"] = round(r["whole_images"]["min_ms"] / r[k]["min_ms"], 2)
        r[k]["speedup_median"] = round(r["whole_images"]["median_ms"] / r[k]["median_ms"], 2)
    sess.set_timing(2)
    session(); sync()
    r["session_kernels_ms"] = {k: round(v, 3) for k, v in sess.last_timings()}
    sess.set_timing(0)
    sess.close()
    print(json.dumps(r))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(r, indent=1) + "\n")


if __name__ == "__main__":
    main()
