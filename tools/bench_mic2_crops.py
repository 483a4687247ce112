#!/usr/bin/env python3
"""Times a 3-D training sampler's read of a MIC2 volume: 64 random 128 x 128 x 64 crops of a 256-frame 512 x 512 12-bit stack, from
an independent and from a temporal file, three ways:
  (a) whole_stack : decompress_multi_frame to the host, numpy crops, one upload per crop (all there was before the crop calls);
  (b) read_crops  : mic2_read_crops from the file in host memory into a device tensor;
  (c) session     : Session.mic2_read_crops with the file in device memory.
All three must give the same bytes.  Minimum and median of --runs runs after a warm-up, the device idle at the end of each run;
per-kernel device times of (c) through Session.set_timing.  Writes profiles/mic2_crops.json (--out)."""
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
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--crops", type=int, default=64)
    ap.add_argument("--crop", type=int, nargs=3, default=[128, 128, 64], metavar=("CW", "CH", "CD"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mic2_crops.json"))
    a = ap.parse_args()
    import torch
    mic = entry.load_package()
    synth = importlib.import_module("medical_image_codec_amd.synth")
    n, w, h = a.frames, a.size, a.size
    cw, ch, cd = a.crop
    img = synth.xr_like(cols=w, rows=h, depth=12, seed=3)
    vol = np.stack([np.roll(img, 3 * k, axis=1) for k in range(n)])
    rng = np.random.default_rng(7)
    xyz = np.stack([rng.integers(0, w - cw + 1, a.crops), rng.integers(0, h - ch + 1, a.crops), rng.integers(0, n - cd + 1, a.crops)], axis=1)
    sync = torch.cuda.synchronize
    result = dict(device=mic.device_name(), volume=[n, h, w], crops=a.crops, crop=[cw, ch, cd], runs=a.runs, files={})
    for temporal in (False, True):
        data = mic.compress_multi_frame(vol, w, h, 4095, temporal=temporal)
        frames, pieces = mic.mic2_crop_plan(w, h, n, temporal, xyz, cw, ch, cd)
        keep = {}

        def whole_stack():
            stack = mic.decompress_multi_frame(data)
            keep["a"] = [torch.from_numpy(np.ascontiguousarray(stack[z: z + cd, y: y + ch, x: x + cw]).view(np.int16)).cuda() for x, y, z in xyz]
        t = torch.empty((a.crops, cd, ch, cw), dtype=torch.int16, device="cuda")
        nbytes = t.numel() * 2

        def read_crops():
            keep["st"], keep["stats"] = mic.mic2_read_crops(data, xyz, cw, ch, cd, t.data_ptr(), nbytes)
        sess = mic.Session(8, w * h)
        d_file = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
        head = data[: 20 + 8 * n]
        t2 = torch.empty_like(t)

        def session():
            keep["st2"], keep["stats2"] = sess.mic2_read_crops(head, d_file.data_ptr(), len(data), xyz, cw, ch, cd, t2.data_ptr(), nbytes)
        r = dict(file_bytes=len(data), frames_decoded=int(frames.size), pieces=int(pieces))
        r["whole_stack"] = timed(whole_stack, a.runs, sync)
        r["read_crops"] = timed(read_crops, a.runs, sync)
        r["session"] = timed(session, a.runs, sync)
        want = torch.stack(keep["a"])
        assert torch.equal(want, t) and torch.equal(want, t2), "the three ways disagree"
        assert (keep["st"] == 0).all() and (keep["st2"] == 0).all() and keep["stats"] == keep["stats2"]
        r["slabs"] = int(keep["stats"]["slabs"])
        sess.set_timing(2)
        session(); sync()
        r["session_kernels_ms"] = {k: round(v, 3) for k, v in sess.last_timings()}
        sess.set_timing(0)
        sess.close()
        result["files"]["temporal" if temporal else "independent"] = r
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
