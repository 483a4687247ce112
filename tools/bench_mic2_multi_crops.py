#!/usr/bin/env python3
"""Times a 3-D training step's read of a batch of crops, each from another MIC2 volume of a dataset: --volumes volumes of --frames
frames of 512 x 512 at 12 bits (rolled XR-like images, a seed per volume), coded independent and temporal, and two batches of
128 x 128 x 64 crops -- one crop from each of 16 volumes, and 8 crops from 4 volumes -- three ways:
  (a) loop    : mic2_read_crops, one call per volume (the code as it was: the yardstick);
  (b) multi   : one mic2_multi_read_crops from the files in host memory;
  (c) session : one Session.mic2_multi_read_crops with the files in device memory.
All three must give the same bytes.  Also one volume with 64 crops through the old door and through the new one.  Minimum and
median of --runs runs after a warm-up, the device idle at the end of each run; per-kernel device times of (c) through
Session.set_timing.  Writes profiles/mic2_multi_crops.json (--out)."""
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
    return dict(min_ms=round(min(ts), 3), median_ms=round(statistics.median(ts), 3), max_ms=round(max(ts), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=16)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--crop", type=int, nargs=3, default=[128, 128, 64], metavar=("CW", "CH", "CD"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mic2_multi_crops.json"))
    a = ap.parse_args()
    import torch
    mic = entry.load_package()
    synth = importlib.import_module("medical_image_codec_amd.synth")
    nv, n, w, h = a.volumes, a.frames, a.size, a.size
    cw, ch, cd = a.crop
    sync = torch.cuda.synchronize
    files = {False: [], True: []}
    for v in range(nv):
        img = synth.xr_like(cols=w, rows=h, depth=12, seed=100 + v)
        vol = np.stack([np.roll(img, 3 * k, axis=1) for k in range(n)])
        for temporal in (False, True):
            files[temporal].append(mic.compress_multi_frame(vol, w, h, 4095, temporal=temporal))
    rng = np.random.default_rng(7)

    def origins(count):
        return np.stack([rng.integers(0, w - cw + 1, count), rng.integers(0, h - ch + 1, count), rng.integers(0, n - cd + 1, count)], axis=1)
    # the crops of a batch sorted by volume: the loop writes each volume's crops into its own stretch of the tensor
    batches = {"16_crops_16_volumes": np.column_stack([origins(nv), np.arange(nv)]),
               "8_crops_4_volumes": np.column_stack([origins(8), np.repeat(np.arange(4) * (nv // 4), 2)]),
               "64_crops_1_volume": np.column_stack([origins(64), np.zeros(64, dtype=np.int64)])}
    result = dict(device=mic.device_name(), volumes=nv, volume=[n, h, w], crop=[cw, ch, cd], runs=a.runs, files={})
    kinds = {"independent": files[False], "temporal": files[True],
             "mixed": [files[bool(v & 1)][v] for v in range(nv)]}
    for kind, fl in kinds.items():
        heads = [f[: 20 + 8 * n] for f in fl]
        d_files = [torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy()).cuda() for f in fl]
        ptrs, lens = [d.data_ptr() for d in d_files], [len(f) for f in fl]
        result["files"][kind] = dict(file_bytes=int(sum(lens)))
        for name, xyzv in batches.items():
            nc = len(xyzv)
            t = [torch.empty((nc, cd, ch, cw), dtype=torch.int16, device="cuda") for _ in range(3)]
            nbytes = t[0].numel() * 2
            per_crop = cd * ch * cw * 2
            runs_of = [(int(v), np.flatnonzero(xyzv[:, 3] == v)) for v in np.unique(xyzv[:, 3])]
            keep = {}

            def loop():
                keep["a"] = [mic.mic2_read_crops(fl[v], xyzv[idx, :3], cw, ch, cd, t[0].data_ptr() + int(idx[0]) * per_crop, len(idx) * per_crop)
                             for v, idx in runs_of]

            def multi():
                keep["b"] = mic.mic2_multi_read_crops(fl, xyzv, cw, ch, cd, t[1].data_ptr(), nbytes)
            sess = mic.Session(8, w * h)

            def session():
                keep["c"] = sess.mic2_multi_read_crops(heads, ptrs, lens, xyzv, cw, ch, cd, t[2].data_ptr(), nbytes)
            units, pieces, _ = mic.mic2_multi_crop_plan(fl, xyzv, cw, ch, cd)
            r = dict(crops=nc, volumes_named=len(runs_of), frames_decoded=int(len(units)), pieces=int(pieces))
            r["loop"] = timed(loop, a.runs, sync)
            r["multi"] = timed(multi, a.runs, sync)
            r["session"] = timed(session, a.runs, sync)
            assert torch.equal(t[0], t[1]) and torch.equal(t[0], t[2]), "the three ways disagree"
            assert all((st == 0).all() for st, _ in keep["a"]) and (keep["b"][0] == 0).all() and (keep["c"][0] == 0).all()
            assert keep["b"][2] == keep["c"][2] and keep["b"][2]["frames_decoded"] == len(units)
            r["loop_slabs"] = int(sum(s["slabs"] for _, s in keep["a"]))
            r["multi_slabs"] = int(keep["b"][2]["slabs"])
            r["loop_over_multi_min"] = round(r["loop"]["min_ms"] / r["multi"]["min_ms"], 2)
            sess.set_timing(2)
            session(); sync()
            r["session_kernels_ms"] = {k: round(v, 3) for k, v in sess.last_timings()}
            sess.set_timing(0)
            sess.close()
            result["files"][kind][name] = r
            print(kind, name, json.dumps({k: r[k] for k in ("loop", "multi", "session", "loop_slabs", "multi_slabs")}), flush=True)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
