#!/usr/bin/env python3
"""Patches of many slides per call against the loop of single-slide calls.
  mixed   -- 64 distinct 2048 x 2048 RGB slides (256 x 256 tiles; files in host memory), 8 random 256 x 256 patches of each, half
             of them at level 0 and half at level 1, into one device tensor:
               multi -- one mic_hip_wsi_multi_read_patches call
               loop  -- what there was before: one mic_hip_wsi_read_patches call per (slide, level) pair, into slices of the tensor
  single  -- the tools/bench_wsi_patches.py workload (512 random 256 x 256 patches of level 0 of one 8192 x 8192 slide) through the
             new call and through mic_hip_wsi_read_patches: what the self-describing pieces cost when nothing is mixed
Ten runs each (after one warm-up), min and median wall time, the calls' stats; the record goes to profiles/wsi_multi_patches.json.

  python tools/bench_wsi_multi_patches.py [--slides 64] [--size 2048] [--per-slide 8] [--patch 256] [--single-size 8192]
                                          [--single-patches 512] [--runs 10] [--out profiles/wsi_multi_patches.json]
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
    ap.add_argument("--slides", type=int, default=64)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--per-slide", type=int, default=8)
    ap.add_argument("--patch", type=int, default=256)
    ap.add_argument("--single-size", type=int, default=8192)
    ap.add_argument("--single-patches", type=int, default=512)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wsi_multi_patches.json"))
    a = ap.parse_args()
    import torch
    import importlib
    mic = entry.load_package()
    synth = importlib.import_module("medical_image_codec_amd.synth")
    sync = torch.cuda.synchronize
    p = a.patch
    rec = dict(device=mic.device_name(), runs=a.runs)
    stats = {}

    # ---- mixed: many slides, two levels
    W = H = a.size
    files, level1 = [], []
    for s in range(a.slides):
        img = np.ascontiguousarray(synth.wsi_like(W, H, seed=100 + s))
        files.append(mic.compress_wsi(img, W, H))
        if s in (0, a.slides - 1):
            level1.append((s, img, mic.decompress_wsi_level(files[-1], 1)))
    rng = np.random.default_rng(1)
    q = []
    for s in range(a.slides):
        for k in range(a.per_slide):
            level = k % 2                                                   # half at level 0, half at level 1
            lw, lh = W >> level, H >> level
            q.append((int(rng.integers(0, lw - p)), int(rng.integers(0, lh - p)), s, level))
    q = np.asarray([q[i] for i in rng.permutation(len(q))], dtype=np.int32)
    n = len(q)
    out = torch.empty((n, p, p, 3), dtype=torch.uint8, device="cuda")
    rec["mixed"] = dict(slides=a.slides, slide=[W, H], tile=256, levels_used=[0, 1], patches=n, patch=[p, p], file_bytes=sum(len(f) for f in files))

    def by_multi():
        st, stats["multi"] = mic.wsi_multi_read_patches(files, q, p, p, out.data_ptr(), out.numel())
        assert (st == 0).all()
    rec["mixed"]["multi"] = timed(by_multi, a.runs, sync)
    ref = out.cpu().numpy().copy()
    for s, img, l1 in level1:
        for i in np.nonzero(q[:, 2] == s)[0]:
            src = img if q[i, 3] == 0 else l1
            assert np.array_equal(ref[i], src[q[i, 1]: q[i, 1] + p, q[i, 0]: q[i, 0] + p])

    # the loop's groups: the patches of each (slide, level) pair.  The loop gets its patch list sorted by slide and level, so that a
    # group's patches are one slice of the tensor and no call pays for a copy to its places in the shuffled order.
    order = np.lexsort((q[:, 3], q[:, 2]))
    qs = q[order]
    out2 = torch.empty_like(out)
    groups = []
    i = 0
    while i < n:
        j = i
        while j < n and (qs[j, 2], qs[j, 3]) == (qs[i, 2], qs[i, 3]):
            j += 1
        groups.append((int(qs[i, 2]), int(qs[i, 3]), np.ascontiguousarray(qs[i:j, :2]), i, j))
        i = j
    stats["loop"] = dict(calls=len(groups), tiles_decoded=0, pieces=0, slabs=0)

    def by_loop():
        tot = dict(tiles_decoded=0, pieces=0, slabs=0)
        for s, level, xy, i0, i1 in groups:                                 # into slices of the same tensor (sorted by slide and level)
            part = out2[i0:i1]
            st, gs = mic.wsi_read_patches(files[s], level, xy, p, p, part.data_ptr(), part.numel())
            assert (st == 0).all()
            for k in tot:
                tot[k] += gs[k]
        stats["loop"].update(tot)
    rec["mixed"]["loop"] = timed(by_loop, a.runs, sync)
    assert np.array_equal(out2.cpu().numpy(), ref[order])
    rec["mixed"]["loop_over_multi_median"] = rec["mixed"]["loop"]["median_ms"] / rec["mixed"]["multi"]["median_ms"]
    rec["mixed"]["loop_over_multi_min"] = rec["mixed"]["loop"]["min_ms"] / rec["mixed"]["multi"]["min_ms"]
    del files, out, out2

    # ---- single: one slide, one level, both calls
    W = H = a.single_size
    n = a.single_patches
    img = np.ascontiguousarray(synth.wsi_like(W, H, seed=11))
    data = mic.compress_wsi(img, W, H)
    rng = np.random.default_rng(1)
    xy = np.stack([rng.integers(0, W - p, n), rng.integers(0, H - p, n)], 1).astype(np.int32)
    xysl = np.concatenate([xy, np.zeros((n, 2), dtype=np.int32)], 1)
    out = torch.empty((n, p, p, 3), dtype=torch.uint8, device="cuda")
    rec["single"] = dict(slide=[W, H], tile=256, patches=n, patch=[p, p], file_bytes=len(data))

    def one_old():
        st, stats["single_old"] = mic.wsi_read_patches(data, 0, xy, p, p, out.data_ptr(), out.numel())
        assert (st == 0).all()
    rec["single"]["old"] = timed(one_old, a.runs, sync)
    ref = out.cpu().numpy().copy()
    out.fill_(0xA5)

    def one_multi():
        st, stats["single_multi"] = mic.wsi_multi_read_patches([data], xysl, p, p, out.data_ptr(), out.numel())
        assert (st == 0).all()
    rec["single"]["multi"] = timed(one_multi, a.runs, sync)
    assert np.array_equal(out.cpu().numpy(), ref)
    rec["single"]["multi_over_old_median"] = rec["single"]["multi"]["median_ms"] / rec["single"]["old"]["median_ms"]
    rec["single"]["multi_over_old_min"] = rec["single"]["multi"]["min_ms"] / rec["single"]["old"]["min_ms"]

    rec["stats"] = stats
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)

    def short(v):
        if isinstance(v, dict):
            return {k: short(x) for k, x in v.items() if k != "runs_ms"}
        return round(v, 3) if isinstance(v, float) else v
    print(json.dumps(short(rec)))


if __name__ == "__main__":
    main()
