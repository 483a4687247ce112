#!/usr/bin/env python3
"""The MIC3 tile cache against the tree without it.  Three workloads, one warm-up and the min of --runs calls each, wall time
around the call and a device synchronise, as tools/bench_wsi_patches.py measures:
  (a) one slide:   512 random 256 x 256 patches of level 0 of an 8192 x 8192 RGB slide (1024 tiles), FRESH origins every call,
                   through a WsiReader and through the session store; without a cache, cold with an empty cache that holds the
                   slide, and in steady state with that cache
  (b) thrashing:   (a) with a cache of half the slide's tiles
  (c) many slides: 8 patches from each of 64 slides of 2048 x 2048 at levels 0 and 1, through wsi_readers_read_patches, the
                   readers sharing one cache
The yardstick is the PARENT commit, built in a directory of its own and run by this same file:

  python tools/bench_wsi_tile_cache.py --root <parent checkout> --out parent.json      # (a tree without TileCache runs the uncached rows only)
  python tools/bench_wsi_tile_cache.py --parent parent.json [--out profiles/wsi_tile_cache.json]

With --parent the record holds both trees' rows and the ratios the cache is judged by."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(root):
    spec = importlib.util.spec_from_file_location("graft_entry_under_test", os.path.join(root, "__graft_entry__.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    return entry.load_package()


def timed(fn, runs, sync, warm=1):
    """fn(k) for call k; the first `warm` calls are not counted"""
    ts = []
    for k in range(warm + runs):
        t0 = time.perf_counter()
        fn(k); sync()
        if k >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return dict(min_ms=min(ts), max_ms=max(ts), median_ms=statistics.median(ts), runs_ms=ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE, help="the checkout to measure (its libmic_hip.so must be built)")
    ap.add_argument("--parent", default=None, help="the record of the parent commit, made by this tool with --root")
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--patches", type=int, default=512)
    ap.add_argument("--patch", type=int, default=256)
    ap.add_argument("--slides", type=int, default=64)
    ap.add_argument("--slide-size", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "wsi_tile_cache.json"))
    a = ap.parse_args()
    import torch
    mic = load(os.path.abspath(a.root))
    synth = importlib.import_module("medical_image_codec_amd.synth")
    cached = hasattr(mic, "TileCache")
    sync = torch.cuda.synchronize
    W = H = a.size
    n, p = a.patches, a.patch
    rec = dict(device=mic.device_name(), has_cache=cached, runs=a.runs, slide=[W, H], tile=256, patches=n, patch=[p, p])

    img = np.ascontiguousarray(synth.wsi_like(W, H, seed=11))
    data = mic.compress_wsi(img, W, H)
    ntiles = ((W + 255) // 256) * ((H + 255) // 256)
    rng = np.random.default_rng(1)
    origins = [np.stack([rng.integers(0, W - p, n), rng.integers(0, H - p, n)], 1).astype(np.int32) for _ in range(a.runs + 3)]
    out = torch.empty((n, p, p, 3), dtype=torch.uint8, device="cuda")

    def check(xy):
        got = out.cpu().numpy()
        for i in (0, n // 2, n - 1):
            assert np.array_equal(got[i], img[xy[i, 1]: xy[i, 1] + p, xy[i, 0]: xy[i, 0] + p])

    sess = mic.Session(3 * 1024, 256 * 256)
    d_img = torch.from_numpy(img.reshape(-1)).cuda()
    sess.wsi_encode(d_img.data_ptr(), W, H)
    rd = mic.WsiReader(data)
    doors = dict(reader=lambda xy: rd.read_patches(0, xy, p, p, out.data_ptr(), out.numel()),
                 store=lambda xy: sess.wsi_read_patches(0, xy, p, p, out.data_ptr(), out.numel()))
    attach = dict(reader=lambda c: rd.set_cache(c), store=lambda c: sess.set_tile_cache(c)) if cached else {}
    one = {}
    for door, call in doors.items():
        row = {}
        row["no_cache"] = timed(lambda k: call(origins[k]), a.runs, sync)
        check(origins[a.runs])
        if cached:
            for name, slots in (("holds_slide", ntiles), ("half_slide", ntiles // 2)):
                cache = mic.TileCache(256, 256, slots=slots)
                attach[door](cache)
                cold = []
                for k in range(3):                                            # a cold call: an empty cache, arena already allocated behind the first
                    cache.clear()
                    t0 = time.perf_counter()
                    call(origins[k]); sync()
                    cold.append((time.perf_counter() - t0) * 1e3)
                row[name + "_cold_ms"] = cold[1:]
                before = cache.stats()
                row[name] = timed(lambda k: call(origins[k]), a.runs, sync, warm=3)   # (three calls of fresh origins touch nearly every tile)
                check(origins[a.runs + 2])
                after = cache.stats()
                row[name + "_stats"] = {k: after[k] - before[k] for k in ("hits", "misses", "bypassed", "evictions", "calls")}
                row[name + "_stats"]["device_bytes"] = after["device_bytes"]
                attach[door](None)
                cache.close()
        one[door] = row
    rec["one_slide"] = one
    rd.close()
    sess.close()

    # (c) many slides at two levels through readers that share a cache
    ns, sw = a.slides, a.slide_size
    files = [mic.compress_wsi(np.ascontiguousarray(synth.wsi_like(sw, sw, seed=100 + s)), sw, sw) for s in range(ns)]
    rds = [mic.WsiReader(d) for d in files]
    per_slide_tiles = (sw // 256) ** 2 + (sw // 512) ** 2 + 8
    def quads(seed):
        r = np.random.default_rng(seed)
        q = []
        for s in range(ns):
            for j in range(8):
                lv = j % 2
                lim = (sw >> lv) - p
                q.append((int(r.integers(0, lim)), int(r.integers(0, lim)), s, lv))
        return np.asarray(q, dtype=np.int32)
    qs = [quads(50 + k) for k in range(a.runs + 6)]
    out2 = torch.empty((len(qs[0]), p, p, 3), dtype=torch.uint8, device="cuda")
    many = {}
    call = lambda q: mic.wsi_readers_read_patches(rds, q, p, p, out2.data_ptr(), out2.numel())
    many["no_cache"] = timed(lambda k: call(qs[k]), a.runs, sync)
    if cached:
        cache = mic.TileCache(256, 256, slots=ns * per_slide_tiles)
        for r in rds:
            r.set_cache(cache)
        before = cache.stats()
        many["shared_cache"] = timed(lambda k: call(qs[k]), a.runs, sync, warm=6)
        after = cache.stats()
        many["shared_cache_stats"] = {k: after[k] - before[k] for k in ("hits", "misses", "bypassed", "evictions", "calls")}
        many["same_call_again"] = timed(lambda k: call(qs[0]), a.runs, sync)
        for r in rds:
            r.set_cache(None)
        cache.close()
    for r in rds:
        r.close()
    rec["many_slides"] = dict(slides=ns, slide=[sw, sw], patches=len(qs[0]), **many)

    if a.parent:
        with open(a.parent) as f:
            par = json.load(f)
        rec = dict(this=rec, parent=par, verdict={})
        v = rec["verdict"]
        for door in ("reader", "store"):
            pr, th = par["one_slide"][door]["no_cache"], rec["this"]["one_slide"][door]
            v[door] = dict(parent_min_ms=pr["min_ms"], parent_spread_ms=pr["max_ms"] - pr["min_ms"],
                           no_cache_minus_parent_min_ms=th["no_cache"]["min_ms"] - pr["min_ms"])
            if cached:
                v[door].update(steady_min_ms=th["holds_slide"]["min_ms"], parent_over_steady=pr["min_ms"] / th["holds_slide"]["min_ms"],
                               cold_ms=min(th["holds_slide_cold_ms"]), cold_over_parent=min(th["holds_slide_cold_ms"]) / pr["min_ms"],
                               thrash_min_ms=th["half_slide"]["min_ms"], thrash_over_parent=th["half_slide"]["min_ms"] / pr["min_ms"])
        pm, tm = par["many_slides"], rec["this"]["many_slides"]
        v["many_slides"] = dict(parent_min_ms=pm["no_cache"]["min_ms"], parent_spread_ms=pm["no_cache"]["max_ms"] - pm["no_cache"]["min_ms"],
                                no_cache_minus_parent_min_ms=tm["no_cache"]["min_ms"] - pm["no_cache"]["min_ms"])
        if cached:
            v["many_slides"].update(shared_cache_min_ms=tm["shared_cache"]["min_ms"], same_call_again_min_ms=tm["same_call_again"]["min_ms"])
        print(json.dumps(v, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
