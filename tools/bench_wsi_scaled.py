#!/usr/bin/env python3
"""Times the scaled MIC3 patch doors (scale=(num, den), mic_hip_*_read_patches_scaled) against what a caller did before them: the
native door at the source extent followed by framework kernels.  The workload is bench_typed_readers.py's: 512 patches of 256 x 256
out of an 8192 x 8192 RGB slide -> bf16, channels first, per-channel mean / std; from the session's store, and through a WsiReader
with a tile cache that holds the slide (warm).  Scales 2 / 1, 3 / 2 and 13 / 6.  Each cell: minimum and maximum of --runs runs
behind a warm-up, wall clock around a device synchronise:
  (a) native_torch : the native door for n rectangles of sw x sh, then torch.nn.functional.interpolate(mode="area") and the cast,
                     normalise and permute that build the same-shaped tensor (native and torch_ops are also timed alone);
  (b) scaled       : the scaled door alone.
Torch's area filter is float and, off the whole factors, not the exact area average: the comparison is of time only (the largest
difference is recorded).  One condition is recorded: scale 1 / 1 through the _scaled door against the _as door of the parent commit
on the same workload -- scaled_unit_within_parent_spread: |min - parent min| <= parent max - parent min.
--native-only --tree DIR times what a checkout of the parent commit can run (the native door at every source extent, the _as door at
256 x 256) and writes it to --out; the full run takes that file as --parent and then also reports (a) with the parent's native part.
Writes profiles/wsi_scaled.json (--out)."""
import argparse
import importlib
import importlib.util
import json
import os
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [(2, 1), (3, 2), (13, 6)]


def load(tree):
    """the package of the checkout at `tree` (its own build)"""
    spec = importlib.util.spec_from_file_location("__graft_entry__", os.path.join(tree, "__graft_entry__.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    return entry.load_package(), importlib.import_module("medical_image_codec_amd.synth")


def timed(fn, runs):
    import torch
    fn(); fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slide", type=int, default=8192)
    ap.add_argument("--patches", type=int, default=512)
    ap.add_argument("--patch", type=int, default=256)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed (its own build); default: this one")
    ap.add_argument("--native-only", action="store_true", help="time the native and _as doors alone: all a checkout of the parent commit can run")
    ap.add_argument("--parent", default=None, help="the file a --native-only run of the parent commit's checkout wrote")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wsi_scaled.json"))
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    mic, synth = load(a.tree)
    W = H = a.slide
    n, p = a.patches, a.patch
    result = dict(device=mic.device_name(), runs=a.runs, native_only=bool(a.native_only), slide=[W, H], patches=n, patch=[p, p], cells={})
    img = np.ascontiguousarray(synth.wsi_like(W, H, seed=11))
    sess = mic.Session(3 * 1024, 256 * 256)
    d_img = torch.from_numpy(img.reshape(-1)).cuda()
    sess.wsi_encode(d_img.data_ptr(), W, H)
    data = mic.compress_wsi(img, W, H)
    rd = mic.WsiReader(data)
    cache = mic.TileCache(256, 256, slots=((W + 255) // 256) * ((H + 255) // 256))
    rd.set_cache(cache)
    doors = dict(store=lambda *x, **k: sess.wsi_read_patches(0, *x, **k), reader_cached=lambda *x, **k: rd.read_patches(0, *x, **k))
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
    pairs = np.stack([1.0 / (255.0 * std), -mean / std], 1).astype(np.float32)
    ta, tb = (torch.from_numpy(pairs[:, k].copy()).cuda().view(1, 3, 1, 1) for k in range(2))
    spec = mic.OutSpec("bf16", channels_first=True, affine=pairs)
    t_typ = torch.empty((n, 3, p, p), dtype=torch.bfloat16, device="cuda")
    rng = np.random.default_rng(1)

    # scale 1 / 1: the _as door (both trees) and the _scaled door (this one)
    xy1 = np.stack([rng.integers(0, W - p, n), rng.integers(0, H - p, n)], 1).astype(np.int32)
    for door, call in doors.items():
        def typed_as(call=call):
            st, _ = call(xy1, p, p, t_typ.data_ptr(), t_typ.numel() * 2, spec=spec)
            assert (st == 0).all()
        cell = dict(typed_as=timed(typed_as, a.runs))
        if not a.native_only:
            def unit(call=call):
                st, _ = call(xy1, p, p, t_typ.data_ptr(), t_typ.numel() * 2, spec=spec, scale=(1, 1))
                assert (st == 0).all()
            cell["scaled_unit"] = timed(unit, a.runs)
        result["cells"][door + "/1_1"] = cell

    for num, den in SCALES:
        sw = sh = -(-p * num // den)
        xy = np.stack([rng.integers(0, W - sw, n), rng.integers(0, H - sh, n)], 1).astype(np.int32)
        t_nat = torch.empty((n, sh, sw, 3), dtype=torch.uint8, device="cuda")

        def torch_ops():
            x = F.interpolate(t_nat.permute(0, 3, 1, 2).to(torch.float32), size=(p, p), mode="area")
            return (x * ta + tb).to(torch.bfloat16).contiguous()
        for door, call in doors.items():
            def native(call=call):
                st, _ = call(xy, sw, sh, t_nat.data_ptr(), t_nat.numel())
                assert (st == 0).all()
            cell = dict(source=[sw, sh], native=timed(native, a.runs))
            if not a.native_only:
                keep = {}

                def both():
                    native()
                    keep["a"] = torch_ops()

                def scaled(call=call):
                    st, _ = call(xy, p, p, t_typ.data_ptr(), t_typ.numel() * 2, spec=spec, scale=(num, den))
                    assert (st == 0).all()
                cell["native_torch"] = timed(both, a.runs)
                cell["torch_ops"] = timed(lambda: keep.__setitem__("a", torch_ops()), a.runs)
                cell["scaled"] = timed(scaled, a.runs)
                torch.cuda.synchronize()
                cell["scaled_vs_torch_max_abs_diff"] = float((keep["a"].float() - t_typ.float()).abs().max().item())
                cell["scaled_over_native_torch"] = round(cell["scaled"]["min_ms"] / cell["native_torch"]["min_ms"], 3)
                cell["bytes"] = dict(native=t_nat.numel(), scaled=t_typ.numel() * 2)
            result["cells"]["%s/%d_%d" % (door, num, den)] = cell
            print(door, (num, den), json.dumps(cell), flush=True)
        del t_nat
    if not a.native_only:
        sess.set_timing(True)
        sess.wsi_read_patches(0, xy, p, p, t_typ.data_ptr(), t_typ.numel() * 2, spec=spec, scale=SCALES[-1])
        result["store_13_6_last_timings_ms"] = {k: round(v, 3) for k, v in sess.last_timings()}
    if a.parent:
        parent = json.load(open(a.parent))
        for name, cell in result["cells"].items():
            pc = parent["cells"][name]
            if "scaled_unit" in cell:
                pa = pc["typed_as"]
                cell["parent_typed_as"] = pa
                cell["scaled_unit_within_parent_spread"] = bool(abs(cell["scaled_unit"]["min_ms"] - pa["min_ms"]) <= pa["max_ms"] - pa["min_ms"])
            else:
                cell["parent_native"] = pc["native"]
                cell["parent_native_plus_torch_ops_min_ms"] = round(pc["native"]["min_ms"] + cell["torch_ops"]["min_ms"], 3)
    rd.set_cache(None)
    cache.close()
    rd.close()
    sess.close()
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
