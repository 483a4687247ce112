#!/usr/bin/env python3
"""Times the typed output of the patch and crop readers (OutSpec, mic_hip_*_as) against what a caller did before it: the native
door followed by framework kernels.  Three workloads, taken from bench_wsi_patches.py, bench_mic2_crops.py and bench_strips_crops.py:
  wsi    : 512 patches of 256 x 256 of an 8192 x 8192 RGB slide in the session's store -> bf16, channels first, per-channel mean / std;
  mic2   : 64 crops of 128 x 128 x 64 of a 256-frame 512 x 512 MIC2 stack in device memory, coded independent and temporal
           -> f32 with the volume's slope / intercept;
  strips : 512 crops of 512 x 512 over 288 XR-shaped 12-bit PICS-8 files in device memory -> f16 through a window, clamped to [0, 1].
Each three ways, timed with events on the session's stream (the torch operations run on that stream too): minimum and maximum of
--runs runs after a warm-up:
  (a) native       : the native door;
  (b) native_torch : the native door, then the torch operations that build the same tensor (.to, multiply and add, clamp,
                     permute().contiguous());
  (c) typed        : the typed door alone;
and (a') native_as: the native format through the _as door (a NATIVE spec).  (c) is checked against (b): equal up to the one
rounding the fused multiply-add saves.  The conditions recorded: c_le_b -- (c).min <= (b).min + ((a).max - (a).min) --, and, with
--parent FILE (what `--native-only --tree DIR` wrote for a checkout of the parent commit), as_native_within_parent_spread.
Writes profiles/typed_readers.json (--out)."""
import argparse
import importlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(tree):
    """the package of the checkout at `tree` (its own build)"""
    spec = importlib.util.spec_from_file_location("__graft_entry__", os.path.join(tree, "__graft_entry__.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    return entry.load_package(), importlib.import_module("medical_image_codec_amd.synth")


def timed(fn, runs, stream):
    import torch
    fn(); fn()
    stream.synchronize()
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def measure(name, sess, native, torch_ops, typed, native_as, runs, native_only, out_bytes):
    """native() / typed() / native_as() fill their tensors; torch_ops() builds (b)'s tensor from native()'s -> this workload's record"""
    import torch
    stream = torch.cuda.ExternalStream(sess.stream)
    rec = {}
    with torch.cuda.stream(stream):
        rec["native"] = timed(native, runs, stream)
        if not native_only:
            keep = {}

            def both():
                native()
                keep["b"] = torch_ops()
            rec["native_torch"] = timed(both, runs, stream)
            rec["typed"] = timed(lambda: keep.__setitem__("c", typed()), runs, stream)
            rec["native_as"] = timed(native_as, runs, stream)
            stream.synchronize()
            b, c = keep["b"].float(), keep["c"].float()
            rec["typed_vs_torch_max_abs_diff"] = float((b - c).abs().max().item())
            assert torch.allclose(b, c, rtol=2.0 ** -7, atol=2.0 ** -10), (name, rec["typed_vs_torch_max_abs_diff"])
            spread = rec["native"]["max_ms"] - rec["native"]["min_ms"]
            rec["native_spread_ms"] = round(spread, 3)
            rec["c_le_b"] = bool(rec["typed"]["min_ms"] <= rec["native_torch"]["min_ms"] + spread)
            rec["typed_minus_native_ms"] = round(rec["typed"]["min_ms"] - rec["native"]["min_ms"], 3)
            rec["bytes_stored"] = out_bytes
    print(name, json.dumps(rec), flush=True)
    return rec


def wsi(mic, synth, a):
    import torch
    W = H = a.slide
    n, p = a.patches, a.patch
    img = np.ascontiguousarray(synth.wsi_like(W, H, seed=11))
    rng = np.random.default_rng(1)
    xy = np.stack([rng.integers(0, W - p, n), rng.integers(0, H - p, n)], 1).astype(np.int32)
    sess = mic.Session(3 * 1024, 256 * 256)
    d_img = torch.from_numpy(img.reshape(-1)).cuda()
    sess.wsi_encode(d_img.data_ptr(), W, H)
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])     # the usual ImageNet normalisation of x / 255
    pairs = np.stack([1.0 / (255.0 * std), -mean / std], 1).astype(np.float32)
    t_nat = torch.empty((n, p, p, 3), dtype=torch.uint8, device="cuda")
    t_typ = torch.empty((n, 3, p, p), dtype=torch.bfloat16, device="cuda")
    ta, tb = (torch.from_numpy(pairs[:, k].copy()).cuda() for k in range(2))

    def native():
        st, _ = sess.wsi_read_patches(0, xy, p, p, t_nat.data_ptr(), t_nat.numel())
        assert (st == 0).all()

    def torch_ops():
        return (t_nat.to(torch.float32) * ta + tb).to(torch.bfloat16).permute(0, 3, 1, 2).contiguous()
    if a.native_only:
        return sess, native, None, None, None, 0
    spec, nspec = mic.OutSpec("bf16", channels_first=True, affine=pairs), mic.OutSpec("native")

    def typed():
        st, _ = sess.wsi_read_patches(0, xy, p, p, t_typ.data_ptr(), t_typ.numel() * 2, spec=spec)
        assert (st == 0).all()
        return t_typ

    def native_as():
        sess.wsi_read_patches(0, xy, p, p, t_nat.data_ptr(), t_nat.numel(), spec=nspec)
    return sess, native, torch_ops, typed, native_as, dict(native=t_nat.numel(), typed=t_typ.numel() * 2)


def mic2(mic, synth, a, temporal):
    import torch
    n, w, h = a.frames, 512, 512
    cw, ch, cd = 128, 128, 64
    img = synth.xr_like(cols=w, rows=h, depth=12, seed=100)
    vol = np.stack([np.roll(img, 3 * k, axis=1) for k in range(n)])
    data = mic.compress_multi_frame(vol, w, h, 4095, temporal=temporal)
    rng = np.random.default_rng(7)
    nc = a.crops3d
    xyzv = np.stack([rng.integers(0, w - cw + 1, nc), rng.integers(0, h - ch + 1, nc), rng.integers(0, n - cd + 1, nc), np.zeros(nc, dtype=np.int64)], 1)
    sess = mic.Session(8, w * h)
    d_file = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    heads, ptrs, lens = [data[: 20 + 8 * n]], [d_file.data_ptr()], [len(data)]
    slope, intercept = 1.0, -1024.0                                                   # a CT-like rescale
    t_nat = torch.empty((nc, cd, ch, cw), dtype=torch.int16, device="cuda")           # (u16 samples: 12 bits, so int16 reads them)
    t_typ = torch.empty((nc, cd, ch, cw), dtype=torch.float32, device="cuda")

    def native():
        st, _, _ = sess.mic2_multi_read_crops(heads, ptrs, lens, xyzv, cw, ch, cd, t_nat.data_ptr(), t_nat.numel() * 2)
        assert (st == 0).all()

    def torch_ops():
        return t_nat.to(torch.float32) * slope + intercept
    if a.native_only:
        return (sess, d_file), native, None, None, None, 0
    spec, nspec = mic.OutSpec("f32", affine=[(slope, intercept)]), mic.OutSpec("native")

    def typed():
        st, _, _ = sess.mic2_multi_read_crops(heads, ptrs, lens, xyzv, cw, ch, cd, t_typ.data_ptr(), t_typ.numel() * 4, spec=spec)
        assert (st == 0).all()
        return t_typ

    def native_as():
        sess.mic2_multi_read_crops(heads, ptrs, lens, xyzv, cw, ch, cd, t_nat.data_ptr(), t_nat.numel() * 2, spec=nspec)
    return (sess, d_file), native, torch_ops, typed, native_as, dict(native=t_nat.numel() * 2, typed=t_typ.numel() * 4)


def strips(mic, synth, a):
    import torch
    n, w, h, cw, ch = a.images, 2577, 2048, 512, 512
    d_px = synth.xr_like_batch_torch(n, cols=w, rows=h, depth=12, seed0=1, noise=synth.XR_NOISE_PUBLISHED_RATIO, device="cuda")
    images = d_px.cpu().numpy().view(np.uint16)
    del d_px
    files = []
    for i0 in range(0, n, 48):
        for st, f in mic.compress_parallel_strips_batch(list(images[i0: i0 + 48]), 4095, 8, 2):
            assert st == 0, st
            files.append(f.copy())
    del images
    rng = np.random.default_rng(7)
    nc = a.crops2d
    xyf = np.stack([rng.integers(0, w - cw + 1, nc), rng.integers(0, h - ch + 1, nc), rng.integers(0, n, nc)], axis=1)
    sess = mic.Session(8, w * (h // 8 + 1))
    lens = [f.size for f in files]
    offs = np.concatenate([[0], np.cumsum([(ln + 255) // 256 * 256 for ln in lens])])
    d_all = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda")
    for f, o in zip(files, offs):
        d_all[int(o): int(o) + f.size] = torch.from_numpy(f).cuda()
    ptrs = [d_all.data_ptr() + int(o) for o in offs[:-1]]
    heads = [mic.strips_head(f) for f in files]
    a_, b_ = 1.0 / 1024, -1.5                                                         # window centre 2048, width 1024 -> [0, 1]
    t_nat = torch.empty((nc, ch, cw), dtype=torch.int16, device="cuda")
    t_typ = torch.empty((nc, ch, cw), dtype=torch.float16, device="cuda")

    def native():
        st, _, _ = sess.strips_read_crops(heads, ptrs, lens, xyf, cw, ch, t_nat.data_ptr(), t_nat.numel() * 2)
        assert (st == 0).all()

    def torch_ops():
        return (t_nat.to(torch.float32) * a_ + b_).clamp(0.0, 1.0).to(torch.float16)
    if a.native_only:
        return (sess, d_all), native, None, None, None, 0
    spec, nspec = mic.OutSpec("f16", affine=[(a_, b_)], clamp=(0.0, 1.0)), mic.OutSpec("native")

    def typed():
        st, _, _ = sess.strips_read_crops(heads, ptrs, lens, xyf, cw, ch, t_typ.data_ptr(), t_typ.numel() * 2, spec=spec)
        assert (st == 0).all()
        return t_typ

    def native_as():
        sess.strips_read_crops(heads, ptrs, lens, xyf, cw, ch, t_nat.data_ptr(), t_nat.numel() * 2, spec=nspec)
    return (sess, d_all), native, torch_ops, typed, native_as, dict(native=t_nat.numel() * 2, typed=t_typ.numel() * 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slide", type=int, default=8192)
    ap.add_argument("--patches", type=int, default=512)
    ap.add_argument("--patch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--crops3d", type=int, default=64)
    ap.add_argument("--images", type=int, default=288)
    ap.add_argument("--crops2d", type=int, default=512)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed (its own build); default: this one")
    ap.add_argument("--native-only", action="store_true", help="time (a) alone: all a checkout of the parent commit can run")
    ap.add_argument("--parent", default=None, help="the file a --native-only run of the parent commit's checkout wrote")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "typed_readers.json"))
    a = ap.parse_args()
    mic, synth = load(a.tree)
    result = dict(device=mic.device_name(), runs=a.runs, native_only=bool(a.native_only), workloads={})
    for name, make in (("wsi_rgb_bf16_channels_first", lambda: wsi(mic, synth, a)),
                       ("mic2_independent_f32", lambda: mic2(mic, synth, a, False)),
                       ("mic2_temporal_f32", lambda: mic2(mic, synth, a, True)),
                       ("strips_f16_window", lambda: strips(mic, synth, a))):
        keep, native, torch_ops, typed, native_as, nbytes = make()
        sess = keep[0] if isinstance(keep, tuple) else keep
        result["workloads"][name] = measure(name, sess, native, torch_ops, typed, native_as, a.runs, a.native_only, nbytes)
        sess.close()
        del keep
    if a.parent:
        parent = json.load(open(a.parent))
        for name, rec in result["workloads"].items():
            p = parent["workloads"][name]["native"]
            rec["parent_native"] = p
            rec["as_native_within_parent_spread"] = bool(abs(rec["native_as"]["min_ms"] - p["min_ms"]) <= p["max_ms"] - p["min_ms"])
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
