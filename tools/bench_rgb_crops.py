#!/usr/bin/env python3
"""Times a 2-D training sampler's read of a dataset of single-frame RGB files: 512 random 224 x 224 crops (overhang allowed) over the
RGB batch bench's ultrasound-like cine loop (tools/bench_rgb_batch.py: 256 frames of 800 x 600, synth.us_like), five ways:
  (1) whole_images   : decompress_rgb_batch of the files the crops name into buffers kept across runs, numpy crops, one upload per
                       crop (all there was before the crop calls);
  (2) session_decode : Session.rgb_decode of the named blobs, which lie in device memory, into HBM and torch slicing into the tensor;
  (3) read_crops     : one rgb_read_crops call from the files in host memory into a device tensor;
  (4) session        : one Session.rgb_read_crops call with the blobs in device memory;
  (5) typed          : (4) to bf16, channels first, with mean / std, against (4) native plus the torch operations that build that tensor.
(1) to (4) must give the same bytes.  Minimum, median and max - min spread of --runs runs after a warm-up, the device idle at the end
of each run.  The same calls (3) and (4) then run over full-colour frames of the same size (synth.wsi_like: three coded planes a
frame against the loop's mostly one), to show what a slab of coded planes alone buys: slabs and planes_decoded / planes_total of both.
The default workspace ceiling holds either call in one chain, and a process reads its ceiling once: (3) and (4) over both loops run
again in a child process under --ceiling-mb (MIC_HIP_WS_BUDGET_MB), where the chains differ.  Writes profiles/rgb_crops.json (--out)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def timed(fn, runs, sync):
    fn(); sync()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(min_ms=round(min(ts), 3), median_ms=round(statistics.median(ts), 3), spread_ms=round(max(ts) - min(ts), 3))


def clip(x, y, cw, ch, w, h):
    x0, x1, y0, y1 = max(x, 0), min(x + cw, w), max(y, 0), min(y + ch, h)
    return (x0, x1, y0, y1) if x1 > x0 and y1 > y0 else None


def encode(mic, imgs):
    blobs = []
    for i0 in range(0, len(imgs), 32):
        for st, b in mic.compress_rgb_batch(imgs[i0: i0 + 32]):
            assert st == 0, st
            blobs.append(b.copy())
    return blobs


def device_blobs(torch, blobs):
    offs = np.concatenate([[0], np.cumsum([b.size for b in blobs])]).astype(np.uint64)
    return torch.from_numpy(np.concatenate(blobs)).cuda(), offs


def under_ceiling(a, mic, synth, torch):
    """the child's part (--ceiling-child): (3) and (4) over both loops under the workspace ceiling the environment sets"""
    n, w, h = a.frames, a.width, a.height
    cw, ch = a.crop
    with ThreadPoolExecutor(16) as ex:
        grey = list(ex.map(lambda f: synth.us_like(w, h, f, seed=5), range(n)))
        tint = list(ex.map(lambda k: synth.wsi_like(w, h, seed=100 + k), range(min(n, 16))))
    rng = np.random.default_rng(7)
    xyf = np.stack([rng.integers(-cw // 2, w - cw // 2, a.crops), rng.integers(-ch // 2, h - ch // 2, a.crops), rng.integers(0, n, a.crops)], axis=1)
    t = torch.empty((a.crops, ch, cw, 3), dtype=torch.uint8, device="cuda")
    sess = mic.Session(8, w * h)
    out = {}
    for name, imgs in (("us_like", grey), ("full_colour", [tint[k % len(tint)] for k in range(n)])):
        blobs = encode(mic, imgs)
        entries = [(b, w, h) for b in blobs]
        d_all, offs = device_blobs(torch, blobs)
        keep = {}

        def read_crops():
            keep["st"], _, keep["stats"] = mic.rgb_read_crops(entries, xyf, cw, ch, t.data_ptr(), t.numel())

        def session():
            keep["st4"], _, keep["stats4"] = sess.rgb_read_crops(d_all.data_ptr(), offs, [(0, w, h)] * n, xyf, cw, ch, t.data_ptr(), t.numel())
        r = dict(read_crops=timed(read_crops, a.runs, torch.cuda.synchronize), session=timed(session, a.runs, torch.cuda.synchronize))
        assert (keep["st"] == 0).all() and (keep["st4"] == 0).all() and keep["stats"] == keep["stats4"]
        r.update({k: int(v) for k, v in keep["stats"].items()})
        out[name] = r
    sess.close()
    print("CEILING " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ceiling-mb", type=int, default=4096, help="the workspace ceiling of the second, child run (MIC_HIP_WS_BUDGET_MB)")
    ap.add_argument("--ceiling-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--crops", type=int, default=512)
    ap.add_argument("--crop", type=int, nargs=2, default=[224, 224], metavar=("CW", "CH"))
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgb_crops.json"))
    a = ap.parse_args()
    import torch
    mic = entry.load_package()
    synth = importlib.import_module("medical_image_codec_amd.synth")
    if a.ceiling_child:
        return under_ceiling(a, mic, synth, torch)
    n, w, h = a.frames, a.width, a.height
    cw, ch = a.crop
    with ThreadPoolExecutor(16) as ex:
        imgs = list(ex.map(lambda f: synth.us_like(w, h, f, seed=5), range(n)))
        tint = list(ex.map(lambda k: synth.wsi_like(w, h, seed=100 + k), range(min(n, 16))))
    blobs = encode(mic, imgs)
    rng = np.random.default_rng(7)
    xyf = np.stack([rng.integers(-cw // 2, w - cw // 2, a.crops), rng.integers(-ch // 2, h - ch // 2, a.crops), rng.integers(0, n, a.crops)], axis=1)
    entries = [(b, w, h) for b in blobs]
    file_of, planes, pieces, _ = mic.rgb_crop_plan(entries, xyf, cw, ch)
    named = [int(f) for f in file_of]
    place = {f: k for k, f in enumerate(named)}
    sync = torch.cuda.synchronize
    keep = {}
    nbytes = a.crops * ch * cw * 3
    # (1)
    outs = [np.empty(w * h * 3, dtype=np.uint8) for _ in named]

    def whole_images():
        res = mic.decompress_rgb_batch([blobs[f] for f in named], [(w, h)] * len(named), outs)
        crops = []
        for x, y, f in xyf:
            c = np.zeros((ch, cw, 3), np.uint8)
            o = clip(int(x), int(y), cw, ch, w, h)
            if o:
                x0, x1, y0, y1 = o
                c[y0 - y: y1 - y, x0 - x: x1 - x] = res[place[int(f)]][1][y0:y1, x0:x1]
            crops.append(torch.from_numpy(c).cuda())
        keep["t1"] = crops
    # (2): the named blobs back to back on the device, decoded into one tensor of whole images
    sess = mic.Session(8, w * h)
    d_named, offs_named = device_blobs(torch, [blobs[f] for f in named])
    table = [(k * w * h * 3, w, h) for k in range(len(named))]
    d_images = torch.empty((len(named), h, w, 3), dtype=torch.uint8, device="cuda")
    t2 = torch.empty((a.crops, ch, cw, 3), dtype=torch.uint8, device="cuda")
    clips = [(i, place.get(int(f), -1), int(x), int(y), clip(int(x), int(y), cw, ch, w, h)) for i, (x, y, f) in enumerate(xyf)]

    def session_decode():
        st, fp = sess.rgb_decode(d_named.data_ptr(), offs_named, table, d_images.data_ptr())
        assert (st == 0).all()
        t2.zero_()
        for i, k, x, y, o in clips:
            if o:
                x0, x1, y0, y1 = o
                t2[i, y0 - y: y1 - y, x0 - x: x1 - x] = d_images[k, y0:y1, x0:x1]
    # (3), (4)
    t3, t4 = torch.empty_like(t2), torch.empty_like(t2)
    d_all, offs_all = device_blobs(torch, blobs)
    images_all = [(0, w, h)] * n

    def read_crops():
        keep["st3"], _, keep["stats3"] = mic.rgb_read_crops(entries, xyf, cw, ch, t3.data_ptr(), nbytes)

    def session():
        keep["st4"], _, keep["stats4"] = sess.rgb_read_crops(d_all.data_ptr(), offs_all, images_all, xyf, cw, ch, t4.data_ptr(), nbytes)
    # (5)
    pairs = [(1.0 / (255.0 * s), -m / s) for m, s in zip(MEAN, STD)]
    spec = mic.OutSpec("bf16", channels_first=True, affine=pairs)
    t5 = torch.empty((a.crops, 3, ch, cw), dtype=torch.bfloat16, device="cuda")
    ta = torch.tensor([p[0] for p in pairs], dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    tb = torch.tensor([p[1] for p in pairs], dtype=torch.float32, device="cuda").view(1, 3, 1, 1)

    def typed():
        sess.rgb_read_crops(d_all.data_ptr(), offs_all, images_all, xyf, cw, ch, t5.data_ptr(), t5.numel() * 2, spec=spec)

    def native_plus_torch():
        session()
        keep["t5"] = (t4.permute(0, 3, 1, 2).float() * ta + tb).to(torch.bfloat16).contiguous()
    r = dict(device=mic.device_name(), frames=n, shape=[h, w], crops=a.crops, crop=[ch, cw], runs=a.runs, generator="synth.us_like(seed=5)",
             file_bytes=int(sum(b.size for b in blobs)), files_named=len(named))
    r["whole_images"] = timed(whole_images, a.runs, sync)
    r["session_decode"] = timed(session_decode, a.runs, sync)
    r["read_crops"] = timed(read_crops, a.runs, sync)
    r["session"] = timed(session, a.runs, sync)
    r["typed"] = timed(typed, a.runs, sync)
    r["native_plus_torch"] = timed(native_plus_torch, a.runs, sync)
    want = torch.stack(keep["t1"])
    assert torch.equal(want, t2) and torch.equal(want, t3) and torch.equal(want, t4), "the four ways disagree"
    assert (keep["st3"] == 0).all() and (keep["st4"] == 0).all() and keep["stats3"] == keep["stats4"]
    stats = keep["stats3"]
    assert stats["planes_decoded"] == planes and stats["pieces"] == pieces
    # the same tensor inside the images (fma against multiply, then add: a bf16 step at most); outside them the typed door writes its
    # pad, 0, where the torch operations turn the native door's 0 into b
    inside = np.zeros((a.crops, 1, ch, cw), dtype=bool)
    for i, k, x, y, o in clips:
        if o:
            inside[i, 0, o[2] - y: o[3] - y, o[0] - x: o[1] - x] = True
    inside = torch.from_numpy(inside).cuda()
    r["typed"]["max_abs_diff_vs_torch_inside"] = float(((t5.float() - keep["t5"].float()).abs() * inside).max().item())
    assert bool(((t5.float() == 0) | inside).all().item())
    r.update(planes_decoded=int(stats["planes_decoded"]), planes_total=int(stats["planes_total"]), pieces=int(pieces), slabs=int(stats["slabs"]),
             planes_decoded_share=round(stats["planes_decoded"] / stats["planes_total"], 4))
    for k, base in (("read_crops", "whole_images"), ("session", "session_decode"), ("typed", "native_plus_torch")):
        r[k]["against"] = base
        r[k]["speedup_min"] = round(r[base]["min_ms"] / r[k]["min_ms"], 2)
        r[k]["speedup_median"] = round(r[base]["median_ms"] / r[k]["median_ms"], 2)
        r[k]["at_or_below_beyond_spread"] = bool(r[base]["min_ms"] - r[k]["min_ms"] > r[base]["spread_ms"])
    sess.set_timing(2)
    session(); sync()
    r["session_kernels_ms"] = {k: round(v, 3) for k, v in sess.last_timings()}
    sess.set_timing(0)
    # full colour: the same crops of frames whose three planes are all coded
    del d_images, d_named, outs
    colour = [tint[k % len(tint)] for k in range(n)]
    cblobs = encode(mic, colour)
    centries = [(b, w, h) for b in cblobs]
    d_call, offs_call = device_blobs(torch, cblobs)

    def colour_read_crops():
        keep["cst"], _, keep["cstats"] = mic.rgb_read_crops(centries, xyf, cw, ch, t3.data_ptr(), nbytes)

    def colour_session():
        keep["cst4"], _, keep["cstats4"] = sess.rgb_read_crops(d_call.data_ptr(), offs_call, images_all, xyf, cw, ch, t4.data_ptr(), nbytes)
    c = dict(generator="synth.wsi_like, %d distinct frames repeated" % len(tint), file_bytes=int(sum(b.size for b in cblobs)))
    c["read_crops"] = timed(colour_read_crops, a.runs, sync)
    c["session"] = timed(colour_session, a.runs, sync)
    assert (keep["cst"] == 0).all() and torch.equal(t3, t4) and keep["cstats"] == keep["cstats4"]
    i0 = next(i for i, k, x, y, o in clips if o)
    x, y, f = (int(v) for v in xyf[i0])
    x0, x1, y0, y1 = clips[i0][4]
    assert np.array_equal(t3[i0].cpu().numpy()[y0 - y: y1 - y, x0 - x: x1 - x], colour[f][y0:y1, x0:x1])
    cs = keep["cstats"]
    c.update(planes_decoded=int(cs["planes_decoded"]), planes_total=int(cs["planes_total"]), slabs=int(cs["slabs"]),
             planes_decoded_share=round(cs["planes_decoded"] / cs["planes_total"], 4))
    r["full_colour"] = c
    sess.close()
    # the ceiling is read once per process: both loops again in a child under a ceiling that one chain of them does not fit
    import subprocess
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--ceiling-child", "--frames", str(n), "--width", str(w), "--height", str(h),
                            "--crops", str(a.crops), "--crop", str(cw), str(ch), "--runs", str(a.runs)],
                           env=dict(os.environ, MIC_HIP_WS_BUDGET_MB=str(a.ceiling_mb)), capture_output=True, text=True, timeout=600)
    line = [ln for ln in child.stdout.splitlines() if ln.startswith("CEILING ")]
    assert child.returncode == 0 and line, child.stdout + child.stderr
    r["under_ceiling"] = dict(ceiling_mb=a.ceiling_mb, **json.loads(line[0][len("CEILING "):]))
    print(json.dumps(r))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(r, indent=1) + "\n")


if __name__ == "__main__":
    main()
