"""RGB: one batch call against the per-image loop, on an ultrasound-like cine loop (256 frames of 800 x 600, synth.us_like).

Three figures, all from this tree's library in one process, the rounds alternating between them:
  (a) the loop of mic_hip_rgb_compress / mic_hip_rgb_decompress single calls -- the single-image path, which the batch leaves as it was;
  (b) ONE mic_hip_rgb_compress_batch / mic_hip_rgb_decompress_batch call over the same frames;
  (c) mic_hip_session_rgb_encode / _decode on frames and blobs that already lie on the device.
Host buffers in and out for (a) and (b), pageable and pinned.  min / median wall ms over --steps after --warmup (every call ends in a
device synchronisation); GB/s count raw RGB bytes.  (b)'s files must equal (a)'s byte for byte: asserted.  Then the two forms of
k_rgb_batch_planes -- a lane loading bytes one at a time, or four pixels as three dwords -- by HIP events through the session's
timing, alternating.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_rgb_batch.py [--frames 256] [--width 800] [--height 600] [--steps 10] [--warmup 2] [--out profiles/rgb_batch.json]"""
import argparse
import ctypes as C
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


def stats(t):
    return {"min_ms": round(min(t), 3), "median_ms": round(statistics.median(t), 3)}


def timed_rounds(fns, steps, warmup):
    """every fn `warmup` times, then `steps` rounds that run each fn once in turn: {name: [ms]}"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    t = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            t0 = time.perf_counter(); fn(); t[k].append((time.perf_counter() - t0) * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as entry
    mic = entry.load_package()
    synth = importlib.import_module("medical_image_codec_amd.synth")
    assert mic.device_name(), "no gfx950 device: nothing is measured without one"
    n, W, H = args.frames, args.width, args.height
    with ThreadPoolExecutor(8) as ex:
        px = np.stack(list(ex.map(lambda f: synth.us_like(W, H, f, seed=5), range(n))))
    raw = px.nbytes
    L = mic.lib()
    cap = mic.rgb_bound(W, H)
    res = {"workload": {"frames": n, "width": W, "height": H, "generator": "synth.us_like(seed=5)", "raw_bytes": raw}, "device": mic.device_name(),
           "steps": args.steps, "warmup": args.warmup}
    for kind in ("pageable", "pinned"):
        pinned = kind == "pinned"
        if pinned:
            src = mic.host_alloc(raw).reshape(px.shape); src[...] = px
            outs_a = [mic.host_alloc(cap) for _ in range(n)]; outs_b = [mic.host_alloc(cap) for _ in range(n)]
            back = [mic.host_alloc(W * H * 3) for _ in range(n)]
        else:
            src = px
            outs_a = [np.empty(cap, np.uint8) for _ in range(n)]; outs_b = [np.empty(cap, np.uint8) for _ in range(n)]
            back = [np.empty(W * H * 3, np.uint8) for _ in range(n)]
        imgs = [src[i] for i in range(n)]
        lens = [C.c_size_t(0) for _ in range(n)]
        files = {}

        def loop_enc():
            for i in range(n):
                rc = L.mic_hip_rgb_compress(imgs[i].ctypes.data, W, H, outs_a[i].ctypes.data, cap, C.byref(lens[i]))
                assert rc == 0, rc

        def loop_dec():
            for i in range(n):
                rc = L.mic_hip_rgb_decompress(outs_a[i].ctypes.data, lens[i].value, W, H, back[i].ctypes.data, back[i].size)
                assert rc == 0, rc

        def batch_enc():
            r = mic.compress_rgb_batch(imgs, False, outs=outs_b)
            assert all(st == 0 for st, _ in r)
            files["b"] = [b for _, b in r]

        def batch_dec():
            r = mic.decompress_rgb_batch(files["b"], [(W, H)] * n, outs=back)
            assert all(st == 0 for st, _ in r)

        t = timed_rounds({"loop_encode": loop_enc, "batch_encode": batch_enc}, args.steps, args.warmup)
        same = all(files["b"][i].tobytes() == outs_a[i][: lens[i].value].tobytes() for i in range(n))
        assert same, "a batch file differs from the single call's"
        for b in back:
            b[...] = 0
        t.update(timed_rounds({"loop_decode": loop_dec}, args.steps, args.warmup))
        assert all(np.array_equal(b.reshape(H, W, 3), px[i]) for i, b in enumerate(back))
        for b in back:
            b[...] = 0
        t.update(timed_rounds({"batch_decode": batch_dec}, args.steps, args.warmup))
        assert all(np.array_equal(b.reshape(H, W, 3), px[i]) for i, b in enumerate(back))
        for k, v in t.items():
            res[k + "_" + kind] = dict(stats(v), GBps=round(raw / min(v) / 1e6, 3))
        for d in ("encode", "decode"):
            res["ratio_%s_%s" % (d, kind)] = round(statistics.median(t["loop_" + d]) / statistics.median(t["batch_" + d]), 2)
        res["batch_files_equal_loop_files"] = bool(same and res.get("batch_files_equal_loop_files", True))
        res["compressed_bytes"] = int(sum(v.value for v in lens))
        if pinned:
            for b in [src] + outs_a + outs_b + back:
                mic.host_free(b)
    # (c) the session calls on device-resident frames, and the two forms of the plane kernel
    d_rgb = torch.from_numpy(px.reshape(-1)).cuda()
    table = mic.Session.make_rgb_images([(i * W * H * 3, W, H) for i in range(n)])
    s = mic.Session(4, 64 * 64)
    state = {}

    def sess_enc():
        state["enc"] = s.rgb_encode(d_rgb.data_ptr(), table)
        assert (state["enc"][2] == 0).all()

    timed_rounds({"e": sess_enc}, 0, 1)
    d_blobs, offs, _, _ = state["enc"]
    keep = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda")
    mic.device_copy(keep.data_ptr(), d_blobs, int(offs[-1]))
    out = torch.zeros_like(d_rgb)

    def sess_dec():
        st, _ = s.rgb_decode(keep.data_ptr(), offs, table, out.data_ptr())
        assert (st == 0).all()

    t = timed_rounds({"session_encode": sess_enc, "session_decode": sess_dec}, args.steps, args.warmup)
    torch.cuda.synchronize()
    assert torch.equal(out, d_rgb)
    for k, v in t.items():
        res[k] = dict(stats(v), GBps=round(raw / min(v) / 1e6, 3))
    kern = {"bytewise": [], "grouped": []}
    s.set_timing(2)
    for r in range(args.steps + args.warmup):
        for name, flag in (("bytewise", 1), ("grouped", 0)):
            L.mic_hip_debug_rgb_planes_bytewise(flag)
            s.set_timing(2)
            sess_enc()
            ms = dict(s.last_timings()).get("k_rgb_batch_planes")
            if r >= args.warmup and ms is not None:
                kern[name].append(ms)
    L.mic_hip_debug_rgb_planes_bytewise(0)
    s.set_timing(0)
    s.close()
    res["plane_kernel"] = {k: dict(stats(v), GBps_rgb_in=round(raw / min(v) / 1e6, 1)) for k, v in kern.items() if v}
    if len(res["plane_kernel"]) == 2:
        res["plane_kernel"]["shipped"] = "grouped"
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
