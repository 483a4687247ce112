"""PICA: one batch call against the per-image loop, on the XR-shaped 12-bit frames bench.py uses (288 x 2577 x 2048, 8 strips).

Each measurement runs in a child process of its own (one library per process), alternating A / B:
  A  --lib PATH: another build of libmic_hip.so (the parent commit's), looping over mic_hip_pica_compress / _decompress;
  B  this tree's library: the same loop, then ONE mic_hip_pica_compress_batch / _decompress_batch call over the same frames and the
     PICS batch on the same frames for context.
Then, each a pass of its own: the per-kernel device times of a PICA batch call from A / B builds of this tree (--timing-lib:
EXTRA_FLAGS=-DMIC_PICA_TIMING; --nopick-lib: -DMIC_PICA_TIMING -DMIC_PICA_NO_PICK, the pack WITHOUT k_pica_pick; neither switch exists
in the product library), and the avg and gradient chains over the same 768 equal strips through the session API with timing on, for
this tree and for every build of --session-libs (the parent, variants of k_dec_predict_grad).
Host buffers in and out, pageable and pinned.  min / median wall ms over --steps after --warmup; GB/s count raw pixels.
Prints one JSON line.

    python tools/bench_pica_batch.py [--images 288] [--steps 10] [--warmup 2] [--rounds 3] [--lib parent/libmic_hip.so] [--timing-lib ...] [--nopick-lib ...]
        [--session-libs parent=...,ahead1=...] [--reuse-rounds earlier.json ...]"""
import argparse
import ctypes as C
import importlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, STRIPS, MAXV = 2577, 2048, 8, 4095


def frames(n):
    import torch
    import __graft_entry__ as entry
    entry.load_package()
    synth = importlib.import_module("medical_image_codec_amd.synth")
    d = synth.xr_like_batch_torch(n, cols=W, rows=H, depth=12, seed0=1, noise=synth.XR_NOISE_PUBLISHED_RATIO, device=torch.device("cuda:0"))
    a = d.cpu().numpy().astype(np.uint16).reshape(n, H, W)
    del d
    return a


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": round(min(t), 3), "median_ms": round(statistics.median(t), 3)}


def child_loop(args):
    """the per-image loop through the C ABI of --lib (or this tree's library)"""
    px = frames(args.images)
    L = C.CDLL(args.lib or os.path.join(ROOT, "medical-image-codec_amd", "libmic_hip.so"))
    L.mic_hip_pica_compress.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint16, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_pica_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    L.mic_hip_host_alloc.restype = C.c_void_p; L.mic_hip_host_alloc.argtypes = [C.c_size_t]
    n = args.images
    cap = 16 + 16 * STRIPS + 4 * W * H + 135168 * STRIPS
    res = {}
    for kind in ("pageable", "pinned"):
        if kind == "pinned":
            def pin(nbytes, dt):
                p = L.mic_hip_host_alloc(nbytes)
                return np.frombuffer((C.c_uint8 * nbytes).from_address(p), dtype=np.uint8).view(dt)
            src = pin(px.nbytes, np.uint16).reshape(px.shape); src[...] = px
            outs = [pin(cap, np.uint8) for _ in range(n)]; back = pin(px.nbytes, np.uint16).reshape(px.shape)
        else:
            src = px; outs = [np.empty(cap, np.uint8) for _ in range(n)]; back = np.empty_like(px)
        lens = [C.c_size_t(0) for _ in range(n)]

        def enc():
            for i in range(n):
                rc = L.mic_hip_pica_compress(src[i].ctypes.data, W, H, MAXV, STRIPS, outs[i].ctypes.data, cap, C.byref(lens[i]))
                assert rc == 0, rc

        def dec():
            for i in range(n):
                rc = L.mic_hip_pica_decompress(outs[i].ctypes.data, lens[i].value, back[i].ctypes.data, W, H)
                assert rc == 0, rc
        res["loop_encode_" + kind] = timed(enc, args.steps, args.warmup)
        res["loop_decode_" + kind] = timed(dec, args.steps, args.warmup)
        assert np.array_equal(back, px)
        res["compressed_bytes"] = int(sum(v.value for v in lens))
    print(json.dumps(res))


def child_batch(args):
    import __graft_entry__ as entry
    px = frames(args.images)
    mic = entry.load_package()
    n = args.images
    res = {}
    for kind in ("pageable", "pinned"):
        pinned = kind == "pinned"
        if pinned:
            src = mic.host_alloc(px.nbytes, np.uint16).reshape(px.shape); src[...] = px
            outs = [mic.host_alloc(mic.pica_bound(W, H, STRIPS)) for _ in range(n)]
            back = [mic.host_alloc(W * H * 2, np.uint16) for _ in range(n)]
        else:
            src = px; outs = [np.empty(mic.pica_bound(W, H, STRIPS), np.uint8) for _ in range(n)]; back = [np.empty(W * H, np.uint16) for _ in range(n)]
        imgs = [src[i] for i in range(n)]
        files = {}

        def enc():
            r = mic.compress_parallel_strips_adaptive_batch(imgs, MAXV, STRIPS, outs=outs)
            assert all(st == 0 for st, _ in r)
            files["pica"] = [b for _, b in r]

        def dec():
            r = mic.decompress_parallel_strips_adaptive_batch(files["pica"], [(W, H)] * n, outs=back)
            assert all(st == 0 for st, _ in r)

        def pics_enc():
            r = mic.compress_parallel_strips_batch(imgs, MAXV, STRIPS, 2, outs=outs)
            assert all(st == 0 for st, _ in r)
            files["pics"] = [b for _, b in r]

        def pics_dec():
            r = mic.decompress_parallel_strips_batch(files["pics"], [(W, H)] * n, outs=back)
            assert all(st == 0 for st, _ in r)
        res["batch_encode_" + kind] = timed(enc, args.steps, args.warmup)
        res["batch_decode_" + kind] = timed(dec, args.steps, args.warmup)
        assert all(np.array_equal(b.reshape(H, W), px[i]) for i, b in enumerate(back))
        res["compressed_bytes"] = int(sum(f.size for f in files["pica"]))
        res["gradient_strips"] = int(sum(int.from_bytes(f[16 + 16 * s + 12: 32 + 16 * s].tobytes(), "little") for f in files["pica"] for s in range(STRIPS)))
        res["pics_encode_" + kind] = timed(pics_enc, args.steps, args.warmup)
        res["pics_decode_" + kind] = timed(pics_dec, args.steps, args.warmup)
        res["pics_compressed_bytes"] = int(sum(f.size for f in files["pics"]))
        if pinned:
            for b in [src] + outs + back:
                mic.host_free(b)
    print(json.dumps(res))


def child_kernels(args):
    """per-kernel device times of one PICA batch call each way: MIC_HIP_LIB is a -DMIC_PICA_TIMING build, which prints them on stderr"""
    import __graft_entry__ as entry
    px = frames(args.images)
    mic = entry.load_package()
    n = args.images
    imgs = [px[i] for i in range(n)]
    for _ in range(2):                                                       # (the second call's lines are the warm ones: the parent keeps the last)
        sys.stderr.write("[mic_hip pica mark]\n"); sys.stderr.flush()
        r = mic.compress_parallel_strips_adaptive_batch(imgs, MAXV, STRIPS)
        out = mic.decompress_parallel_strips_adaptive_batch([b for _, b in r], [(W, H)] * n)
        assert all(st == 0 for st, _ in out) and all(np.array_equal(o, px[i]) for i, (_, o) in enumerate(out))
    print(json.dumps({"compressed_bytes": int(sum(b.size for _, b in r))}))


def child_session(args):
    """both predictors over the same strips (96 frames cut at equal heights, 768 units), device-resident, session timing on:
    the encode chains and -- what decides about k_dec_predict_grad -- the decode chains.  MIC_HIP_LIB picks the build."""
    import torch
    import __graft_entry__ as entry
    m = min(args.images, 96)
    px = frames(m)
    mic = entry.load_package()
    d_px = torch.from_numpy(px.astype(np.int16)).to("cuda:0")
    sh = H // STRIPS
    res = {}
    s = mic.Session(m * STRIPS, W * sh)
    for name, flag in (("avg", 0), ("grad", 0x200)):
        units = mic.Session.make_units([((i * H + k * sh) * W, W, sh, MAXV, 2 | flag) for i in range(m) for k in range(STRIPS)])
        enc_runs, dec_runs = [], []
        for rep in range(2 + args.steps):
            s.set_timing(True)
            s.encode_enqueue(d_px.data_ptr(), units)
            d_blobs, offs, st, _ = s.encode_finish()
            enc_runs.append(dict(s.last_timings()))
            assert (np.asarray(st) == 0).all()
            total = int(offs[-1])
            d_copy = torch.empty(total + 64, dtype=torch.uint8, device="cuda:0")
            mic.device_copy(d_copy.data_ptr(), d_blobs, total)
            d_out = torch.empty_like(d_px)
            s.decode_enqueue(d_copy.data_ptr(), np.asarray(offs, dtype=np.uint64), units, d_out.data_ptr())
            st = s.decode_finish()
            dec_runs.append(dict(s.last_timings()))
            assert (np.asarray(st) == 0).all() and torch.equal(d_out, d_px)
        for what, runs in (("encode", enc_runs[2:]), ("decode", dec_runs[2:])):        # min and median per kernel over the steps
            res["session_%s_%s" % (what, name)] = {k: {"min_ms": round(min(r[k] for r in runs), 4), "median_ms": round(statistics.median(r[k] for r in runs), 4)}
                                                   for k in runs[0] if max(r[k] for r in runs) >= 0.05}
    res["session_units"] = m * STRIPS
    print(json.dumps(res))


def run_child(mode, args, lib=None, env=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--images", str(args.images), "--steps", str(args.steps), "--warmup", str(args.warmup)]
    if lib:
        cmd += ["--lib", lib]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout, env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        raise SystemExit(f"child {mode} failed ({r.returncode}):\n{r.stdout}\n{r.stderr[-4000:]}")
    print(f"[bench_pica_batch] {mode}{' ' + lib if lib else ''} done", file=sys.stderr, flush=True)
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=288)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of libmic_hip.so to loop over (the parent commit's)")
    ap.add_argument("--timing-lib", default=None, help="this tree built with EXTRA_FLAGS=-DMIC_PICA_TIMING: per-kernel times of the batch call")
    ap.add_argument("--nopick-lib", default=None, help="... with -DMIC_PICA_TIMING -DMIC_PICA_NO_PICK: both candidates packed, the host picks")
    ap.add_argument("--session-libs", default="", help="name=path,...: builds whose session chains are timed beside this tree's (parent, variants)")
    ap.add_argument("--reuse-rounds", nargs="*", default=[], help="earlier outputs of this tool whose rounds are taken over (tagged with their file name)")
    ap.add_argument("--child", default=None)
    ap.add_argument("--child-timeout", type=int, default=900)
    args = ap.parse_args()
    if args.child:
        return {"loop": child_loop, "batch": child_batch, "kernels": child_kernels, "session": child_session}[args.child](args)
    raw = W * H * 2 * args.images
    out = {"images": args.images, "shape": [W, H], "strips": STRIPS, "raw_bytes": raw, "steps": args.steps, "warmup": args.warmup, "rounds": []}
    for f in args.reuse_rounds:
        for r in json.load(open(f))["rounds"]:
            out["rounds"].append(dict(r, run=r.get("run", os.path.basename(f))))
    for _ in range(args.rounds):
        rnd = {"run": "this"}
        if args.lib:
            rnd["parent_loop"], _ = run_child("loop", args, lib=args.lib)
        rnd["new_loop"], _ = run_child("loop", args)
        rnd["new_batch"], _ = run_child("batch", args)
        out["rounds"].append(rnd)
    def best(side, key):
        mins = [r[side][key]["min_ms"] for r in out["rounds"] if side in r and key in r[side]]
        meds = [r[side][key]["median_ms"] for r in out["rounds"] if side in r and key in r[side]]
        return {"min_ms": min(mins), "max_of_mins_ms": max(mins), "median_of_medians_ms": statistics.median(meds), "gbps_at_min": round(raw / min(mins) / 1e6, 2)} if mins else None
    out["summary"] = {side + "." + key: best(side, key) for side in ("parent_loop", "new_loop", "new_batch")
                      for key in sorted({k for r in out["rounds"] if side in r for k in r[side] if isinstance(r[side][k], dict)})}
    if out["rounds"]:
        b = out["rounds"][-1]["new_batch"]
        out["ratio"] = round(raw / b["compressed_bytes"], 4); out["pics_ratio"] = round(raw / b["pics_compressed_bytes"], 4)
        out["gradient_strips"] = b["gradient_strips"]
    for tag, lib in (("pick", args.timing_lib), ("no_pick", args.nopick_lib)):        # the pack with and without k_pica_pick, same frames
        if not lib:
            continue
        _, err = run_child("kernels", args, env={"MIC_HIP_LIB": os.path.abspath(lib)})
        last = err.rsplit("[mic_hip pica mark]", 1)[-1]
        for what in ("encode", "decode"):
            out["batch_kernels_%s_%s_ms" % (what, tag)] = {m.group(2): float(m.group(1)) for m in re.finditer(r"\[mic_hip pica %s\]\s+([0-9.]+) ms\s+(.+)" % what, last)}
    out["session"] = {"this": run_child("session", args)[0]}
    for item in filter(None, args.session_libs.split(",")):
        name, path = item.split("=", 1)
        out["session"][name], _ = run_child("session", args, env={"MIC_HIP_LIB": os.path.abspath(path)})   # (a build of THIS ABI: the package loads it)
    out["note"] = ("rounds alternate parent loop / new loop / new batch, one process each; min and median of --steps after --warmup. "
                   "session: per-kernel min / median over the steps, kernels below 0.05 ms left out")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
