#!/usr/bin/env python3
"""Times the conversion of a dataset of MIC2 volumes, both directions and both pipelines, four ways:
  (a) loop    : compress_multi_frame / decompress_multi_frame, one call per volume (the code as it was: the yardstick);
  (b) batch   : one compress_multi_frame_batch / decompress_multi_frame_batch over pageable host buffers;
  (c) pinned  : the same over buffers from host_alloc, which are sent in place;
  (d) session : Session.mic2_encode from volumes in device memory, Session.mic2_decode from the files it left there.
Workloads: "cine" -- 64 volumes of 32 frames of 256 x 256 --, and "stack" -- 16 volumes of 128 frames of 512 x 512, the crop bench's
shape --, 12 bits, rolled XR-like images with a seed per volume.  Every way must give the loop's bytes and pixels, and the batch's
`slabs` must be what mic2_batch_plan says.  The guard: ONE volume through the batch door against the same volume through the single
call, alternating, with the spread of the single call.  Minimum, median and maximum of --runs runs after a warm-up; every call ends
with the device idle.  Writes profiles/mic2_batch.json (--out)."""
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

WORKLOADS = {"cine": (64, 32, 256), "stack": (16, 128, 512)}


def stats_of(ts):
    return dict(min_ms=round(min(ts), 3), median_ms=round(statistics.median(ts), 3), max_ms=round(max(ts), 3))


def timed(fns, runs, sync):
    """the functions one after the other, `runs` times over, after one warm-up round: {name: stats}"""
    ts = {k: [] for k in fns}
    for r in range(runs + 1):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            sync()
            if r:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats_of(v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mic2_batch.json"))
    a = ap.parse_args()
    import torch
    mic = entry.load_package()
    synth = importlib.import_module("medical_image_codec_amd.synth")
    sync = torch.cuda.synchronize
    result = dict(device=mic.device_name(), runs=a.runs, workloads={})
    for name in a.workloads:
        nv, n, size = WORKLOADS[name]
        vols = []
        for v in range(nv):
            img = synth.xr_like(cols=size, rows=size, depth=12, seed=100 + v)
            vols.append(np.stack([np.roll(img, 3 * k, axis=1) for k in range(n)]))
        cuts, nunits = mic.mic2_batch_plan([(size, size, n)] * nv)
        res = dict(volumes=nv, volume=[n, size, size], raw_bytes=int(sum(v.nbytes for v in vols)), planned_slabs=len(cuts) - 1)
        pin_px = [mic.host_alloc(v.nbytes, dtype=np.uint16) for v in vols]
        pin_out = [mic.host_alloc(v.nbytes) for v in vols]                 # (a file of this content is smaller than its pixels)
        for p, v in zip(pin_px, vols):
            p[:] = v.reshape(-1)
        pin_vols = [p.reshape(v.shape) for p, v in zip(pin_px, vols)]
        d_px = torch.from_numpy(np.concatenate([v.reshape(-1) for v in vols]).view(np.int16)).cuda()
        for temporal in (False, True):
            kind = "temporal" if temporal else "independent"
            keep = {}
            desc = [(i * n * size * size, size, size, n, 4095, temporal) for i in range(nv)]
            sess = mic.Session(8, size * size)

            def enc_loop():
                keep["loop"] = [mic.compress_multi_frame(v, size, size, 4095, temporal=temporal) for v in vols]

            def enc_batch():
                keep["batch"] = mic.compress_multi_frame_batch(vols, 4095, temporal)

            def enc_pinned():
                keep["pinned"] = mic.compress_multi_frame_batch(pin_vols, 4095, temporal, outs=pin_out)

            def enc_session():
                keep["session"] = sess.mic2_encode(d_px.data_ptr(), desc)
            r = dict(encode=timed(dict(loop=enc_loop, batch=enc_batch, pinned=enc_pinned, session=enc_session), a.runs, sync))
            files = keep["loop"]
            assert [f for _, _, f in keep["batch"][0]] == files and [f for _, _, f in keep["pinned"][0]] == files, "the batch's files differ"
            d_files, offs, heads, st, _, sstats = keep["session"]
            t = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda")
            mic.device_copy(t.data_ptr(), d_files, int(offs[-1]))
            assert (st == 0).all() and t.cpu().numpy().tobytes() == b"".join(files), "the session's files differ"
            assert keep["batch"][1]["slabs"] == keep["pinned"][1]["slabs"] == sstats["slabs"] == len(cuts) - 1, (keep["batch"][1], sstats, cuts)
            ptrs, lens = [t.data_ptr() + int(o) for o in offs[:-1]], [len(f) for f in files]
            d_back = torch.empty_like(d_px)
            px_off = [d[0] for d in desc]

            def dec_loop():
                keep["dloop"] = [mic.decompress_multi_frame(f) for f in files]

            def dec_batch():
                keep["dbatch"] = mic.decompress_multi_frame_batch(files)

            def dec_pinned():
                keep["dpinned"] = mic.decompress_multi_frame_batch(files, outs=pin_px)

            def dec_session():
                keep["dsession"] = sess.mic2_decode(heads, ptrs, lens, d_back.data_ptr(), px_off, d_px.numel())
            r["decode"] = timed(dict(loop=dec_loop, batch=dec_batch, pinned=dec_pinned, session=dec_session), a.runs, sync)
            for v, got, (st, _, _, px) in zip(vols, keep["dloop"], keep["dbatch"][0]):
                assert st == 0 and np.array_equal(got, v) and np.array_equal(px, v), "the batch's pixels differ"
            assert all(np.array_equal(p.reshape(v.shape), v) for p, v in zip(pin_px, vols)) and torch.equal(d_back, d_px)
            assert keep["dbatch"][1]["slabs"] == keep["dsession"][2]["slabs"] == len(cuts) - 1
            r["file_bytes"] = int(sum(lens))
            r["batch_slabs"] = int(keep["batch"][1]["slabs"])
            for way in ("batch", "pinned", "session"):
                r[f"encode_loop_over_{way}_min"] = round(r["encode"]["loop"]["min_ms"] / r["encode"][way]["min_ms"], 2)
                r[f"decode_loop_over_{way}_min"] = round(r["decode"]["loop"]["min_ms"] / r["decode"][way]["min_ms"], 2)
            # the guard: one volume through the batch door costs no more than through the single call, within the single call's spread
            # (where a difference goes: the same volume from pinned buffers -- no staging copies --, and from device memory -- no transfers)
            one, f1 = vols[0], files[0]
            g = timed(dict(enc_single=lambda: mic.compress_multi_frame(one, size, size, 4095, temporal=temporal),
                           enc_batch_of_one=lambda: mic.compress_multi_frame_batch([one], 4095, temporal),
                           enc_batch_of_one_pinned=lambda: mic.compress_multi_frame_batch(pin_vols[:1], 4095, temporal, outs=pin_out[:1]),
                           enc_session_of_one=lambda: sess.mic2_encode(d_px.data_ptr(), desc[:1], heads=False),
                           dec_single=lambda: mic.decompress_multi_frame(f1),
                           dec_batch_of_one=lambda: mic.decompress_multi_frame_batch([f1]),
                           dec_batch_of_one_pinned=lambda: mic.decompress_multi_frame_batch([f1], outs=pin_px[:1]),
                           dec_session_of_one=lambda: sess.mic2_decode(heads[:1], ptrs[:1], lens[:1], d_back.data_ptr(), px_off[:1], d_px.numel())),
                      max(a.runs, 9), sync)
            for d in ("enc", "dec"):
                s, b = g[f"{d}_single"], g[f"{d}_batch_of_one"]
                g[f"{d}_guard"] = dict(single_min_ms=s["min_ms"], batch_min_ms=b["min_ms"], single_spread_ms=round(s["max_ms"] - s["min_ms"], 3),
                                       holds=bool(b["min_ms"] <= s["min_ms"] + (s["max_ms"] - s["min_ms"])))
            r["one_volume"] = g
            sess.set_timing(2)
            enc_session(); sync()
            r["session_encode_kernels_ms"] = {k: round(v, 3) for k, v in sess.last_timings()}
            sess.set_timing(0)
            sess.close()
            res[kind] = r
            print(name, kind, json.dumps({k: r[k] for k in ("encode", "decode", "batch_slabs")}), flush=True)
            print(name, kind, "one volume", json.dumps({k: g[k] for k in ("enc_guard", "dec_guard")}), flush=True)
        for p in pin_px + pin_out:
            mic.host_free(p)
        result["workloads"][name] = res
    print(json.dumps(result))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
