#!/usr/bin/env python3
"""The MIC2 frame cache against the tree without it and against the parent commit.  The README's MIC2 workload -- 64 random
128 x 128 x 64 crops of a 256-frame 512 x 512 12-bit stack, an independent and a temporal file, through a Mic2Reader -- and the
multi workload: one crop from each of 16 volumes of 128 frames through mic2_readers_read_crops, the readers sharing one cache.
Min and max of --runs calls after a warm-up, wall time around the call and a device synchronise, FRESH origins every call:
  parent      the parent commit's library, loaded in this process (--parent-lib), its reader door
  no_cache    this tree's reader with no cache attached
  cold        an empty cache that holds the volume (cleared in front of every call; the arena is allocated by the warm-up)
  warm        the cache holds the whole volume: the call must report frames_decoded == 0
  half        a cache of half the volume's frames, in steady state
  anchored    (temporal) frames 0 .. 127 resident, every crop in frames 128 .. 255
Beside them a device-to-device copy of the frames a cold independent call fills, and the session timer's entries of a cold call
(mic_hip_mic2_reader_set_timing): k_mic2_accumulate_frames against its traffic bound 2 B x pixels x (residuals + stores + 1) at the
copy's measured rate.  The two checks the feature is held to are computed and recorded, not tuned: the uncached door within the
parent's own max - min spread, and the cold independent call within the uncached call plus twice the copy.

    python tools/bench_mic2_frame_cache.py --parent-lib build_variants/parent/libmic_hip.so [--out profiles/mic2_frame_cache.json]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry


def spread(ts):
    return dict(min_ms=round(min(ts), 3), max_ms=round(max(ts), 3), runs_ms=[round(t, 3) for t in ts])


def timed(fn, runs, sync, before=None, warm=1):
    """fn(k) for call k, before(k) untimed in front of it; the first `warm` calls are not counted"""
    ts = []
    for k in range(warm + runs):
        if before:
            before(k); sync()
        t0 = time.perf_counter()
        fn(k); sync()
        if k >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts)


class ParentReader:
    """mic_hip_mic2_reader_* of another build of the library, by ctypes alone"""

    def __init__(self, L, mic, data):
        self.L, self.data = L, bytes(data)

        def read(user, off, ptr, n):
            C.memmove(ptr, self.data[off: off + n], n)
            return 0
        self.cb = mic._READ_FN(read)
        self.h = C.c_void_p()
        L.mic_hip_mic2_reader_open.argtypes = [mic._READ_FN, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
        L.mic_hip_mic2_reader_read_crops.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.mic_hip_mic2_readers_read_crops.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mic_hip_mic2_reader_close.argtypes = [C.c_void_p]
        L.mic_hip_mic2_reader_close.restype = None
        assert L.mic_hip_mic2_reader_open(self.cb, None, len(self.data), C.byref(self.h)) == 0

    def read_crops(self, xyz, cw, ch, cd, d_out, cap):
        a = np.ascontiguousarray(np.asarray(xyz, dtype=np.int32).reshape(-1, 3))
        st = np.zeros(len(a), dtype=np.int32)
        assert self.L.mic_hip_mic2_reader_read_crops(self.h, a.ctypes.data, len(a), cw, ch, cd, d_out, cap, st.ctypes.data, None) == 0 and (st == 0).all()

    def close(self):
        self.L.mic_hip_mic2_reader_close(self.h)


def parent_readers_call(L, readers, xyzv, cw, ch, cd, d_out, cap):
    hs = np.asarray([r.h.value for r in readers], dtype=np.uintp)
    a = np.ascontiguousarray(np.asarray(xyzv, dtype=np.int32).reshape(-1, 4))
    st = np.zeros(len(a), dtype=np.int32)
    assert L.mic_hip_mic2_readers_read_crops(hs.ctypes.data, len(readers), a.ctypes.data, len(a), cw, ch, cd, d_out, cap, st.ctypes.data, None, None) == 0 and (st == 0).all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libmic_hip.so of the parent commit, built in a directory of its own")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--crops", type=int, default=64)
    ap.add_argument("--crop", type=int, nargs=3, default=[128, 128, 64], metavar=("CW", "CH", "CD"))
    ap.add_argument("--volumes", type=int, default=16)
    ap.add_argument("--volume-frames", type=int, default=128)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mic2_frame_cache.json"))
    a = ap.parse_args()
    import torch
    mic = entry.load_package()
    synth = importlib.import_module("medical_image_codec_amd.synth")
    PL = C.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    sync = torch.cuda.synchronize
    n, w, h = a.frames, a.size, a.size
    cw, ch, cd = a.crop
    npx = w * h
    rec = dict(device=mic.device_name(), volume=[n, h, w], crops=a.crops, crop=[cw, ch, cd], runs=a.runs, parent_lib=bool(PL), files={})
    img = synth.xr_like(cols=w, rows=h, depth=12, seed=3)
    vol = np.stack([np.roll(img, 3 * k, axis=1) for k in range(n)])
    rng = np.random.default_rng(7)

    def origins(z0, z1):
        return np.stack([rng.integers(0, w - cw + 1, a.crops), rng.integers(0, h - ch + 1, a.crops), rng.integers(z0, z1 + 1, a.crops)], axis=1).astype(np.int32)
    lists = [origins(0, n - cd) for _ in range(a.runs + 4)]
    upper = [origins(n // 2, n - cd) for _ in range(a.runs + 4)]
    cover = np.asarray([(0, 0, z) for z in range(0, n, cd)], dtype=np.int32)             # names every frame
    t = torch.empty((a.crops, cd, ch, cw), dtype=torch.int16, device="cuda")
    cap = t.numel() * 2

    def check(xyz):
        got = t.cpu().numpy().view(np.uint16)
        for i in (0, len(xyz) // 2, len(xyz) - 1):
            x, y, z = (int(v) for v in xyz[i])
            assert np.array_equal(got[i], vol[z: z + cd, y: y + ch, x: x + cw])

    # the device-to-device copy a fill is measured against: K frames read and written once
    def copy_ms(frames):
        src = torch.empty(frames * npx, dtype=torch.int16, device="cuda")
        dst = torch.empty_like(src)
        ts = timed(lambda k: dst.copy_(src), a.runs, sync)
        return ts["min_ms"]

    for temporal in (False, True):
        data = mic.compress_multi_frame(vol, w, h, 4095, temporal=temporal)
        r = dict(file_bytes=len(data))
        keep = {}
        if PL:
            prd = ParentReader(PL, mic, data)
            r["parent"] = timed(lambda k: prd.read_crops(lists[k], cw, ch, cd, t.data_ptr(), cap), a.runs, sync)
            check(lists[a.runs])
            prd.close()
        rd = mic.Mic2Reader(data)

        def call(k, ls=lists):
            keep["st"], keep["stats"] = rd.read_crops(ls[k], cw, ch, cd, t.data_ptr(), cap)
            assert (keep["st"] == 0).all()
        r["no_cache"] = timed(call, a.runs, sync)
        check(lists[a.runs])
        r["no_cache_stats"] = dict(keep["stats"])
        full = mic.FrameCache(w, h, n)
        rd.set_cache(full)
        r["cold"] = timed(call, a.runs, sync, before=lambda k: full.clear())
        check(lists[a.runs])
        r["cold_stats"] = dict(keep["stats"])
        filled = int(rd.cache_probe(np.arange(n)).sum())                                 # frames the last cold call kept
        r["cold_frames_filled"] = filled
        r["copy_of_filled_frames_ms"] = copy_ms(filled)
        rd.set_timing(True)
        full.clear()
        call(0); sync()
        r["cold_kernels_ms"] = {k: round(v, 4) for k, v in rd.last_timings()}
        r["cold_timed_stats"] = dict(keep["stats"])
        rd.set_timing(False)
        if temporal:
            # the frame kernel's traffic: every decoded residual read once, every named frame stored once, the anchor read once
            named = len(np.unique(np.concatenate([np.arange(z, z + cd) for z in lists[0][:, 2]])))
            units = int(keep["stats"]["frames_decoded"])
            traffic = 2 * npx * ((units - 1) + named + 1)
            rate = 2 * 2 * filled * npx / (r["copy_of_filled_frames_ms"] * 1e-3)         # bytes read + written per second by the copy
            r["accumulate_frames"] = dict(residuals=units - 1, stores=named, traffic_bytes=traffic, copy_rate_GBps=round(rate / 1e9, 1),
                                          bound_ms=round(traffic / rate * 1e3, 4), measured_ms=r["cold_kernels_ms"].get("k_mic2_accumulate_frames"))
        # warm: the whole volume resident
        full.clear()
        for q in range(0, len(cover), 4):
            rd.read_crops(cover[q: q + 4], 8, 8, cd, t.data_ptr(), cap)
        assert rd.cache_probe(np.arange(n)).all()

        def warm_call(k):
            call(k)
            assert keep["stats"]["frames_decoded"] == 0 and keep["stats"]["slabs"] == 0, keep["stats"]
        r["warm"] = timed(warm_call, a.runs, sync)
        check(lists[a.runs])
        if temporal:
            def half_resident(k):
                full.clear()
                for q in range(0, len(cover) // 2, 4):
                    rd.read_crops(cover[q: min(q + 4, len(cover) // 2)], 8, 8, cd, t.data_ptr(), cap)
            r["anchored"] = timed(lambda k: call(k, upper), a.runs, sync, before=half_resident)
            check(upper[a.runs])
            r["anchored_stats"] = dict(keep["stats"])
        rd.set_cache(None)
        full.close()
        half = mic.FrameCache(w, h, n // 2)
        rd.set_cache(half)
        before = half.stats()
        r["half"] = timed(call, a.runs, sync, warm=3)
        check(lists[a.runs + 2])
        after = half.stats()
        r["half_stats"] = {k: after[k] - before[k] for k in ("hits", "misses", "bypassed", "evictions", "calls")}
        rd.set_cache(None)
        half.close()
        rd.close()
        rec["files"]["temporal" if temporal else "independent"] = r

    # many volumes: one crop from each, the readers sharing a cache that holds them all
    nv, nf = a.volumes, a.volume_frames
    many = {}
    t2 = torch.empty((nv, cd, ch, cw), dtype=torch.int16, device="cuda")
    cap2 = t2.numel() * 2
    vols = []
    for v in range(nv):
        im = synth.xr_like(cols=w, rows=h, depth=12, seed=100 + v)
        vols.append(np.stack([np.roll(im, 3 * k, axis=1) for k in range(nf)]))
    qs = [np.stack([rng.integers(0, w - cw + 1, nv), rng.integers(0, h - ch + 1, nv), rng.integers(0, nf - cd + 1, nv), np.arange(nv)], axis=1).astype(np.int32)
          for _ in range(a.runs + 2)]
    for temporal in (False, True):
        files = [mic.compress_multi_frame(v_, w, h, 4095, temporal=temporal) for v_ in vols]
        m = {}
        keep = {}
        if PL:
            prs = [ParentReader(PL, mic, d) for d in files]
            m["parent"] = timed(lambda k: parent_readers_call(PL, prs, qs[k], cw, ch, cd, t2.data_ptr(), cap2), a.runs, sync)
            for p_ in prs:
                p_.close()
        rds = [mic.Mic2Reader(d) for d in files]

        def mcall(k):
            keep["st"], keep["bad"], keep["stats"] = mic.mic2_readers_read_crops(rds, qs[k], cw, ch, cd, t2.data_ptr(), cap2)
            assert (keep["st"] == 0).all()
        m["no_cache"] = timed(mcall, a.runs, sync)
        cache = mic.FrameCache(w, h, nv * nf)
        for r_ in rds:
            r_.set_cache(cache)
        m["cold"] = timed(mcall, a.runs, sync, before=lambda k: cache.clear())
        m["cold_stats"] = dict(keep["stats"])
        m["same_call_again"] = timed(lambda k: mcall(0), a.runs, sync)
        assert keep["stats"]["frames_decoded"] == 0
        got = t2.cpu().numpy().view(np.uint16)
        for i in (0, nv - 1):
            x, y, z, v = (int(c) for c in qs[0][i])
            assert np.array_equal(got[i], vols[v][z: z + cd, y: y + ch, x: x + cw])
        for r_ in rds:
            r_.set_cache(None)
            r_.close()
        cache.close()
        many["temporal" if temporal else "independent"] = m
    rec["many_volumes"] = dict(volumes=nv, frames=nf, **many)

    v = {}
    for kind, r in rec["files"].items():
        e = dict(no_cache_min_ms=r["no_cache"]["min_ms"], cold_min_ms=r["cold"]["min_ms"], warm_min_ms=r["warm"]["min_ms"], half_min_ms=r["half"]["min_ms"],
                 cold_over_no_cache=round(r["cold"]["min_ms"] / r["no_cache"]["min_ms"], 3), no_cache_over_warm=round(r["no_cache"]["min_ms"] / r["warm"]["min_ms"], 1))
        if "parent" in r:
            e.update(parent_min_ms=r["parent"]["min_ms"], parent_spread_ms=round(r["parent"]["max_ms"] - r["parent"]["min_ms"], 3),
                     no_cache_minus_parent_min_ms=round(r["no_cache"]["min_ms"] - r["parent"]["min_ms"], 3))
            e["uncached_within_parent_spread"] = e["no_cache_minus_parent_min_ms"] <= e["parent_spread_ms"]
        if kind == "independent":
            e["cold_allowance_ms"] = round(r["no_cache"]["min_ms"] + 2 * r["copy_of_filled_frames_ms"], 3)
            e["cold_within_allowance"] = r["cold"]["min_ms"] <= e["cold_allowance_ms"]
        else:
            e["anchored_min_ms"] = r["anchored"]["min_ms"]
            acc = r["accumulate_frames"]
            e["accumulate_frames_over_bound"] = round(acc["measured_ms"] / acc["bound_ms"], 2) if acc["measured_ms"] else None
        v[kind] = e
    for kind, m in rec["many_volumes"].items():
        if isinstance(m, dict) and "no_cache" in m:
            e = dict(no_cache_min_ms=m["no_cache"]["min_ms"], cold_min_ms=m["cold"]["min_ms"], same_call_again_min_ms=m["same_call_again"]["min_ms"])
            if "parent" in m:
                e.update(parent_min_ms=m["parent"]["min_ms"], parent_spread_ms=round(m["parent"]["max_ms"] - m["parent"]["min_ms"], 3),
                         no_cache_minus_parent_min_ms=round(m["no_cache"]["min_ms"] - m["parent"]["min_ms"], 3))
            v["many_" + kind] = e
    rec["verdict"] = v
    print(json.dumps(v, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
