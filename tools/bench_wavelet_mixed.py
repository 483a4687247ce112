"""WaveletV2 frames of mixed shapes in one call against the ways there were before: writes profiles/wavelet_mixed.json.

  1. a mixed directory -- 64 CR-like 2140 x 1760 frames, 64 of 512 x 512, 64 of 256 x 256 and 64 of odd sizes, shuffled, 5 levels -- coded
     and decoded (full size and at level 3) three ways: a loop of single calls; grouped by shape on the host, one
     wavelet_v2_compress_batch / _decompress_batch / _decompress_level_batch per group (the best there was); ONE _jobs call.
  2. one shape through either door: 256 CR frames through wavelet_v2_compress_batch of another build of the library (--parent-lib, the
     commit before) and through wavelet_v2_compress_jobs of this one, alternating in one process.

Every arm is run --runs times (at least five); min, max and mean are kept, and the jobs / grouped ratio with the grouped arm's own
spread beside it.  python tools/bench_wavelet_mixed.py [--runs 5] [--scale 1.0] [--parent-lib PATH] [--out profiles/wavelet_mixed.json]"""
import argparse, ctypes as C, importlib, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry

ODD = [(301, 217), (1023, 769), (77, 1999), (615, 333), (129, 127), (1441, 55), (255, 257), (919, 1201)]


def timed(fn, runs):
    fn()                                                                      # (warm: workspace, staging, tables)
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "ms_mean": round(float(np.mean(ts)), 3), "runs": runs}


def verdict(arms):
    g, j = arms["grouped"], arms["jobs"]
    return {"jobs_over_grouped": round(j["ms_mean"] / g["ms_mean"], 4), "jobs_over_singles": round(j["ms_mean"] / arms["singles"]["ms_mean"], 4),
            "grouped_spread_ms": round(g["ms_max"] - g["ms_min"], 3),
            "jobs_not_slower_than_grouped_beyond_its_spread": bool(j["ms_mean"] <= g["ms_mean"] + (g["ms_max"] - g["ms_min"]))}


def directory(synth, scale):
    per = max(2, int(64 * scale))
    shapes = [(2140, 1760)] * per + [(512, 512)] * per + [(256, 256)] * per + [ODD[k % len(ODD)] for k in range(per)]
    pool = {}
    for sh in set(shapes):                                                    # a few distinct frames per shape, reused
        pool[sh] = [synth.cr_like(cols=sh[1], rows=sh[0], seed=900 + 7 * k + sh[0]) for k in range(4)]
    order = np.random.default_rng(5).permutation(len(shapes))
    return [pool[shapes[i]][i % 4] for i in order]


def by_shape(items, key):
    groups = {}
    for i, it in enumerate(items):
        groups.setdefault(key(it), []).append(i)
    return groups


def mixed_directory(mic, synth, runs, scale):
    frames = directory(synth, scale)
    n = len(frames)
    files = [None] * n
    groups = by_shape(frames, lambda f: f.shape)

    def enc_singles():
        for i, f in enumerate(frames):
            files[i] = mic.wavelet_v2_compress(f, f.shape[0], f.shape[1], 4095, 5)

    def enc_grouped():
        for sh, idx in groups.items():
            for i, (st, b) in zip(idx, mic.wavelet_v2_compress_batch(np.stack([frames[i] for i in idx]), 4095, 5)):
                assert st == 0
                files[i] = b

    stats = {}

    def enc_jobs():
        res, stats["enc"] = mic.wavelet_v2_compress_jobs(frames, 4095, 5)
        for i, (st, b, _) in enumerate(res):
            assert st == 0
            files[i] = b

    out = {"frames": n, "pixels": int(sum(f.size for f in frames)), "shapes": len(groups)}
    enc = {"singles": timed(enc_singles, runs)}
    ref = list(files)
    enc["grouped"] = timed(enc_grouped, runs)
    assert files == ref
    enc["jobs"] = timed(enc_jobs, runs)
    assert files == ref
    out["encode"] = dict(enc, **verdict(enc), stats=stats["enc"])
    for level, name in ((0, "decode"), (3, "decode_level_3")):
        got = [None] * n

        def dec_singles():
            for i, f in enumerate(files):
                got[i] = mic.wavelet_v2_decompress_level(f, level) if level else mic.wavelet_v2_decompress(f)[0]

        def dec_grouped():
            for sh, idx in groups.items():
                fl = [files[i] for i in idx]
                st, px = mic.wavelet_v2_decompress_level_batch(fl, level) if level else mic.wavelet_v2_decompress_batch(fl)
                assert st == [0] * len(idx)
                for k, i in enumerate(idx):
                    got[i] = px[k]

        def dec_jobs():
            res, stats[name] = mic.wavelet_v2_decompress_jobs(files, level)
            for i, (st, img, _) in enumerate(res):
                assert st == 0
                got[i] = img

        dec = {"singles": timed(dec_singles, runs)}
        want = [g.copy() for g in got]
        dec["grouped"] = timed(dec_grouped, runs)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        dec["jobs"] = timed(dec_jobs, runs)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        if level == 0:
            assert all(np.array_equal(a, b) for a, b in zip(got, frames))
        out[name] = dict(dec, **verdict(dec), stats=stats[name])
    return out


def one_shape(mic, synth, runs, scale, parent_lib):
    """256 CR frames: wavelet_v2_compress_batch of the parent's library and wavelet_v2_compress_jobs of this one, alternating"""
    nf, rows, cols = max(4, int(256 * scale)), 2140, 1760
    base = [synth.cr_like(cols=cols, rows=rows, seed=300 + k) for k in range(4)]
    frames = np.stack([base[k % 4] for k in range(nf)])
    stride = rows * cols * 2 + (1 << 20)
    out = np.empty(nf * stride, dtype=np.uint8)
    lens = (C.c_size_t * nf)(); st = (C.c_int32 * nf)()
    outs = [out[i * stride: (i + 1) * stride] for i in range(nf)]
    P = C.CDLL(parent_lib)
    P.mic_hip_wavelet_v2_compress_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint16, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    jobs = (mic.WvEncJob * nf)(*[mic.WvEncJob(frames[i].ctypes.data, rows, cols, 4095, 5, outs[i].ctypes.data, stride, 0, 0, 0) for i in range(nf)])
    bs = mic.WvBatchStats()
    digest = {}

    def parent():
        assert P.mic_hip_wavelet_v2_compress_batch(frames.ctypes.data, nf, rows, cols, 4095, 5, out.ctypes.data, stride, lens, st) == 0
        assert not any(st)
        digest["parent"] = [bytes(outs[i][: lens[i]]) for i in (0, nf // 2, nf - 1)]

    def branch():
        assert mic.lib().mic_hip_wavelet_v2_compress_jobs(jobs, nf, C.byref(bs)) == 0
        assert all(jobs[i].status == 0 for i in range(nf))
        digest["branch"] = [bytes(outs[i][: jobs[i].out_len]) for i in (0, nf // 2, nf - 1)]

    parent(); branch()
    assert digest["parent"] == digest["branch"]
    tp, tb = [], []
    for _ in range(runs):                                                     # alternating: both see the same machine
        t0 = time.perf_counter(); parent(); tp.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); branch(); tb.append((time.perf_counter() - t0) * 1e3)
    arm = lambda ts: {"ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "ms_mean": round(float(np.mean(ts)), 3), "runs": runs}
    return {"frames": nf, "parent_compress_batch": arm(tp), "branch_compress_jobs": arm(tb),
            "branch_over_parent": round(float(np.mean(tb)) / float(np.mean(tp)), 4), "stats": mic._wv_stats(bs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 4 x 64 frames of the directory and of the 256 CR frames")
    ap.add_argument("--parent-lib", default=None, help="libmic_hip.so of the commit before (part 2; left out without it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wavelet_mixed.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("at least five runs per arm")
    mic = entry.load_package()
    synth = importlib.import_module("medical_image_codec_amd.synth")
    res = {"device": mic.device_name(), "runs": args.runs, "scale": args.scale,
           "mixed_directory": mixed_directory(mic, synth, args.runs, args.scale)}
    if args.parent_lib:
        res["one_shape"] = one_shape(mic, synth, args.runs, args.scale, args.parent_lib)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
