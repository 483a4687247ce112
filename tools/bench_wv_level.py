"""WaveletV2 at reduced resolution: ms per batch of the full decode and of the decode at every level r = 1 .. levels, with the kernel
split (Session.set_timing) and the share of the tANS symbols the chain decoded (sum of symbols_decoded / sum of the streams' counts).
256 CR-like frames (1760 x 2140, 12-bit, = synth.cr_like's noise), device-resident through the session, as bench.py's config 3.
usage: python tools/bench_wv_level.py [frames] [levels] [steps]"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
import torch  # noqa: E402

mic = entry.load_package()
synth = importlib.import_module("medical_image_codec_amd.synth")
nf = int(sys.argv[1]) if len(sys.argv) > 1 else 256
levels = int(sys.argv[2]) if len(sys.argv) > 2 else 5
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rows, cols = 2140, 1760
d_px = synth.xr_like_batch_torch(nf, cols=cols, rows=rows, depth=12, seed0=2000, noise=5.0, device="cuda")
sess = mic.Session(nf, 2 * rows * cols + 16)
d_s, offs, st, applied = sess.wavelet_v2_encode(d_px.data_ptr(), nf, rows, cols, levels)
assert (st == 0).all()
packed = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda")     # (the session's stream buffer is reused by its next call)
import ctypes  # noqa: E402
hip = ctypes.CDLL("libamdhip64.so")
assert hip.hipMemcpy(ctypes.c_void_p(packed.data_ptr()), ctypes.c_void_p(d_s), ctypes.c_size_t(int(offs[-1])), 3) == 0
host = packed.cpu().numpy()
count = sum(int.from_bytes(host[int(offs[i]) + 2:int(offs[i]) + 6].tobytes(), "little") for i in range(nf))   # FSE prefix: 0xFF 0x04, u32
print(f"# {nf} frames {cols}x{rows}, {applied} levels, {mic.device_name()}; sum of stream counts {count}")


def run(r):
    nr, nc = rows, cols
    for _ in range(r):
        nr, nc = (nr + 1) // 2, (nc + 1) // 2
    d_out = torch.empty((nf, nr, nc), dtype=torch.int16, device="cuda")

    def one(timing=0):
        sess.set_timing(timing)
        if r == 0:
            s = sess.wavelet_v2_decode(packed.data_ptr(), offs, nf, rows, cols, applied, d_out.data_ptr()); syms = None
        else:
            s, syms = sess.wavelet_v2_decode_level(packed.data_ptr(), offs, nf, rows, cols, applied, r, d_out.data_ptr())
        assert (s == 0).all()
        return syms, sess.last_timings() if timing else []

    one()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        syms, _ = one()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    _, tim = one(2)
    split = {}
    for k, v in tim:
        if v > 0.05:
            split[k] = round(split.get(k, 0.0) + v, 2)
    dec = count if syms is None else int(syms.sum())
    return {"level": r, "band": f"{nc}x{nr}", "ms_median": round(float(np.median(times)) * 1e3, 2), "ms_min": round(min(times) * 1e3, 2),
            "symbols_share": round(dec / count, 5), "kernels_ms": split}


res = [run(r) for r in range(applied + 1)]
for x in res:
    print(json.dumps(x))
full = res[0]["ms_median"]
print("# speed-up over the full decode: " + ", ".join(f"r={x['level']}: {full / x['ms_median']:.1f}x" for x in res[1:]))
sess.close()
