"""Timing of the decode kernels on the bench workload, ignoring decode status (for ablation builds whose output is wrong).
usage: python tools/time_dec.py [frames] [nstates] [noise] [min_tokens4] [min_tokens8]   (noise: a number, or "published" for the
headline's level -- the streams the split instances take; default: xr_like's own.  min_tokens4: the session's four-part threshold;
one above the strips' length, 1000000 say, sends every headline strip to the two-part instance, mark k_dec_tans_ls_split<13>.
min_tokens8: the eight-part threshold; 1000000 keeps the headline strips with the four-part instance, mark k_dec_tans_ls_split4<13>,
the default sends them to the eight-part one, mark k_dec_tans_ls_split8<13>.  0 keeps a value)"""
import ctypes, os, sys, importlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry
import torch
mic = entry.load_package()
synth = importlib.import_module("medical_image_codec_amd.synth")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 288
NS = int(sys.argv[2]) if len(sys.argv) > 2 else 2
W, H, S = 2577, 2048, 8
NOISE = {} if len(sys.argv) <= 3 else {"noise": synth.XR_NOISE_PUBLISHED_RATIO if sys.argv[3] == "published" else float(sys.argv[3])}
base = [synth.xr_like(cols=W, rows=H, depth=12, seed=1 + i, **NOISE) for i in range(4)]
host = np.stack([base[i % 4] for i in range(B)])
d_px = torch.from_numpy(host.view(np.int16)).cuda()
d_out = torch.empty_like(d_px)
sh = (H + S - 1) // S
units = [(b * W * H + y0 * W, W, min(H, y0 + sh) - y0, 4095, NS) for b in range(B) for y0 in range(0, H, sh)]
sess = mic.Session(len(units), W * sh)
if len(sys.argv) > 4:
    assert mic.lib().mic_hip_debug_split4_config(sess._h, ctypes.c_uint32(int(sys.argv[4]))) == 0
if len(sys.argv) > 5:
    assert mic.lib().mic_hip_debug_split8_config(sess._h, ctypes.c_uint32(int(sys.argv[5]))) == 0
cu = mic.Session.make_units(units)
sess.encode_enqueue(d_px.data_ptr(), cu)
d_blobs, offs, st, ns = sess.encode_finish()
print("encode ok", (st == 0).all(), "ratio", host.nbytes / int(offs[-1]))
for it in range(3):
    sess.set_timing(True)
    sess.decode_enqueue(d_blobs, offs, cu, d_out.data_ptr())
    t = sess.last_timings()
    dst = sess.decode_finish()
    if it == 2:
        print("decode status ok:", int((dst == 0).sum()), "of", len(units), " equal:", bool(torch.equal(d_out, d_px)))
        print({k: round(v, 3) for k, v in t if v > 0.03})

import ctypes as C
L = mic.lib()
out = (C.c_uint32 * 32)()
L.mic_hip_debug_unit.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]
for i in (0, 9, 900):
    L.mic_hip_debug_unit(sess._h, i, out)
    d = [out[16 + k] * 16 for k in range(5)]
    if out[16 + 6] and out[16 + 11]:                                    # the partner instance: the chain wave's phases, and the partner wave's own period beside them
        n, m = out[16 + 5], out[16 + 11]
        p = [out[16 + 8 + k] * 16 for k in range(3)]
        print("unit", i, "%d parts, chain wave, cycles per chunk: rounds %.0f  publish %.0f  handshake wait %.0f  loop test %.0f  sum %.0f  (chunks %d)"
              % (out[16 + 6], d[0] / n, d[1] / n, d[2] / n, d[4] / n, sum(d) / n, n))
        print("unit", i, "         partner wave, cycles per chunk: waiting for the chunk %.0f  positions, stage, ring fills, served, loads %.0f  state stores %.0f  "
              "busy %.0f of %.0f  (chunks %d)" % (p[0] / m, p[1] / m, p[2] / m, (p[1] + p[2]) / m, sum(p) / m, m))
    elif out[16 + 6]:                                                   # a split instance's stamps: five phases, chunks, parts per stream
        n = out[16 + 5]
        print("unit", i, "%d parts, cycles per chunk: rounds %.0f  ring stores %.0f  loads %.0f  state stores %.0f  hand-over/snapshot/ballot %.0f  "
              "sum %.0f  (chunks %d)" % tuple([out[16 + 6]] + [d[k] / n for k in range(5)] + [sum(d) / n, n]))
    elif d[4]:
        print("unit", i, "cycles per chunk: rounds %.0f  ring stores %.0f  loads %.0f  state stores %.0f  (chunks %d)" % tuple([d[k] / (d[4] / 16) for k in range(4)] + [d[4] // 16]))
