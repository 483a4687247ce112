"""Diagnostic: what the split instances of the two-state tANS chain (k_dec_tans_ls_parts<8>, <4> and <2>) make of the headline
step's strips -- per step the count of units by the instance whose record they carry and MicUnit.split outcome (not tried / split /
handed back and why, for four- and eight-part records with the boundary that failed), and the spread of the first join.  Of the
eight-part instance's partner waves (MicUnit.partner): the units that stalled (MIC_SPLIT_STALLED: a chain wave and its partner gave
each other up) and the chunks a chain wave found its partner not ready for, against the chunks the partners served.  A unit the
eight-part instance hands back carries the four-part instance's record: with every headline strip on the eight-part list, any
four-part record is such a unit.
usage: tools/split_outcomes.py [frames=288] [steps=20]"""
import ctypes as C, os, sys, importlib, collections
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry
import torch
mic = entry.load_package()
synth = importlib.import_module("medical_image_codec_amd.synth")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 288
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
W, H, S = 2577, 2048, 8
NAMES = {0: "not tried", 1: "split", 2: "handed back: no meeting", 3: "handed back: count", 4: "handed back: no room", 5: "handed back: stalled"}
L = mic.lib()
L.mic_hip_debug_split4.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
L.mic_hip_debug_split8.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
L.mic_hip_debug_partner.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
SPW = 3                                                                 # units of a chain wave: they share its not-ready count
sh = (H + S - 1) // S
units = mic.Session.make_units([(b * W * H + y0 * W, W, min(H, y0 + sh) - y0, 4095, 2) for b in range(B) for y0 in range(0, H, sh)])
sess = mic.Session(B * S, W * sh)
total = collections.Counter()
stalled = not_ready = served = 0


def name(key):
    parts, outcome, fail = key
    if not outcome:
        return NAMES[0]
    return f"{parts} parts {NAMES[outcome]}" + (f" at boundary {fail}" if fail else "")


for step in range(STEPS):
    d_px = synth.xr_like_batch_torch(B, cols=W, rows=H, depth=12, seed0=1 + 1000 * step, noise=synth.XR_NOISE_PUBLISHED_RATIO, device=torch.device("cuda:0"))
    d_out = torch.empty_like(d_px)
    sess.encode_enqueue(d_px.data_ptr(), units); d_blobs, offs, st, ns = sess.encode_finish()
    sess.decode_enqueue(d_blobs, offs, units, d_out.data_ptr()); dst = sess.decode_finish()
    assert (st == 0).all() and (dst == 0).all() and torch.equal(d_out, d_px)
    seen, first = collections.Counter(), []
    for i in range(B * S):
        out = (C.c_uint32 * 8)()                                        # outcome, I_1, I_2, I_3, W, R (0: a two-part unit), failing boundary
        assert L.mic_hip_debug_split4(sess._h, i, out) == 0
        o8 = (C.c_uint32 * 12)()                                        # outcome, I_1 .. I_7, W, R (0: not an eight-part record), failing boundary, parts
        assert L.mic_hip_debug_split8(sess._h, i, o8) == 0
        four, eight = out[5] != 0, o8[9] != 0
        pr = (C.c_uint32 * 4)()                                         # who did the upkeep, chunks served, not-ready chunks of the wave, stalled
        assert L.mic_hip_debug_partner(sess._h, i, pr) == 0
        stalled += int(pr[3]); served += int(pr[1])
        if i % SPW == 0: not_ready += int(pr[2])                        # (every strip is on the eight-part list, in unit order: unit 3 w is wave w's first)
        seen[(8 if eight else 4 if four else 2, int(out[0]), int(o8[10]) if eight else int(out[6]))] += 1
        if out[0] == 1: first.append(int(o8[1]) if eight else int(out[1]) if four else None)
    first = [v for v in first if v is not None]
    total += seen
    print(f"step {step}: " + ", ".join(f"{name(k)} {v}" for k, v in sorted(seen.items())) +
          (f"; I_1 {min(first)} .. {max(first)}" if first else ""), flush=True)
print("all steps: " + ", ".join(f"{name(k)} {v}" for k, v in sorted(total.items())))
print("handed back: %d of %d" % (sum(v for k, v in total.items() if k[1] >= 2), sum(total.values())))
print("four-part records (the eight-part instance's hand-backs when min_tokens8 is below every strip): %d" % sum(v for k, v in total.items() if k[0] == 4))
print("partner waves: %d units stalled; chain waves found their partner not ready for %d chunks; %d chunks served (per unit)" % (stalled, not_ready, served))
