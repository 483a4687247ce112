"""Token stream of the library's tokeniser against the oracle's, case by case of tests/tokeniser_streams.py (or of one group named
on the command line): first mismatch and where it lies, the route counters against the model's."""
import ctypes as C, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry
import torch
mic = entry.load_package()
from oracle import mico
import tokeniser_paths as M, tokeniser_streams as S
L = mic.lib()
L.mic_hip_debug_fetch_tok.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
L.mic_hip_debug_tok_paths.argtypes = [C.c_void_p, C.c_int, C.c_void_p]

def check(cs):
    h, w = cs.img.shape
    d_px = torch.from_numpy(np.ascontiguousarray(cs.img).view(np.int16)).cuda()
    sess = mic.Session(1, w * h)
    cu = mic.Session.make_units([(0, w, h, cs.maxv, 2 | (mic.MIC_HIP_PRED_GRAD if cs.pred else 0))])
    sess.encode_enqueue(d_px.data_ptr(), cu); d_blobs, offs, st, used = sess.encode_finish()
    buf = (C.c_uint32 * 32)(); L.mic_hip_debug_unit(sess._h, 0, buf)
    ntok = buf[0]
    want = (mico.grad_delta_rle_compress if cs.pred else mico.delta_rle_compress)(cs.img, cs.maxv)
    got = np.empty(max(ntok, 1), dtype=np.uint16)
    L.mic_hip_debug_fetch_tok(sess._h, 0, got.ctypes.data, ntok)
    paths = (C.c_uint32 * len(M.NAMES))(); L.mic_hip_debug_tok_paths(sess._h, 0, paths)
    m = min(len(want), ntok)
    bad = np.nonzero(got[:m] != want[:m])[0]
    model, trace = S.model(cs)
    print(f"{cs.name}: {w}x{h} maxv {cs.maxv} status {st} ntok gpu {ntok} oracle {len(want)} mismatches {len(bad)}", "first", bad[:8] if len(bad) else None)
    if len(bad):
        i = int(bad[0])
        print("   gpu ", got[max(0, i - 6): i + 10]); print("   want", want[max(0, i - 6): i + 10])
    if dict(zip(M.NAMES, paths)) != model:
        print("   routes gpu  ", list(paths)); print("   routes model", [model[n] for n in M.NAMES], [(t[0], t[2], t[4]) for t in trace])
    sess.close()

for name in (sys.argv[1:] or S.GROUPS):
    for cs in S.group(name):
        check(cs)
