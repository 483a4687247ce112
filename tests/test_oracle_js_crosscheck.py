"""Cross-check of everything the oracle writes for which no C reference exists (1-state streams, PICS, MIC2 incl. temporal,
MIC3, MICR, MIC1) against the reference's independent JavaScript decoder (web/mic-decoder.js).  tests/golden/make_golden.py
ran that decoder on every stream of oracle_jobs (through tests/js_crosscheck.mjs), checked that it returned the original
samples, and recorded each stream's size and FNV-1a64 and the FNV-1a64 of what the decoder returned (golden.json,
"js_decoder").  The oracle must still write exactly those streams from exactly those samples."""
import json
import os

import numpy as np

from conftest import GOLDEN

GOLD = json.load(open(os.path.join(GOLDEN, "golden.json")))


def oracle_jobs(mico, synth):
    """[(kind, stream, original samples, decoder arguments)]: kind "frame" is a bare CompressSingleFrame stream, "mic2" a MIC2
    file decoded frame by frame, "file" any other container the decoder's decodeFile reads."""
    mr = np.fromfile(os.path.join(GOLDEN, "MR_256_256_image.bin"), dtype="<u2").reshape(256, 256)
    mx = int(mr.max())
    jobs = []
    tok = mico.delta_rle_compress(mr, mx)
    for ns in (1, 2, 4, 8):                                   # 1-state has no C reference
        rc, blob = mico.fse_compress(tok, ns)
        assert rc == 0
        jobs.append(("frame", blob, mr, {"width": 256, "height": 256}))
    for strips, ns in ((1, 2), (8, 2), (8, 4), (5, 8)):
        rc, blob = mico.pics_compress(mr, mx, strips, ns)
        assert rc == 0
        jobs.append(("file", blob, mr, {}))
    stack = synth.ct_stack(frames=4, size=128, depth=12, seed=3)
    for temporal in (False, True):
        rc, blob = mico.mic2_compress(stack, 4095, temporal)
        assert rc == 0
        jobs.append(("mic2", blob, stack, {}))
    img = synth.wsi_like(300, 256, seed=9)
    rc, blob = mico.wsi_compress(img)
    assert rc == 0
    jobs.append(("file", blob, img, {}))
    rc, blob = mico.micr_write(img[:200, :280])               # MICR: header + CompressRGB blob
    assert rc == 0
    jobs.append(("file", blob, np.ascontiguousarray(img[:200, :280]), {}))
    for ns in (2, 4, 8):                                      # MIC1: header + CompressSingleFrame{,4State,8State}
        rc, blob = mico.mic1_write(mr, mx, ns)
        assert rc == 0
        jobs.append(("file", blob, mr, {}))
    return jobs


def test_js_decoder_accepts_oracle_streams(mico, synth):
    recs = GOLD["js_decoder"]
    jobs = oracle_jobs(mico, synth)
    assert len(jobs) == len(recs)
    for i, ((kind, blob, arr, kw), rec) in enumerate(zip(jobs, recs)):
        assert kind == rec["kind"] and kw == rec["args"], i
        assert len(blob) == rec["size"] and f"{mico.fnv1a64(blob):016x}" == rec["fnv1a64"], (i, kind)
        assert f"{mico.fnv1a64(np.ascontiguousarray(arr).tobytes()):016x}" == rec["decoded_fnv1a64"], (i, kind)
