#!/usr/bin/env python3
"""Generates tests/golden/* from the reference's OWN C codec, compiled in place from
/root/reference/ojph (oracle/_ref/libmic_ref.so, `make -C oracle ref`).  Run in the build
container only (the reference does not exist on the GPU box):

    python tests/golden/make_golden.py

Outputs (all data, no reference source):
  CT_512_512_image.bin, MR_256_256_image.bin   the two 16-bit test images the reference's
                                               own tests hold (fseu16_test.go:28-53)
  MR_256_256_{2,4,8}state.mic                  full reference C streams for MR
  <NEMA>_<width>_<height>_2state.mic           full two-state reference C streams of the eight
                                               NEMA images: the images themselves, compactly
  golden.json                                  size / FNV-1a64 / head / tail of the reference
                                               C stream for 10 images x {2,4,8}-state;
                                               "js_decoder": the oracle streams the reference's
                                               JavaScript decoder read back (node required);
                                               "reference_c": what the reference C codec wrote
                                               and read on the inputs of test_gpu_parity.py
"""
import ctypes as C
import importlib
import json
import os
import resource
import shutil
import subprocess
import sys
import tempfile
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
from oracle import mico  # noqa: E402  (only for the FNV helper)

NEMA = {"CT1": (512, 512), "CT2": (512, 512), "MR1": (512, 512), "MR2": (1024, 1024),
        "MR3": (512, 512), "MR4": (512, 512), "NM1": (256, 1024), "XA1": (1024, 1024)}


def load_nema(name):
    """Pixel data of a NEMA *_UNC file without a DICOM library: last
    (7FE0,0010) tag, u32 length at +8, pixels at +12."""
    b = open(f"{REF}/testdata/compsamples_refanddir/IMAGES/REF/{name}_UNC", "rb").read()
    i = b.rfind(bytes([0xE0, 0x7F, 0x10, 0x00]))
    ln = int.from_bytes(b[i + 8:i + 12], "little")
    w, h = NEMA[name]
    return np.frombuffer(b[i + 12:i + 12 + ln], dtype="<u2")[: w * h].reshape(h, w).copy()


def load_synth():
    import __graft_entry__ as entry
    entry.load_package()
    return importlib.import_module("medical_image_codec_amd.synth")


def _rec(b):
    return {"size": len(b), "fnv1a64": f"{mico.fnv1a64(b):016x}"}


def js_decoder_records(synth):
    """The reference's JavaScript decoder (web/mic-decoder.js, driven by tests/js_crosscheck.mjs) on every stream of
    test_oracle_js_crosscheck.oracle_jobs: each must come back as its original samples."""
    sys.path.insert(0, os.path.dirname(HERE))
    import test_oracle_js_crosscheck as jsx
    jobs = jsx.oracle_jobs(mico, synth)
    with tempfile.TemporaryDirectory() as tmp:
        dec = os.path.join(tmp, "mic-decoder.mjs")           # node 12 needs the .mjs suffix for ESM; a temporary copy
        shutil.copy(f"{REF}/web/mic-decoder.js", dec)
        spec = []
        for i, (kind, blob, arr, kw) in enumerate(jobs):
            p_in = os.path.join(tmp, f"in{i}.bin")
            open(p_in, "wb").write(blob)
            spec.append(dict(kind=kind, **{"in": p_in}, out=os.path.join(tmp, f"out{i}.bin"), **kw))
        jp = os.path.join(tmp, "job.json")
        json.dump(spec, open(jp, "w"))
        subprocess.run(["node", os.path.join(os.path.dirname(HERE), "js_crosscheck.mjs"), dec, jp], check=True, timeout=300)
        recs = []
        for (kind, blob, arr, kw), sp in zip(jobs, spec):
            got = open(sp["out"], "rb").read()
            assert got == np.ascontiguousarray(arr).tobytes(), sp["out"]
            recs.append(dict(kind=kind, args=kw, **_rec(blob), decoded_fnv1a64=f"{mico.fnv1a64(got):016x}"))
    return recs


def reference_c_records(R, synth):
    """The reference C codec on the inputs of test_gpu_parity.py: the streams its encoders write (which its decoders read back and
    the oracle writes too), the PICS files of the oracle that its parallel reader takes back, and its streams of single strips /
    frames that PICS and MIC2 files hold when every unit holds the global maximum."""
    sys.path.insert(0, os.path.dirname(HERE))
    import test_gpu_parity as gp
    for name in ("two", "four", "eight"):
        getattr(R, f"mic_compress_{name}_state").argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        getattr(R, f"mic_decompress_{name}_state").argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    for fn in ("mic_decompress_parallel", "mic_decompress_parallel_scalar"):
        getattr(R, fn).argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int]

    def enc(name, px):
        px = np.ascontiguousarray(px)
        out = np.empty(px.size * 4 + 135168, dtype=np.uint8)
        n = C.c_size_t(0)
        assert getattr(R, f"mic_compress_{name}_state")(px.ctypes.data, px.shape[1], px.shape[0], out.ctypes.data, out.size, C.byref(n)) == 0
        return out[: n.value].tobytes()

    frames = []
    for img in gp.ref_codec_frames(synth):
        img = np.ascontiguousarray(img)
        h, w = img.shape
        streams = {}
        for name, ns in (("two", 2), ("four", 4), ("eight", 8)):
            b = enc(name, img)
            a, back = np.frombuffer(b, dtype=np.uint8), np.empty_like(img)
            assert getattr(R, f"mic_decompress_{name}_state")(a.ctypes.data, a.size, back.ctypes.data, w, h) == 0 and np.array_equal(back, img)
            rc, mine = mico.compress_single_frame(img, int(img.max()), ns)
            assert rc == 0 and mine == b, (h, w, ns)
            streams[str(ns)] = _rec(b)
        frames.append({"shape": [h, w], "pixels_fnv1a64": f"{mico.fnv1a64(img.tobytes()):016x}", "streams": streams})
    images, cases = gp.ref_reader_cases(synth)
    reader = []
    for img, mx in images:
        h, w = img.shape
        recs = []
        for strips, ns in cases:
            rc, want = mico.pics_compress(img, mx, strips, ns)
            r = {"strips": strips, "nstates": ns, "rc": rc}
            if rc == 0:
                a = np.frombuffer(want, dtype=np.uint8)
                for fn, threads in (("mic_decompress_parallel", 0), ("mic_decompress_parallel", 3), ("mic_decompress_parallel_scalar", 8)):
                    back = np.zeros_like(img)
                    assert getattr(R, fn)(a.ctypes.data, a.size, back.ctypes.data, w, h, threads) == 0 and np.array_equal(back, img), (strips, ns, fn)
                r.update(_rec(want))
            recs.append(r)
        reader.append(recs)
    img, stack = gp.ref_payload_inputs(synth)
    payloads = {"pics_strips": [_rec(enc("two", img[s * 256:(s + 1) * 256])) for s in range(8)],
                "mic2_frames": [_rec(enc("two", f)) for f in stack]}
    return {"frames": frames, "pics_reader": reader, "payloads": payloads}


def main():
    mico.build(ref=True)
    R = C.CDLL(mico.REF_PATH)
    imgs = {"CT": np.fromfile(f"{REF}/testdata/CT_512_512_image.bin", dtype="<u2").reshape(512, 512),
            "MR": np.fromfile(f"{REF}/testdata/MR_256_256_image.bin", dtype="<u2").reshape(256, 256)}
    for k in NEMA:
        imgs[k] = load_nema(k)
    shutil.copy(f"{REF}/testdata/CT_512_512_image.bin", HERE)
    shutil.copy(f"{REF}/testdata/MR_256_256_image.bin", HERE)
    gold = {"generator": "tests/golden/make_golden.py", "source": "reference C codec ojph/mic_compress_c.c (oracle/_ref)",
            "streams": {}}
    fns = {2: "mic_compress_two_state", 4: "mic_compress_four_state", 8: "mic_compress_eight_state"}
    for name, img in imgs.items():
        h, w = img.shape
        img = np.ascontiguousarray(img)
        for ns, fn in fns.items():
            cap = img.size * 4 + 4096
            out = np.zeros(cap, np.uint8)
            n = C.c_size_t()
            rc = getattr(R, fn)(C.c_void_p(img.ctypes.data), w, h, C.c_void_p(out.ctypes.data), C.c_size_t(cap), C.byref(n))
            assert rc == 0, (name, ns, rc)
            blob = out[: n.value].tobytes()
            gold["streams"][f"{name}/{ns}"] = {
                "width": w, "height": h, "max_value": int(img.max()), "nstates": ns, "size": len(blob),
                "fnv1a64": f"{mico.fnv1a64(blob):016x}", "head": blob[:32].hex(), "tail": blob[-32:].hex(),
                "pixels_fnv1a64": f"{mico.fnv1a64(img.tobytes()):016x}"}
            if name == "MR":
                open(os.path.join(HERE, f"MR_256_256_{ns}state.mic"), "wb").write(blob)
            if name in NEMA and ns == 2:
                open(os.path.join(HERE, f"{name}_{w}_{h}_2state.mic"), "wb").write(blob)
    synth = load_synth()
    gold["js_decoder"] = js_decoder_records(synth)
    gold["reference_c"] = reference_c_records(R, synth)
    json.dump(gold, open(os.path.join(HERE, "golden.json"), "w"), indent=1, sort_keys=True)
    print("wrote", len(gold["streams"]), "stream records")


if __name__ == "__main__":
    # the reference C keeps ~1 MiB of tables on the stack
    resource.setrlimit(resource.RLIMIT_STACK, (resource.RLIM_INFINITY, resource.RLIM_INFINITY))
    threading.stack_size(256 * 1024 * 1024)
    t = threading.Thread(target=main)
    t.start(); t.join()
