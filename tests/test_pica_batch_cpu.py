"""CPU tests of the PICA batch ABI: the header declares the entry points, the library exports them, the Python job structs have
the layout a C compiler gives the header's, and MIC_HIP_PICA_BOUND covers what the reference writes."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRY_POINTS = ["mic_hip_pica_compress_batch", "mic_hip_pica_decompress_batch", "mic_hip_pica_compress_ex", "mic_hip_pica_decompress_ex",
                "mic_hip_pica_boundaries"]

_LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "mic_hip.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
    printf("mic_hip_pica_enc_job %zu\n", sizeof(mic_hip_pica_enc_job));
    F(mic_hip_pica_enc_job, pixels); F(mic_hip_pica_enc_job, width); F(mic_hip_pica_enc_job, height); F(mic_hip_pica_enc_job, max_value);
    F(mic_hip_pica_enc_job, num_strips); F(mic_hip_pica_enc_job, out); F(mic_hip_pica_enc_job, out_cap); F(mic_hip_pica_enc_job, out_len);
    F(mic_hip_pica_enc_job, status); F(mic_hip_pica_enc_job, failed_strip);
    printf("mic_hip_pica_dec_job %zu\n", sizeof(mic_hip_pica_dec_job));
    F(mic_hip_pica_dec_job, compressed); F(mic_hip_pica_dec_job, compressed_len); F(mic_hip_pica_dec_job, pixels_out);
    F(mic_hip_pica_dec_job, width); F(mic_hip_pica_dec_job, height); F(mic_hip_pica_dec_job, status); F(mic_hip_pica_dec_job, failed_strip);
    printf("bound %zu\n", (size_t)MIC_HIP_PICA_BOUND(601, 403, 8));
    return 0;
}
'''


def test_header_declares_and_library_exports_the_batch(mic):
    src = open(os.path.join(ROOT, "include", "mic_hip.h")).read()
    L = ctypes.CDLL(mic.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name) and name in mic.ABI_SYMBOLS, name
    assert "MIC_HIP_PICA_BOUND" in src and "mic_hip_pica_enc_job" in src and "mic_hip_pica_dec_job" in src


def test_job_structs_match_the_c_layout(mic, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    c = tmp_path / "layout.c"
    c.write_text(_LAYOUT_C)
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True, capture_output=True, text=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, T in (("mic_hip_pica_enc_job", mic.PicaEncJob), ("mic_hip_pica_dec_job", mic.PicaDecJob)):
        assert int(got[cname]) == ctypes.sizeof(T), cname
        fields = [k for k in got if k.startswith(cname + ".")]
        assert len(fields) == len(T._fields_)
        for name, _ in T._fields_:
            assert int(got[cname + "." + name]) == getattr(T, name).offset, (cname, name)
    assert int(got["bound"]) == mic.pica_bound(601, 403, 8)


def test_bound_covers_what_the_reference_writes(mic, mico, synth):
    mr = np.fromfile(os.path.join(GOLDEN, "MR_256_256_image.bin"), dtype="<u2").reshape(256, 256)
    ct = np.fromfile(os.path.join(GOLDEN, "CT_512_512_image.bin"), dtype="<u2").reshape(512, 512)
    xr = synth.xr_like(cols=601, rows=403, depth=12, seed=4)
    flat = np.full((100, 37), 9, np.uint16); flat[50, 3] = 10
    rng = np.random.default_rng(1)
    noise = rng.integers(0, 65536, (512, 512)).astype(np.uint16)            # 16-bit noise: both predictors' two-state FSE falls back ...
    noise14 = rng.integers(0, 1 << 14, (512, 512)).astype(np.uint16)        # ... and at 14 bits the file is larger than the pixels
    coded = 0
    for img, mx in ((mr, int(mr.max())), (ct, int(ct.max())), (xr, 4095), (flat, 255), (noise, 65535), (noise14, 16383)):
        for ns in (1, 4, 8, 16):
            rc, f = mico.pica_compress(img, mx, ns)
            if rc == 0:
                coded += 1
                assert len(f) <= mic.pica_bound(img.shape[1], img.shape[0], ns), (img.shape, ns)
    assert coded >= 10
    assert mico.pica_compress(noise, 65535, 4)[0] != 0                       # (the one-state fallback gives up as well: an error, no file to bound)
    rc, f = mico.pica_compress(noise14, 16383, 4)
    assert rc == 0 and noise14.nbytes < len(f) <= mic.pica_bound(512, 512, 4)
