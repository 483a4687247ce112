"""CPU tests of the RGB batch interface: the capacity bound against the oracle's output lengths, the ultrasound-like generator, and the
job structs' layout as a C compiler sees include/mic_hip.h (no device is touched)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def test_rgb_bound_against_the_oracle(mic, mico):
    """MIC_HIP_RGB_BOUND is three raw planes: reached exactly by the 2 x 1 image whose planes are all raw, never exceeded by the others"""
    two = np.array([[[10, 200, 30], [11, 100, 50]]], np.uint8)
    rc, blob = mico.wsi_compress_tile(two)
    assert rc == 0 and len(blob) == 27 == 12 + 3 * (1 + 4) == mic.rgb_bound(2, 1)
    rc, f = mico.micr_write(two)
    assert rc == 0 and len(f) == mic.rgb_bound(2, 1, container=True) == 39
    ramp = np.repeat((np.arange(300) % 256).astype(np.uint8)[None, :, None], 3, axis=2)
    rc, blob = mico.wsi_compress_tile(ramp)                                    # raw Y, constant-zero Co and Cg
    assert rc == 0 and len(blob) == 12 + (1 + 600) + 1 + 1 <= mic.rgb_bound(300, 1)
    for im in (np.zeros((1, 1, 3), np.uint8), np.array([[[200, 150, 100]]], np.uint8)):
        rc, blob = mico.wsi_compress_tile(im)
        assert rc == 0 and len(blob) <= mic.rgb_bound(1, 1)


def test_us_like_is_deterministic(synth):
    a, b = synth.us_like(160, 120, 5, seed=3), synth.us_like(160, 120, 5, seed=3)
    assert a.dtype == np.uint8 and a.shape == (120, 160, 3) and np.array_equal(a, b)
    assert not np.array_equal(a, synth.us_like(160, 120, 6, seed=3))           # the speckle drifts with the frame
    assert not np.array_equal(a, synth.us_like(160, 120, 5, seed=4))
    plain = synth.us_like(160, 120, 4, seed=3)
    assert (plain[..., 0] == plain[..., 1]).all() and (plain[..., 1] == plain[..., 2]).all()   # R = G = B: Co and Cg constant zero
    assert (a[..., 0] != a[..., 2]).any()                                     # frame 5 carries the colour box
    assert (plain == 0).mean() > 0.3 and plain.max() > 100                     # a sector on black


_SIZES_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "mic_hip.h"
int main(void) {
    printf("%zu %zu %zu\n", sizeof(mic_hip_rgb_enc_job), sizeof(mic_hip_rgb_dec_job), sizeof(mic_hip_rgb_image));
    printf("%zu %zu %zu %zu\n", offsetof(mic_hip_rgb_enc_job, container), offsetof(mic_hip_rgb_enc_job, out_len),
           offsetof(mic_hip_rgb_enc_job, failed_plane), (size_t)MIC_HIP_RGB_BOUND(2));
    printf("%zu %zu %zu\n", offsetof(mic_hip_rgb_dec_job, out_cap), offsetof(mic_hip_rgb_dec_job, container), offsetof(mic_hip_rgb_dec_job, failed_plane));
    return 0;
}
"""


def test_job_structs_match_the_header(mic, tmp_path):
    """built the way tests/test_c_driver.py builds its driver: gcc against include/mic_hip.h"""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "sizes.c"
    src.write_text(_SIZES_C)
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True, text=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = [int(v) for v in out]
    E, D, I = mic.RgbEncJob, mic.RgbDecJob, mic.RgbImage
    assert got[:3] == [ctypes.sizeof(E), ctypes.sizeof(D), ctypes.sizeof(I)]
    assert got[3:7] == [E.container.offset, E.out_len.offset, E.failed_plane.offset, mic.rgb_bound(2, 1)]
    assert got[7:] == [D.out_cap.offset, D.container.offset, D.failed_plane.offset]


def test_batch_symbols_are_bound(mic):
    for name in ("mic_hip_rgb_compress_batch", "mic_hip_rgb_decompress_batch", "mic_hip_session_rgb_encode", "mic_hip_session_rgb_decode"):
        assert name in mic.ABI_SYMBOLS and hasattr(mic.lib(), name)
