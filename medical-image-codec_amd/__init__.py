"""medical-image-codec_amd: MI355X (gfx950) implementation of MIC's parallel-strip hot path.

This package is a thin ctypes binding over the C ABI of ``libmic_hip.so``
(``include/mic_hip.h``) -- the same entry points the reference's Go package binds through
cgo.  Function names mirror the reference's Go API
(``parallelstrips.go``, ``multiframecompress.go``) so tests read like the reference's.

There is no CPU fallback: importing works without a GPU (for symbol checks), but every
codec call raises ``MicError`` unless the HIP library runs on a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MIC_HIP_LIB") or os.path.join(_HERE, "libmic_hip.so")   # (MIC_HIP_LIB: an A/B build of the same ABI, tools/ only)

MIC_OK = 0
MIC_ERR_ARGS = -1
MIC_ERR_NOMEM = -2
MIC_ERR_USE_RLE = -3
MIC_ERR_CAPACITY = -5
MIC_ERR_CORRUPT = -6
MIC_ERR_DEVICE = -7
MIC_ERR_INTERNAL = -8
MIC_ERR_UNSUPPORTED = -9
MIC_HIP_PRED_GRAD = 0x200          # OR'ed into a session unit's nstates: gradient-adaptive predictor (include/mic_hip.h)
MIC_ERR_INCOMPRESSIBLE = -10
MIC_ERR_IO = -11                   # a read / write callback of the MIC3 streaming calls failed
MIC_HIP_GAP_REMOVAL = 0x800        # OR'ed into a session unit's nstates: a gap-removal stream (include/mic_hip.h)
MIC_ERR_MISMATCH = -12             # the verify calls: decoded pixels differ from the reference pixels / the expected CRC-32

_ERR_NAMES = {
    MIC_ERR_ARGS: "bad arguments", MIC_ERR_NOMEM: "out of memory",
    MIC_ERR_USE_RLE: "input is single value repeated",        # ErrUseRLE, fseu16.go:36
    MIC_ERR_CAPACITY: "output buffer too small", MIC_ERR_CORRUPT: "corrupt stream",
    MIC_ERR_DEVICE: "no usable gfx950 device / HIP error", MIC_ERR_INTERNAL: "internal error",
    MIC_ERR_UNSUPPORTED: "unsupported", MIC_ERR_INCOMPRESSIBLE: "input is not compressible",  # fseu16.go:33
    MIC_ERR_IO: "read / write callback failed",
    MIC_ERR_MISMATCH: "decoded pixels differ from the reference",
}


class MicError(RuntimeError):
    def __init__(self, code: int, where: str = ""):
        self.code = code
        super().__init__(f"{where}: {_ERR_NAMES.get(code, 'error')} (rc={code})")


class ErrUseRLE(MicError):
    """Reference sentinel ErrUseRLE (fseu16.go:36)."""


class ErrIncompressible(MicError):
    """Reference sentinel ErrIncompressible (fseu16.go:33)."""


def _raise(code: int, where: str):
    if code == MIC_ERR_USE_RLE:
        raise ErrUseRLE(code, where)
    if code == MIC_ERR_INCOMPRESSIBLE:
        raise ErrIncompressible(code, where)
    raise MicError(code, where)


class EncJob(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("max_value", C.c_uint16), ("nstates", C.c_uint16),
                ("out", C.c_void_p), ("out_cap", C.c_size_t), ("out_len", C.c_size_t),
                ("status", C.c_int32), ("nstates_used", C.c_int32)]


class DecJob(C.Structure):
    _fields_ = [("compressed", C.c_void_p), ("compressed_len", C.c_size_t),
                ("pixels_out", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("status", C.c_int32)]


class PicsEncJob(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("max_value", C.c_uint16), ("nstates", C.c_uint16), ("num_strips", C.c_int32),
                ("out", C.c_void_p), ("out_cap", C.c_size_t), ("out_len", C.c_size_t), ("status", C.c_int32),
                ("failed_strip", C.c_int32)]


class PicsDecJob(C.Structure):
    _fields_ = [("compressed", C.c_void_p), ("compressed_len", C.c_size_t),
                ("pixels_out", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("status", C.c_int32),
                ("failed_strip", C.c_int32)]


class PicaEncJob(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("max_value", C.c_uint16), ("num_strips", C.c_int32),
                ("out", C.c_void_p), ("out_cap", C.c_size_t), ("out_len", C.c_size_t), ("status", C.c_int32),
                ("failed_strip", C.c_int32)]


class PicaDecJob(C.Structure):
    _fields_ = [("compressed", C.c_void_p), ("compressed_len", C.c_size_t),
                ("pixels_out", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("status", C.c_int32),
                ("failed_strip", C.c_int32)]


class RgbEncJob(C.Structure):
    """mic_hip_rgb_enc_job"""
    _fields_ = [("rgb", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("container", C.c_int32),
                ("out", C.c_void_p), ("out_cap", C.c_size_t), ("out_len", C.c_size_t), ("status", C.c_int32),
                ("failed_plane", C.c_int32)]


class RgbDecJob(C.Structure):
    """mic_hip_rgb_dec_job"""
    _fields_ = [("compressed", C.c_void_p), ("compressed_len", C.c_size_t), ("rgb_out", C.c_void_p), ("out_cap", C.c_size_t),
                ("width", C.c_int32), ("height", C.c_int32), ("container", C.c_int32), ("status", C.c_int32),
                ("failed_plane", C.c_int32)]


class RgbImage(C.Structure):
    """mic_hip_rgb_image"""
    _fields_ = [("rgb_off", C.c_uint64), ("width", C.c_int32), ("height", C.c_int32)]


class PatchStats(C.Structure):
    """mic_hip_patch_stats"""
    _fields_ = [("tiles_decoded", C.c_uint64), ("pieces", C.c_uint64), ("slabs", C.c_uint64)]


class TileCacheStats(C.Structure):
    """mic_hip_tile_cache_stats"""
    _fields_ = [(f_, C.c_uint64) for f_ in ("slots", "resident", "hits", "misses", "bypassed", "evictions", "calls", "device_bytes")]


class MultiPatchStats(C.Structure):
    """mic_hip_multi_patch_stats"""
    _fields_ = [("tiles_decoded", C.c_uint64), ("pieces", C.c_uint64), ("slabs", C.c_uint64), ("slides_read", C.c_uint64)]


class CropStats(C.Structure):
    """mic_hip_crop_stats"""
    _fields_ = [("frames_decoded", C.c_uint64), ("pieces", C.c_uint64), ("slabs", C.c_uint64)]


class MultiCropStats(C.Structure):
    """mic_hip_multi_crop_stats"""
    _fields_ = [("frames_decoded", C.c_uint64), ("pieces", C.c_uint64), ("slabs", C.c_uint64), ("volumes_read", C.c_uint64)]


class Mic2EncJob(C.Structure):
    """mic_hip_mic2_enc_job"""
    _fields_ = [("frames", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("nframes", C.c_int32),
                ("max_value", C.c_uint16), ("temporal", C.c_uint16),
                ("out", C.c_void_p), ("out_cap", C.c_size_t), ("out_len", C.c_size_t),
                ("status", C.c_int32), ("failed_frame", C.c_int32)]


class Mic2DecJob(C.Structure):
    """mic_hip_mic2_dec_job"""
    _fields_ = [("compressed", C.c_void_p), ("compressed_len", C.c_size_t), ("frames_out", C.c_void_p), ("frames_cap_px", C.c_size_t),
                ("width", C.c_int32), ("height", C.c_int32), ("nframes", C.c_int32), ("temporal", C.c_int32),
                ("status", C.c_int32), ("failed_frame", C.c_int32)]


class Mic2BatchStats(C.Structure):
    """mic_hip_mic2_batch_stats"""
    _fields_ = [("units", C.c_uint64), ("slabs", C.c_uint64), ("volumes_done", C.c_uint64)]


class Mic2Volume(C.Structure):
    """mic_hip_mic2_volume"""
    _fields_ = [("px_off", C.c_uint64), ("width", C.c_int32), ("height", C.c_int32), ("nframes", C.c_int32),
                ("max_value", C.c_uint16), ("temporal", C.c_uint16)]


class WvEncJob(C.Structure):
    """mic_hip_wv_enc_job"""
    _fields_ = [("pixels", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32), ("max_value", C.c_uint16), ("levels", C.c_int32),
                ("out", C.c_void_p), ("out_cap", C.c_size_t), ("out_len", C.c_size_t), ("status", C.c_int32),
                ("levels_applied", C.c_int32)]


class WvDecJob(C.Structure):
    """mic_hip_wv_dec_job"""
    _fields_ = [("compressed", C.c_void_p), ("compressed_len", C.c_size_t), ("level", C.c_int32),
                ("pixels_out", C.c_void_p), ("out_cap_px", C.c_size_t),
                ("rows", C.c_int32), ("cols", C.c_int32), ("levels", C.c_int32), ("out_rows", C.c_int32), ("out_cols", C.c_int32),
                ("status", C.c_int32), ("symbols_decoded", C.c_uint64)]


class WvBatchStats(C.Structure):
    """mic_hip_wv_batch_stats"""
    _fields_ = [("sub_batches", C.c_uint64), ("chains", C.c_uint64), ("frames_done", C.c_uint64), ("redo_frames", C.c_uint64)]


class StripCropStats(C.Structure):
    """mic_hip_strip_crop_stats"""
    _fields_ = [("strips_decoded", C.c_uint64), ("strips_total", C.c_uint64), ("pieces", C.c_uint64), ("slabs", C.c_uint64)]


class RgbFile(C.Structure):
    """mic_hip_rgb_file"""
    _fields_ = [("data", C.c_void_p), ("len", C.c_size_t), ("width", C.c_int32), ("height", C.c_int32), ("container", C.c_int32)]


class RgbCropStats(C.Structure):
    """mic_hip_rgb_crop_stats"""
    _fields_ = [("planes_decoded", C.c_uint64), ("planes_total", C.c_uint64), ("pieces", C.c_uint64), ("slabs", C.c_uint64)]


class Unit(C.Structure):
    _fields_ = [("px_offset", C.c_uint64), ("width", C.c_int32), ("height", C.c_int32),
                ("max_value", C.c_uint16), ("nstates", C.c_uint16)]


class VerifyResult(C.Structure):
    """mic_hip_verify_result: status MIC_OK (checked and equal), MIC_ERR_MISMATCH, or the codec's own status (not checked);
    crc32 of the reference pixels (zlib.crc32 of their little-endian bytes); differing samples; the first one's pixel index (-1)."""
    _fields_ = [("status", C.c_int32), ("crc32", C.c_uint32), ("mismatches", C.c_uint64), ("first_mismatch", C.c_int64)]

    def __repr__(self):
        return f"VerifyResult(status={self.status}, crc32=0x{self.crc32:08x}, mismatches={self.mismatches}, first_mismatch={self.first_mismatch})"


# every symbol include/mic_hip.h declares (tests/test_abi.py checks the .so exports them all)
ABI_SYMBOLS = [
    "mic_hip_set_device", "mic_hip_set_devices", "mic_hip_get_devices", "mic_hip_shard_plan", "mic_hip_wsi_band_plan", "mic_hip_device_name", "mic_hip_version",
    "mic_hip_compress_frame", "mic_hip_decompress_frame",
    "mic_hip_fse_compress_u16", "mic_hip_fse_decompress_u16_auto", "mic_hip_fse_compress_u16_ex", "mic_hip_fse_decompress_u16_ex",
    "mic_hip_compress_batch", "mic_hip_decompress_batch", "mic_hip_host_alloc", "mic_hip_host_free",
    "mic_hip_pics_compress", "mic_hip_pics_compress_ex", "mic_hip_pics_info", "mic_hip_pics_decompress", "mic_hip_pics_decompress_ex",
    "mic_hip_pics_compress_batch", "mic_hip_pics_decompress_batch",
    "mic_hip_mic2_compress", "mic_hip_mic2_compress_temporal", "mic_hip_mic2_info", "mic_hip_mic2_decompress",
    "mic_hip_mic2_decompress_frame",
    "mic_hip_mic2_crop_plan", "mic_hip_mic2_read_crops", "mic_hip_mic2_reader_open", "mic_hip_mic2_reader_info",
    "mic_hip_mic2_reader_read_crops", "mic_hip_mic2_reader_close", "mic_hip_session_mic2_read_crops",
    "mic_hip_mic2_multi_crop_plan", "mic_hip_mic2_multi_read_crops", "mic_hip_mic2_readers_read_crops",
    "mic_hip_session_mic2_multi_read_crops",
    "mic_hip_mic2_compress_batch", "mic_hip_mic2_decompress_batch", "mic_hip_mic2_batch_plan",
    "mic_hip_session_mic2_encode", "mic_hip_session_mic2_decode",
    "mic_hip_strips_crop_plan", "mic_hip_strips_read_crops", "mic_hip_session_strips_read_crops",
    "mic_hip_rgb_crop_plan", "mic_hip_rgb_read_crops", "mic_hip_session_rgb_read_crops",
    "mic_hip_wavelet_v2_compress", "mic_hip_wavelet_v2_compress_batch", "mic_hip_wavelet_v2_decompress_batch", "mic_hip_wavelet_v2_info", "mic_hip_wavelet_v2_decompress",
    "mic_hip_wavelet_v2_level_info", "mic_hip_wavelet_v2_decompress_level", "mic_hip_wavelet_v2_decompress_level_batch",
    "mic_hip_wavelet_v2_compress_jobs", "mic_hip_wavelet_v2_decompress_jobs", "mic_hip_wavelet_v2_batch_plan",
    "mic_hip_session_wavelet_v2_encode_mixed", "mic_hip_session_wavelet_v2_decode_mixed",
    "mic_hip_compress_frame_gap", "mic_hip_decompress_frame_gap", "mic_hip_compress_batch_gap", "mic_hip_decompress_batch_gap",
    "mic_hip_compress_frame_grad", "mic_hip_decompress_frame_grad", "mic_hip_pica_compress", "mic_hip_pica_info", "mic_hip_pica_decompress",
    "mic_hip_pica_compress_ex", "mic_hip_pica_decompress_ex", "mic_hip_pica_compress_batch", "mic_hip_pica_decompress_batch", "mic_hip_pica_boundaries",
    "mic_hip_rgb_compress", "mic_hip_rgb_decompress", "mic_hip_micr_compress", "mic_hip_micr_info", "mic_hip_micr_decompress",
    "mic_hip_rgb_compress_batch", "mic_hip_rgb_decompress_batch", "mic_hip_session_rgb_encode", "mic_hip_session_rgb_decode",
    "mic_hip_mic1_compress", "mic_hip_mic1_info", "mic_hip_mic1_decompress",
    "mic_hip_wsi_compress", "mic_hip_wsi_compress_ex", "mic_hip_wsi_format", "mic_hip_wsi_info", "mic_hip_wsi_level_info",
    "mic_hip_wsi_decompress_tile", "mic_hip_wsi_decompress_level", "mic_hip_wsi_decompress_region",
    "mic_hip_wsi_patch_plan", "mic_hip_wsi_read_patches", "mic_hip_wsi_reader_read_patches", "mic_hip_session_wsi_read_patches",
    "mic_hip_wsi_multi_patch_plan", "mic_hip_wsi_multi_read_patches", "mic_hip_wsi_readers_read_patches",
    "mic_hip_wsi_writer_open", "mic_hip_wsi_writer_push_rows", "mic_hip_wsi_writer_finish", "mic_hip_wsi_writer_device_bytes",
    "mic_hip_wsi_writer_stats", "mic_hip_wsi_writer_close",
    "mic_hip_wsi_reader_open", "mic_hip_wsi_reader_info", "mic_hip_wsi_reader_decompress_tile", "mic_hip_wsi_reader_decompress_region",
    "mic_hip_wsi_reader_close",
    "mic_hip_session_create", "mic_hip_session_create_on", "mic_hip_session_device", "mic_hip_session_workspace_bytes", "mic_hip_session_destroy", "mic_hip_session_stream",
    "mic_hip_device_copy",
    "mic_hip_session_wavelet_v2_encode", "mic_hip_session_wavelet_v2_decode", "mic_hip_session_wavelet_v2_decode_level",
    "mic_hip_session_wsi_encode", "mic_hip_session_wsi_write", "mic_hip_session_wsi_payload", "mic_hip_session_wsi_decode_level", "mic_hip_session_wsi_levels",
    "mic_hip_session_encode", "mic_hip_session_decode",
    "mic_hip_session_encode_enqueue", "mic_hip_session_encode_finish",
    "mic_hip_session_decode_enqueue", "mic_hip_session_decode_finish",
    "mic_hip_session_set_timing", "mic_hip_session_last_timings",
    "mic_hip_out_spec_check",
    "mic_hip_wsi_read_patches_as",
    "mic_hip_wsi_reader_read_patches_as",
    "mic_hip_session_wsi_read_patches_as",
    "mic_hip_wsi_multi_read_patches_as",
    "mic_hip_wsi_readers_read_patches_as",
    "mic_hip_mic2_read_crops_as",
    "mic_hip_mic2_reader_read_crops_as",
    "mic_hip_session_mic2_read_crops_as",
    "mic_hip_mic2_multi_read_crops_as",
    "mic_hip_mic2_readers_read_crops_as",
    "mic_hip_session_mic2_multi_read_crops_as",
    "mic_hip_strips_read_crops_as",
    "mic_hip_session_strips_read_crops_as",
    "mic_hip_rgb_read_crops_as",
    "mic_hip_session_rgb_read_crops_as",
    "mic_hip_wsi_scaled_extent",
    "mic_hip_wsi_read_patches_scaled",
    "mic_hip_wsi_reader_read_patches_scaled",
    "mic_hip_session_wsi_read_patches_scaled",
    "mic_hip_wsi_multi_read_patches_scaled",
    "mic_hip_wsi_readers_read_patches_scaled",
    "mic_hip_tile_cache_slot_bytes", "mic_hip_tile_cache_create", "mic_hip_tile_cache_clear", "mic_hip_tile_cache_get_stats",
    "mic_hip_tile_cache_destroy", "mic_hip_tile_cache_plan",
    "mic_hip_wsi_reader_set_cache", "mic_hip_wsi_reader_cache_probe", "mic_hip_session_set_tile_cache", "mic_hip_session_tile_cache_probe",
    "mic_hip_frame_cache_slot_bytes", "mic_hip_frame_cache_create", "mic_hip_mic2_reader_set_cache", "mic_hip_mic2_reader_cache_probe",
    "mic_hip_mic2_reader_set_timing", "mic_hip_mic2_reader_last_timings",
    "mic_hip_crc32_combine", "mic_hip_compress_batch_verified", "mic_hip_pics_compress_batch_verified",
    "mic_hip_decompress_batch_crc", "mic_hip_pics_decompress_batch_crc",
    "mic_hip_session_digest", "mic_hip_session_verify", "mic_hip_session_encode_verified",
]

# the readers of many rectangles per call; each has an _as twin that takes a trailing mic_hip_out_spec (OutSpec)
_RECT_DOORS = [s_[:-3] for s_ in ABI_SYMBOLS if s_.endswith("_as")]

_lib: Optional[C.CDLL] = None
# mic_hip_write_fn / mic_hip_read_fn (include/mic_hip.h)
_WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint8), C.c_size_t)
_READ_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint8), C.c_size_t)


def _share_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels carry their own libamdhip64.so (SONAME libamdhip64.so.7) and ask for it by
    the bare name, which the loader does not match against /opt/rocm's copy once libmic_hip.so has pulled that in: a process that
    loads this library first and imports torch afterwards ends up with two runtimes, and the second one finds no GPU.  When a torch
    install is present its copy is loaded first (by path, without importing torch), so either import order gives one runtime.
    MIC_HIP_NO_TORCH_PRELOAD=1 turns the preload off (a process that never imports torch, or whose torch wheel is built against another
    HIP major version than libmic_hip.so: binding this library to that runtime would be an ABI mismatch nobody reports)."""
    import importlib.util
    if "torch" in sys.modules or os.environ.get("MIC_HIP_NO_TORCH_PRELOAD") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError as e:
            import warnings
            warnings.warn(f"mic_hip: could not preload torch's HIP runtime ({cand}: {e}); importing torch after this library may "
                          "leave the process with two runtimes", RuntimeWarning)


def _check_one_hip_runtime():
    """After libmic_hip.so is mapped: exactly one libamdhip64 in the process, or say so loudly (two runtimes = the second finds no
    GPU; see _share_torch_hip_runtime)."""
    try:
        with open("/proc/self/maps") as f:
            paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    except OSError:
        return
    real = {os.path.realpath(q) for q in paths}
    if len(real) > 1:
        import warnings
        warnings.warn("mic_hip: more than one HIP runtime is mapped into this process: " + ", ".join(sorted(real)) +
                      " -- device calls of the one loaded second will fail; import torch before this package, or set "
                      "MIC_HIP_NO_TORCH_PRELOAD=1 and never import torch", RuntimeWarning)


def lib() -> C.CDLL:
    """Loads libmic_hip.so (built in-tree by csrc/build.sh); fails loudly when missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run medical-image-codec_amd/csrc/build.sh "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    _share_torch_hip_runtime()
    L = C.CDLL(LIB_PATH)
    _check_one_hip_runtime()
    L.mic_hip_device_name.restype = C.c_char_p
    L.mic_hip_version.restype = C.c_char_p
    L.mic_hip_session_stream.restype = C.c_void_p
    L.mic_hip_session_stream.argtypes = [C.c_void_p]
    L.mic_hip_session_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_size_t]
    L.mic_hip_device_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.mic_hip_session_create_on.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.c_int, C.c_size_t]
    L.mic_hip_session_device.argtypes = [C.c_void_p]
    L.mic_hip_session_workspace_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.mic_hip_session_workspace_bytes.restype = C.c_size_t
    L.mic_hip_session_wavelet_v2_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                                    C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int)]
    L.mic_hip_session_wavelet_v2_decode.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.c_void_p, C.POINTER(C.c_int32)]
    L.mic_hip_session_wavelet_v2_decode_level.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int, C.c_int,
                                                          C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]
    L.mic_hip_session_wsi_encode.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 7 + [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mic_hip_session_wsi_write.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_session_wsi_payload.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p, C.c_size_t]
    L.mic_hip_session_wsi_decode_level.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.mic_hip_session_wsi_levels.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
    L.mic_hip_session_destroy.argtypes = [C.c_void_p]
    L.mic_hip_wsi_writer_open.argtypes = [C.c_int] * 8 + [_WRITE_FN, C.c_void_p, C.POINTER(C.c_void_p)]
    L.mic_hip_wsi_writer_push_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.mic_hip_wsi_writer_finish.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mic_hip_wsi_writer_device_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mic_hip_wsi_writer_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.mic_hip_wsi_writer_close.argtypes = [C.c_void_p]
    L.mic_hip_wsi_writer_close.restype = None
    L.mic_hip_wsi_reader_open.argtypes = [_READ_FN, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.mic_hip_wsi_reader_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 7
    L.mic_hip_wsi_reader_decompress_tile.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                     C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mic_hip_wsi_reader_decompress_region.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p, C.c_size_t,
                                                       C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mic_hip_wsi_reader_close.argtypes = [C.c_void_p]
    _patch_args = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(PatchStats)]
    L.mic_hip_wsi_patch_plan.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mic_hip_wsi_read_patches.argtypes = [C.c_void_p, C.c_size_t] + _patch_args
    L.mic_hip_wsi_reader_read_patches.argtypes = [C.c_void_p] + _patch_args
    L.mic_hip_session_wsi_read_patches.argtypes = [C.c_void_p] + _patch_args
    _multi_patch_args = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]            # xysl, n, pw, ph, channels, bits_per_sample
    _multi_patch_out = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(MultiPatchStats)]
    L.mic_hip_wsi_multi_patch_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + _multi_patch_args + [
        C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]
    L.mic_hip_wsi_multi_read_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + _multi_patch_args + _multi_patch_out
    L.mic_hip_wsi_readers_read_patches.argtypes = [C.c_void_p, C.c_int] + _multi_patch_args + _multi_patch_out
    L.mic_hip_wsi_reader_close.restype = None
    L.mic_hip_session_destroy.restype = None
    L.mic_hip_compress_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint16, C.c_int,
                                         C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_decompress_frame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    L.mic_hip_compress_frame_gap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint16, C.c_int,
                                             C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_decompress_frame_gap.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    L.mic_hip_fse_compress_u16.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_fse_decompress_u16_auto.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_fse_compress_u16_ex.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_fse_decompress_u16_ex.argtypes = [C.c_void_p, C.c_size_t, C.c_int64, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_compress_batch.argtypes = [C.POINTER(EncJob), C.c_int]
    L.mic_hip_decompress_batch.argtypes = [C.POINTER(DecJob), C.c_int]
    L.mic_hip_compress_batch_gap.argtypes = [C.POINTER(EncJob), C.c_int]
    L.mic_hip_decompress_batch_gap.argtypes = [C.POINTER(DecJob), C.c_int]
    L.mic_hip_pics_compress.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint16, C.c_int, C.c_int,
                                        C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_pics_compress_ex.argtypes = L.mic_hip_pics_compress.argtypes + [C.POINTER(C.c_int)]
    L.mic_hip_pics_decompress_ex.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.mic_hip_set_devices.argtypes = [C.POINTER(C.c_int), C.c_int]
    L.mic_hip_get_devices.argtypes = [C.POINTER(C.c_int), C.c_int]
    L.mic_hip_shard_plan.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.mic_hip_wsi_band_plan.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mic_hip_pics_compress_batch.argtypes = [C.POINTER(PicsEncJob), C.c_int]
    L.mic_hip_pics_decompress_batch.argtypes = [C.POINTER(PicsDecJob), C.c_int]
    L.mic_hip_host_alloc.argtypes = [C.c_size_t]
    L.mic_hip_host_alloc.restype = C.c_void_p
    L.mic_hip_host_free.argtypes = [C.c_void_p]
    L.mic_hip_host_free.restype = None
    L.mic_hip_pics_info.argtypes = [C.c_void_p, C.c_size_t] + [C.POINTER(C.c_int)] * 4
    L.mic_hip_pics_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    L.mic_hip_mic2_compress.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint16,
                                        C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_mic2_compress_temporal.argtypes = L.mic_hip_mic2_compress.argtypes
    L.mic_hip_mic2_info.argtypes = [C.c_void_p, C.c_size_t] + [C.POINTER(C.c_int)] * 4
    L.mic_hip_mic2_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.mic_hip_mic2_decompress_frame.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]
    _crop_args = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(CropStats)]
    L.mic_hip_mic2_crop_plan.argtypes = [C.c_int] * 4 + [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mic_hip_mic2_read_crops.argtypes = [C.c_void_p, C.c_size_t] + _crop_args
    L.mic_hip_mic2_reader_open.argtypes = [_READ_FN, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.mic_hip_mic2_reader_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 4
    L.mic_hip_mic2_reader_read_crops.argtypes = [C.c_void_p] + _crop_args
    L.mic_hip_mic2_reader_close.argtypes = [C.c_void_p]
    L.mic_hip_mic2_reader_close.restype = None
    L.mic_hip_session_mic2_read_crops.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t] + _crop_args
    _multi_crop_args = [C.c_void_p] + [C.c_int] * 4                                        # xyzv, n, cw, ch, cd
    _multi_crop_out = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(MultiCropStats)]
    L.mic_hip_mic2_multi_crop_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + _multi_crop_args + [
        C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]
    L.mic_hip_mic2_multi_read_crops.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + _multi_crop_args + _multi_crop_out
    L.mic_hip_mic2_readers_read_crops.argtypes = [C.c_void_p, C.c_int] + _multi_crop_args + _multi_crop_out
    L.mic_hip_session_mic2_multi_read_crops.argtypes = [C.c_void_p] * 5 + [C.c_int] + _multi_crop_args + _multi_crop_out
    L.mic_hip_mic2_compress_batch.argtypes = [C.POINTER(Mic2EncJob), C.c_int, C.POINTER(Mic2BatchStats)]
    L.mic_hip_mic2_decompress_batch.argtypes = [C.POINTER(Mic2DecJob), C.c_int, C.POINTER(Mic2BatchStats)]
    L.mic_hip_mic2_batch_plan.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mic_hip_session_mic2_encode.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Mic2Volume), C.c_int, C.POINTER(C.c_void_p), C.c_void_p,
                                              C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(Mic2BatchStats)]
    L.mic_hip_session_mic2_decode.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                              C.POINTER(Mic2BatchStats)]
    _strip_crop_args = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(StripCropStats)]
    L.mic_hip_strips_crop_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]
    L.mic_hip_strips_read_crops.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + _strip_crop_args
    L.mic_hip_session_strips_read_crops.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + _strip_crop_args
    _rgb_crop_args = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(RgbCropStats)]
    L.mic_hip_rgb_crop_plan.argtypes = [C.POINTER(RgbFile), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]
    L.mic_hip_rgb_read_crops.argtypes = [C.POINTER(RgbFile), C.c_int] + _rgb_crop_args
    L.mic_hip_session_rgb_read_crops.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RgbImage), C.c_int] + _rgb_crop_args
    L.mic_hip_wavelet_v2_compress.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint16, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_wavelet_v2_compress_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint16, C.c_int, C.c_void_p, C.c_size_t,
                                                    C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    L.mic_hip_wavelet_v2_decompress_batch.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
    L.mic_hip_wavelet_v2_info.argtypes = [C.c_void_p, C.c_size_t] + [C.POINTER(C.c_int)] * 4
    L.mic_hip_wavelet_v2_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.mic_hip_wavelet_v2_level_info.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mic_hip_wavelet_v2_decompress_level.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]
    L.mic_hip_wavelet_v2_decompress_level_batch.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_void_p,
                                                            C.c_size_t, C.POINTER(C.c_int32), C.c_void_p]
    L.mic_hip_wavelet_v2_compress_jobs.argtypes = [C.POINTER(WvEncJob), C.c_int, C.POINTER(WvBatchStats)]
    L.mic_hip_wavelet_v2_decompress_jobs.argtypes = [C.POINTER(WvDecJob), C.c_int, C.POINTER(WvBatchStats)]
    L.mic_hip_wavelet_v2_batch_plan.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.mic_hip_session_wavelet_v2_encode_mixed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                                          C.c_void_p, C.c_void_p, C.c_void_p]
    L.mic_hip_session_wavelet_v2_decode_mixed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                          C.c_void_p, C.c_void_p, C.c_void_p]
    L.mic_hip_wsi_compress.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_compress_frame_grad.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint16, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_decompress_frame_grad.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    L.mic_hip_pica_compress.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint16, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_pica_info.argtypes = [C.c_void_p, C.c_size_t] + [C.POINTER(C.c_int)] * 3
    L.mic_hip_pica_compress_ex.argtypes = L.mic_hip_pica_compress.argtypes + [C.POINTER(C.c_int)]
    L.mic_hip_pica_decompress_ex.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.mic_hip_pica_compress_batch.argtypes = [C.POINTER(PicaEncJob), C.c_int]
    L.mic_hip_pica_decompress_batch.argtypes = [C.POINTER(PicaDecJob), C.c_int]
    L.mic_hip_pica_boundaries.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.mic_hip_pica_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    L.mic_hip_rgb_compress.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_rgb_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    L.mic_hip_micr_compress.argtypes = L.mic_hip_rgb_compress.argtypes
    L.mic_hip_rgb_compress_batch.argtypes = [C.POINTER(RgbEncJob), C.c_int]
    L.mic_hip_rgb_decompress_batch.argtypes = [C.POINTER(RgbDecJob), C.c_int]
    L.mic_hip_session_rgb_encode.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(RgbImage), C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]
    L.mic_hip_session_rgb_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RgbImage), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mic_hip_micr_info.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mic_hip_micr_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.mic_hip_mic1_compress.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint16, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_mic1_info.argtypes = L.mic_hip_micr_info.argtypes
    L.mic_hip_mic1_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.mic_hip_wsi_compress_ex.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.mic_hip_wsi_format.argtypes = [C.c_void_p, C.c_size_t] + [C.POINTER(C.c_int)] * 3
    L.mic_hip_wsi_info.argtypes = [C.c_void_p, C.c_size_t] + [C.POINTER(C.c_int)] * 5 + [C.POINTER(C.c_uint64)]
    L.mic_hip_wsi_level_info.argtypes = [C.c_void_p, C.c_size_t, C.c_int] + [C.POINTER(C.c_int)] * 4
    L.mic_hip_wsi_decompress_tile.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mic_hip_wsi_decompress_level.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]
    L.mic_hip_wsi_decompress_region.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mic_hip_session_encode_enqueue.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Unit), C.c_int]
    L.mic_hip_session_encode_finish.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                                C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.mic_hip_session_decode_enqueue.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                                 C.POINTER(Unit), C.c_int, C.c_void_p]
    L.mic_hip_session_decode_finish.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    for name in _RECT_DOORS:
        getattr(L, name + "_as").argtypes = getattr(L, name).argtypes + [C.c_void_p]
    L.mic_hip_out_spec_check.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
    for name in _RECT_DOORS:
        if hasattr(L, name + "_scaled"):                                                     # the MIC3 patch readers: spec, scale_num, scale_den
            getattr(L, name + "_scaled").argtypes = getattr(L, name).argtypes + [C.c_void_p, C.c_int, C.c_int]
    L.mic_hip_wsi_scaled_extent.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mic_hip_session_set_timing.argtypes = [C.c_void_p, C.c_int]
    L.mic_hip_session_last_timings.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]
    L.mic_hip_tile_cache_slot_bytes.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_uint64)]
    L.mic_hip_tile_cache_create.argtypes = [C.c_int] * 4 + [C.c_uint64, C.POINTER(C.c_void_p)]
    L.mic_hip_tile_cache_clear.argtypes = [C.c_void_p]
    L.mic_hip_frame_cache_slot_bytes.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    L.mic_hip_frame_cache_create.argtypes = [C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
    L.mic_hip_mic2_reader_set_cache.argtypes = [C.c_void_p, C.c_void_p]
    L.mic_hip_mic2_reader_cache_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.mic_hip_mic2_reader_set_timing.argtypes = [C.c_void_p, C.c_int]
    L.mic_hip_mic2_reader_last_timings.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]
    L.mic_hip_tile_cache_get_stats.argtypes = [C.c_void_p, C.POINTER(TileCacheStats)]
    L.mic_hip_tile_cache_destroy.argtypes = [C.c_void_p]
    L.mic_hip_wsi_reader_set_cache.argtypes = [C.c_void_p, C.c_void_p]
    L.mic_hip_wsi_reader_cache_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.mic_hip_session_set_tile_cache.argtypes = [C.c_void_p, C.c_void_p]
    L.mic_hip_session_tile_cache_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.mic_hip_tile_cache_plan.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
    L.mic_hip_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
    L.mic_hip_crc32_combine.restype = C.c_uint32
    L.mic_hip_compress_batch_verified.argtypes = [C.POINTER(EncJob), C.c_int, C.POINTER(VerifyResult)]
    L.mic_hip_pics_compress_batch_verified.argtypes = [C.POINTER(PicsEncJob), C.c_int, C.POINTER(VerifyResult)]
    L.mic_hip_decompress_batch_crc.argtypes = [C.POINTER(DecJob), C.c_int, C.c_void_p, C.c_void_p]
    L.mic_hip_pics_decompress_batch_crc.argtypes = [C.POINTER(PicsDecJob), C.c_int, C.c_void_p, C.c_void_p]
    L.mic_hip_session_digest.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Unit), C.c_int, C.c_void_p]
    L.mic_hip_session_verify.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(Unit), C.c_int, C.c_void_p, C.POINTER(VerifyResult)]
    L.mic_hip_session_encode_verified.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Unit), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_int32), C.POINTER(VerifyResult)]
    L.mic_hip_debug_verify_geometry.argtypes = [C.POINTER(C.c_uint32)]
    _lib = L
    return L


class _OutSpecStruct(C.Structure):
    """mic_hip_out_spec"""
    _fields_ = [("dtype", C.c_int32), ("flags", C.c_uint32), ("affine", C.c_void_p), ("naffine", C.c_int32),
                ("clamp_lo", C.c_float), ("clamp_hi", C.c_float), ("pad", C.c_float)]


OUT_DTYPES = {"native": 0, "u8": 1, "u16": 2, "f16": 3, "bf16": 4, "f32": 5}
OUT_CHANNELS_FIRST, OUT_CLAMP = 1, 2


class OutSpec:
    """mic_hip_out_spec: what the patch and crop readers write when they are given ``spec=``.  dtype: "u8", "u16", "f16", "bf16",
    "f32" (or "native": the door's own format, everything else at its default).  affine: None, or pairs (a, b) -- one, one per
    channel, or one per (source, channel), source-major -- as anything np.asarray turns into an (n, 2) float32 array: the sample is
    fmaf(x, a, b).  clamp: None or (lo, hi), applied behind the affine.  pad: the value of every sample the native door leaves 0
    by definition.  The object keeps the struct and the affine array alive; pass it to as many calls as you like."""

    def __init__(self, dtype="f32", channels_first: bool = False, affine=None, clamp=None, pad: float = 0.0):
        if dtype not in OUT_DTYPES:
            raise ValueError(f"OutSpec: unknown dtype {dtype!r}")
        self.dtype = dtype
        self.channels_first = bool(channels_first)
        self._affine = None if affine is None else np.ascontiguousarray(np.asarray(affine, dtype=np.float32).reshape(-1, 2))
        lo, hi = (0.0, 0.0) if clamp is None else clamp
        flags = (OUT_CHANNELS_FIRST if channels_first else 0) | (OUT_CLAMP if clamp is not None else 0)
        self.struct = _OutSpecStruct(OUT_DTYPES[dtype], flags, None if self._affine is None else self._affine.ctypes.data,
                                     0 if self._affine is None else len(self._affine), lo, hi, pad)

    def ref(self):
        return C.addressof(self.struct)

    def sample_bytes(self, channels: int = 1, bits: int = 16, nsources: int = 1) -> int:
        """bytes of one output sample for sources of `channels` samples a pixel and `bits` bits a sample (out_spec_check)"""
        return out_spec_check(self, channels, bits, nsources)

    def shape(self, n: int, *dims: int, channels: int = 1) -> Tuple[int, ...]:
        """the tensor's shape for n rectangles of `dims` (ph, pw or cd, ch, cw): channels last unless channels_first; no channel
        axis for one channel"""
        if channels == 1:
            return (n, *dims)
        return (n, channels, *dims) if self.channels_first else (n, *dims, channels)


def out_spec_check(spec: OutSpec, channels: int = 1, bits_per_sample: int = 16, nsources: int = 1) -> int:
    """mic_hip_out_spec_check: the bytes of one output sample, or MicError(MIC_ERR_ARGS) for a spec the doors refuse.  No device."""
    nb = C.c_size_t(0)
    rc = lib().mic_hip_out_spec_check(spec.ref() if spec is not None else None, channels, bits_per_sample, nsources, C.byref(nb))
    if rc:
        _raise(rc, "out_spec_check")
    return nb.value


def _door(name: str, spec: Optional[OutSpec], scale=None):
    """the C entry point of a rectangle reader: the native symbol, or with a spec its _as twin with the spec bound as last argument;
    with scale=(num, den) (the MIC3 patch readers) its _scaled twin with the spec, or NULL, and the scale bound behind the rest"""
    if scale is not None:
        num, den = (int(v) for v in scale)
        twin = getattr(lib(), name + "_scaled")
        return lambda *a: twin(*a, spec.ref() if spec is not None else None, num, den)
    if spec is None:
        return getattr(lib(), name)
    twin = getattr(lib(), name + "_as")
    return lambda *a: twin(*a, spec.ref())


def device_name() -> str:
    return lib().mic_hip_device_name().decode()


def device_copy(d_dst: int, d_src: int, nbytes: int) -> None:
    """device -> device copy (a session's result buffers are reused by its next call)"""
    rc = lib().mic_hip_device_copy(d_dst, d_src, nbytes)
    if rc:
        _raise(rc, "device_copy")


def _frame_bound(npx: int) -> int:
    """MIC_HIP_FRAME_BOUND (include/mic_hip.h): worst-case bytes of one coded frame / strip"""
    return 4 * npx + 135168


def _u16(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint16)
    return a


def _bytes_arr(b) -> np.ndarray:
    return np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else np.ascontiguousarray(b, dtype=np.uint8)


# ------------------------------------------------------------------ bare FSE stage
def fse_compress_u16(symbols, flavour: int = 2, table_log: int = 0) -> bytes:
    """FSECompressU16 / TwoState / FourState / EightState (flavour 1/2/4/8) and
    RANSCompressU16EightState (flavour 108); table_log = ScratchU16.TableLog (fseu16.go:101-102; 0 = default)."""
    sym = _u16(symbols).reshape(-1)
    cap = sym.size * 2 + 200000
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().mic_hip_fse_compress_u16_ex(sym.ctypes.data, sym.size, flavour, table_log, out.ctypes.data, cap, C.byref(n))
    if rc:
        _raise(rc, "fse_compress_u16")
    return out[: n.value].tobytes()


def fse_decompress_u16_auto(data, cap: int, decompress_limit: int = 0) -> np.ndarray:
    """FSEDecompressU16Auto (fse2state.go:102-116); decompress_limit = ScratchU16.DecompressLimit (fseu16.go:87-91; 0 = default)."""
    c = _bytes_arr(data)
    out = np.empty(cap, dtype=np.uint16)
    n = C.c_size_t(0)
    rc = lib().mic_hip_fse_decompress_u16_ex(c.ctypes.data, c.size, decompress_limit, out.ctypes.data, cap, C.byref(n))
    if rc:
        _raise(rc, "fse_decompress_u16_auto")
    return out[: n.value].copy()


# ------------------------------------------------------------------ unit codec
def compress_single_frame(pixels, width: int, height: int, max_value: int, nstates: int = 2) -> bytes:
    """CompressSingleFrame / 4State / 8State (multiframecompress.go:15,38,67)."""
    px = _u16(pixels).reshape(-1)
    if px.size != width * height:
        raise MicError(MIC_ERR_ARGS, "compress_single_frame")
    cap = _frame_bound(px.size)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().mic_hip_compress_frame(px.ctypes.data, width, height, max_value, nstates, out.ctypes.data, cap, C.byref(n))
    if rc:
        _raise(rc, "compress_single_frame")
    return out[: n.value].tobytes()


def decompress_single_frame(compressed, width: int, height: int) -> np.ndarray:
    """DecompressSingleFrame (multiframecompress.go:97)."""
    c = _bytes_arr(compressed)
    out = np.empty(width * height, dtype=np.uint16)
    rc = lib().mic_hip_decompress_frame(c.ctypes.data, c.size, out.ctypes.data, width, height)
    if rc:
        _raise(rc, "decompress_single_frame")
    return out.reshape(height, width)


def _encode_batch(where: str, symbol: str, job_type, images, bound, outs=None, **fields):
    """The body of every batch encoder: one `job_type` job per (height, width) uint16 image, every other input field one value
    or one per image; without the caller's `outs`, image i gets a buffer of bound(i, array) bytes.  Returns (jobs, outs) once
    `symbol` has run."""
    n = len(images)
    arrs = [_u16(a) for a in images]
    if outs is None:
        outs = [np.empty(bound(i, a), dtype=np.uint8) for i, a in enumerate(arrs)]
    per = {k: v if np.ndim(v) else [v] * n for k, v in fields.items()}
    jobs = (job_type * n)()
    for i, a in enumerate(arrs):
        h, w = a.shape
        jobs[i].pixels = a.ctypes.data; jobs[i].width = w; jobs[i].height = h
        for k, v in per.items():
            setattr(jobs[i], k, int(v[i]))
        jobs[i].out = outs[i].ctypes.data; jobs[i].out_cap = outs[i].size
    rc = (getattr(lib(), symbol) if isinstance(symbol, str) else symbol)(jobs, n)      # (a callable: a door with further arguments)
    if rc:
        _raise(rc, where)
    return jobs, outs


def _decode_batch(where: str, symbol: str, job_type, files, dims, outs=None):
    """The body of every batch decoder: one `job_type` job per file, dims: (width, height) per file.  Returns (jobs, images),
    images[i] the (height, width) uint16 view of file i's out buffer."""
    n = len(files)
    cs = [_bytes_arr(f) for f in files]
    if outs is None:
        outs = [np.empty(w * h, dtype=np.uint16) for (w, h) in dims]
    jobs = (job_type * n)()
    for i in range(n):
        jobs[i].compressed = cs[i].ctypes.data; jobs[i].compressed_len = cs[i].size
        jobs[i].pixels_out = outs[i].ctypes.data; jobs[i].width = dims[i][0]; jobs[i].height = dims[i][1]
    rc = (getattr(lib(), symbol) if isinstance(symbol, str) else symbol)(jobs, n)
    if rc:
        _raise(rc, where)
    return jobs, [o.reshape(h, w) for o, (w, h) in zip(outs, dims)]


def compress_batch(frames: Sequence[np.ndarray], max_values: Sequence[int], nstates: int = 2
                   ) -> List[Tuple[int, bytes, int]]:
    """One launch chain over many frames; returns [(status, blob, nstates_used)]."""
    jobs, outs = _encode_batch("compress_batch", "mic_hip_compress_batch", EncJob, frames, lambda i, a: _frame_bound(a.size),
                               max_value=max_values, nstates=nstates)
    return [(j.status, o[: j.out_len].tobytes() if j.status == 0 else b"", j.nstates_used) for j, o in zip(jobs, outs)]


def decompress_batch(blobs: Sequence[bytes], dims: Sequence[Tuple[int, int]]) -> List[Tuple[int, Optional[np.ndarray]]]:
    jobs, imgs = _decode_batch("decompress_batch", "mic_hip_decompress_batch", DecJob, blobs, dims)
    return [(j.status, im if j.status == 0 else None) for j, im in zip(jobs, imgs)]


# ------------------------------------------------------------------ gap removal
def _gap_frame_bound(npx: int) -> int:
    """MIC_HIP_GAP_FRAME_BOUND (include/mic_hip.h)"""
    return _frame_bound(npx) + 8195


def compress_single_frame_gap_removal(pixels, width: int, height: int, max_value: int, nstates: int = 2) -> bytes:
    """CompressSingleFrameGapRemoval (gapremovalcompressu16.go:52); nstates 4 / 8 code the compact tokens with the
    CompressSingleFrame4State / 8State chains (the reference's decoder reads them)."""
    px = _u16(pixels).reshape(-1)
    if px.size != width * height:
        raise MicError(MIC_ERR_ARGS, "compress_single_frame_gap_removal")
    cap = _gap_frame_bound(px.size)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().mic_hip_compress_frame_gap(px.ctypes.data, width, height, max_value, nstates, out.ctypes.data, cap, C.byref(n))
    if rc:
        _raise(rc, "compress_single_frame_gap_removal")
    return out[: n.value].tobytes()


def decompress_single_frame_gap_removal(compressed, width: int, height: int) -> np.ndarray:
    """DecompressSingleFrameGapRemoval (gapremovalcompressu16.go:178); MicError(MIC_ERR_CORRUPT) for a malformed map or a decoded
    compact symbol >= numSymbols (only one the payload emits, as :270-273)."""
    c = _bytes_arr(compressed)
    out = np.empty(width * height, dtype=np.uint16)
    rc = lib().mic_hip_decompress_frame_gap(c.ctypes.data, c.size, out.ctypes.data, width, height)
    if rc:
        _raise(rc, "decompress_single_frame_gap_removal")
    return out.reshape(height, width)


def compress_batch_gap_removal(frames: Sequence[np.ndarray], max_values: Sequence[int], nstates: int = 2
                               ) -> List[Tuple[int, bytes, int]]:
    """compress_single_frame_gap_removal over many frames in one call; returns [(status, blob, nstates_used)]."""
    jobs, outs = _encode_batch("compress_batch_gap_removal", "mic_hip_compress_batch_gap", EncJob, frames,
                               lambda i, a: _gap_frame_bound(a.size), max_value=max_values, nstates=nstates)
    return [(j.status, o[: j.out_len].tobytes() if j.status == 0 else b"", j.nstates_used) for j, o in zip(jobs, outs)]


def decompress_batch_gap_removal(blobs: Sequence[bytes], dims: Sequence[Tuple[int, int]]) -> List[Tuple[int, Optional[np.ndarray]]]:
    """decompress_single_frame_gap_removal over many streams in one call; returns [(status, pixels or None)]."""
    jobs, imgs = _decode_batch("decompress_batch_gap_removal", "mic_hip_decompress_batch_gap", DecJob, blobs, dims)
    return [(j.status, im if j.status == 0 else None) for j, im in zip(jobs, imgs)]


# ------------------------------------------------------------------ PICS
def compress_parallel_strips(pixels, width: int, height: int, max_value: int, num_strips: int, nstates: int = 2) -> bytes:
    """CompressParallelStrips / 4State / 8State (parallelstrips.go:55,128,199); a strip's error carries its index, as the
    reference's "parallelstrips: strip %d: %w" does (:97): MicError.strip."""
    px = _u16(pixels).reshape(-1)
    if px.size != width * height:
        raise MicError(MIC_ERR_ARGS, "parallelstrips: pixel count != width*height")
    cap = px.size * 4 + 135168 * max(num_strips, 1) + 8 * max(num_strips, 1) + 20
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0); bad = C.c_int(-1)
    rc = lib().mic_hip_pics_compress_ex(px.ctypes.data, width, height, max_value, num_strips, nstates, out.ctypes.data, cap, C.byref(n), C.byref(bad))
    if rc:
        try:
            _raise(rc, "parallelstrips" + (f": strip {bad.value}" if bad.value >= 0 else ""))
        except MicError as e:
            e.strip = bad.value
            raise
    return out[: n.value].tobytes()


def set_devices(devices: Sequence[int]) -> None:
    """mic_hip_set_devices: the GPUs the batch entry points spread their jobs over (the first is the default device)."""
    arr = (C.c_int * len(devices))(*devices)
    rc = lib().mic_hip_set_devices(arr, len(devices))
    if rc:
        _raise(rc, "set_devices")


def get_devices() -> List[int]:
    arr = (C.c_int * 64)()
    n = lib().mic_hip_get_devices(arr, 64)
    return [arr[i] for i in range(min(n, 64))]


def shard_plan(weights: Sequence[int], shards: int) -> List[int]:
    """mic_hip_shard_plan: first[0..shards] of the contiguous cut the batch entry points make over several devices."""
    w = (C.c_uint64 * len(weights))(*[int(x) for x in weights])
    first = (C.c_int * (shards + 1))()
    rc = lib().mic_hip_shard_plan(w, len(weights), shards, first)
    if rc:
        _raise(rc, "shard_plan")
    return list(first)


def wsi_band_plan(width: int, height: int, tile_w: int = 0, tile_h: int = 0, levels: int = 0, shards: int = 1) -> Tuple[int, List[int]]:
    """mic_hip_wsi_band_plan: (K, row_first[0..shards]) -- the bands of tile rows compress_wsi codes one per device of set_devices."""
    k = C.c_int(0)
    first = (C.c_int * (max(shards, 0) + 1))()
    rc = lib().mic_hip_wsi_band_plan(width, height, tile_w, tile_h, levels, shards, C.byref(k), first)
    if rc:
        _raise(rc, "wsi_band_plan")
    return k.value, list(first)


def pics_bound(width: int, height: int, num_strips: int) -> int:
    """MIC_HIP_PICS_BOUND"""
    ns = max(num_strips, 1)
    return 20 + 8 * ns + 4 * width * height + 135168 * ns


def compress_parallel_strips_batch(images: Sequence[np.ndarray], max_value: int, num_strips: int, nstates: int = 2,
                                   outs: Optional[Sequence[np.ndarray]] = None) -> List[Tuple[int, "np.ndarray"]]:
    """Many images, one call (mic_hip_pics_compress_batch): [(status, file bytes as a uint8 view of its out buffer)].
    images: (height, width) uint16 arrays (ordinary or pinned memory); outs: caller buffers of >= pics_bound bytes, or None."""
    jobs, outs = _encode_batch("compress_parallel_strips_batch", "mic_hip_pics_compress_batch", PicsEncJob, images,
                               lambda i, a: pics_bound(a.shape[1], a.shape[0], num_strips), outs,
                               max_value=max_value, nstates=nstates, num_strips=num_strips)
    compress_parallel_strips_batch.failed_strips = [j.failed_strip for j in jobs]     # (of the last call: index of each job's failing strip, -1)
    return [(j.status, o[: j.out_len]) for j, o in zip(jobs, outs)]


def decompress_parallel_strips_batch(files: Sequence, dims: Sequence[Tuple[int, int]],
                                     outs: Optional[Sequence[np.ndarray]] = None) -> List[Tuple[int, "np.ndarray"]]:
    """Many PICS files, one call (mic_hip_pics_decompress_batch): [(status, (height, width) uint16 pixels)]."""
    jobs, imgs = _decode_batch("decompress_parallel_strips_batch", "mic_hip_pics_decompress_batch", PicsDecJob, files, dims, outs)
    return [(j.status, im) for j, im in zip(jobs, imgs)]


# ------------------------------------------------------------------ verified encode, CRC-32 digests
def crc32_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """mic_hip_crc32_combine: zlib.crc32(A + B) from zlib.crc32(A), zlib.crc32(B) and len(B) in bytes.  Needs no device."""
    return int(lib().mic_hip_crc32_combine(crc_a & 0xFFFFFFFF, crc_b & 0xFFFFFFFF, int(len_b)))


def verify_geometry() -> Tuple[int, int, int]:
    """mic_hip_debug_verify_geometry (a debug probe): the pixels a lane, a wave and a work-group of the digest kernel take"""
    out = (C.c_uint32 * 3)()
    rc = lib().mic_hip_debug_verify_geometry(out)
    if rc:
        _raise(rc, "verify_geometry")
    return int(out[0]), int(out[1]), int(out[2])


def _verified(where: str, symbol: str, job_type, images, bound, outs, **fields):
    """_encode_batch through a _verified door: (jobs, outs, the VerifyResult per job)"""
    res = (VerifyResult * max(len(images), 1))()
    call = getattr(lib(), symbol)
    jobs, outs = _encode_batch(where, lambda j, n: call(j, n, res), job_type, images, bound, outs, **fields)
    return jobs, outs, [res[i] for i in range(len(images))]


def compress_batch_verified(frames: Sequence[np.ndarray], max_values: Sequence[int], nstates: int = 2):
    """compress_batch, every stream decoded again on the device and compared with its frame (mic_hip_compress_batch_verified):
    [(status, blob, nstates_used, VerifyResult)].  A frame that fails the check has status MIC_ERR_MISMATCH and still its bytes."""
    jobs, outs, res = _verified("compress_batch_verified", "mic_hip_compress_batch_verified", EncJob, frames,
                                lambda i, a: _frame_bound(a.size), None, max_value=max_values, nstates=nstates)
    return [(j.status, o[: j.out_len].tobytes(), j.nstates_used, r) for j, o, r in zip(jobs, outs, res)]


def pics_compress_batch_verified(images: Sequence[np.ndarray], max_value: int, num_strips: int, nstates: int = 2,
                                 outs: Optional[Sequence[np.ndarray]] = None):
    """compress_parallel_strips_batch with the check (mic_hip_pics_compress_batch_verified): [(status, file bytes, VerifyResult of
    the whole image, failed_strip)]."""
    jobs, outs, res = _verified("pics_compress_batch_verified", "mic_hip_pics_compress_batch_verified", PicsEncJob, images,
                                lambda i, a: pics_bound(a.shape[1], a.shape[0], num_strips), outs,
                                max_value=max_value, nstates=nstates, num_strips=num_strips)
    return [(j.status, o[: j.out_len], r, j.failed_strip) for j, o, r in zip(jobs, outs, res)]


def _decode_crc(where: str, symbol: str, job_type, files, dims, expect, outs):
    n = len(files)
    crc = np.zeros(max(n, 1), dtype=np.uint32)
    exp = None if expect is None else np.ascontiguousarray(expect, dtype=np.uint32)
    if exp is not None and exp.size != n:
        raise ValueError(where + ": expect must hold one CRC per file")
    call = getattr(lib(), symbol)
    jobs, imgs = _decode_batch(where, lambda j, k: call(j, k, None if exp is None else exp.ctypes.data, crc.ctypes.data), job_type, files, dims, outs)
    return [(j.status, im, int(crc[i])) for i, (j, im) in enumerate(zip(jobs, imgs))]


def decompress_batch_crc(blobs: Sequence[bytes], dims: Sequence[Tuple[int, int]], expect=None, outs=None):
    """decompress_batch with the CRC-32 of every decoded frame, taken on the device (mic_hip_decompress_batch_crc):
    [(status, pixels, crc32)].  expect: one CRC per blob; a frame whose CRC differs has status MIC_ERR_MISMATCH (and its pixels)."""
    return _decode_crc("decompress_batch_crc", "mic_hip_decompress_batch_crc", DecJob, blobs, dims, expect, outs)


def pics_decompress_batch_crc(files: Sequence, dims: Sequence[Tuple[int, int]], expect=None, outs=None):
    """decompress_parallel_strips_batch with the CRC-32 of every decoded image (mic_hip_pics_decompress_batch_crc)."""
    return _decode_crc("pics_decompress_batch_crc", "mic_hip_pics_decompress_batch_crc", PicsDecJob, files, dims, expect, outs)


def host_alloc(nbytes: int, dtype=np.uint8) -> np.ndarray:
    """A pinned host buffer (mic_hip_host_alloc) as a numpy array; free it with host_free(arr)."""
    p = lib().mic_hip_host_alloc(nbytes)
    if not p:
        raise MicError(MIC_ERR_NOMEM, "host_alloc")
    buf = (C.c_uint8 * nbytes).from_address(p)
    a = np.frombuffer(buf, dtype=np.uint8).view(dtype)
    _PINNED[p] = nbytes
    return a


def host_free(a: np.ndarray) -> None:
    """Frees the pinned allocation `a` lies in -- `a` itself, or any view of it (a reshape, a slice: the allocation is found by
    address).  A buffer that host_alloc did not hand out raises instead of leaking quietly."""
    addr = int(a.ctypes.data)
    for p, n in _PINNED.items():
        if p <= addr < p + max(n, 1):
            del _PINNED[p]
            lib().mic_hip_host_free(p)
            return
    raise ValueError("host_free: not (a view of) a buffer from host_alloc, or freed already")


_PINNED = {}


def pics_info(compressed) -> Tuple[int, int, int, int]:
    c = _bytes_arr(compressed)
    w, h, n, sh = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = lib().mic_hip_pics_info(c.ctypes.data, c.size, C.byref(w), C.byref(h), C.byref(n), C.byref(sh))
    if rc:
        _raise(rc, "parallelstrips")
    return w.value, h.value, n.value, sh.value


def decompress_parallel_strips(compressed) -> Tuple[np.ndarray, int, int]:
    """DecompressParallelStrips (parallelstrips.go:270): returns (pixels, width, height)."""
    c = _bytes_arr(compressed)
    w, h, _, _ = pics_info(c)
    out = np.empty(w * h, dtype=np.uint16)
    bad = C.c_int(-1)
    rc = lib().mic_hip_pics_decompress_ex(c.ctypes.data, c.size, out.ctypes.data, w, h, C.byref(bad))
    if rc:
        try:
            _raise(rc, "parallelstrips" + (f": strip {bad.value}" if bad.value >= 0 else ""))
        except MicError as e:
            e.strip = bad.value
            raise
    return out.reshape(h, w), w, h


# ------------------------------------------------------------------ MIC2
def compress_multi_frame(frames: np.ndarray, width: int, height: int, max_value: int, temporal: bool = False) -> bytes:
    """CompressMultiFrame (multiframecompress.go:179): independent frames, or the temporal pipeline
    (frame 0 spatial, ZigZag residuals of consecutive frames after it)."""
    fr = _u16(frames)
    nframes = fr.shape[0]
    cap = fr.size * 4 + 135168 * nframes + 8 * nframes + 20
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    fn = lib().mic_hip_mic2_compress_temporal if temporal else lib().mic_hip_mic2_compress
    rc = fn(fr.ctypes.data, width, height, nframes, max_value, out.ctypes.data, cap, C.byref(n))
    if rc:
        _raise(rc, "compress_multi_frame")
    return out[: n.value].tobytes()


def decompress_multi_frame(compressed) -> np.ndarray:
    """DecompressMultiFrame (multiframecompress.go:227)."""
    c = _bytes_arr(compressed)
    w, h, n, t = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = lib().mic_hip_mic2_info(c.ctypes.data, c.size, C.byref(w), C.byref(h), C.byref(n), C.byref(t))
    if rc:
        _raise(rc, "decompress_multi_frame")
    out = np.empty(max(n.value, 0) * max(w.value, 0) * max(h.value, 0), dtype=np.uint16)
    rc = lib().mic_hip_mic2_decompress(c.ctypes.data, c.size, out.ctypes.data, out.size)
    if rc:
        _raise(rc, "decompress_multi_frame")
    return out.reshape(n.value, h.value, w.value)


def decompress_frame(compressed, frame_idx: int) -> np.ndarray:
    """DecompressFrame (multiframecompress.go:266): one frame of a MIC2 file."""
    c = _bytes_arr(compressed)
    w, h, n, t = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = lib().mic_hip_mic2_info(c.ctypes.data, c.size, C.byref(w), C.byref(h), C.byref(n), C.byref(t))
    if rc:
        _raise(rc, "decompress_frame")
    out = np.empty(max(w.value, 0) * max(h.value, 0), dtype=np.uint16)
    rc = lib().mic_hip_mic2_decompress_frame(c.ctypes.data, c.size, frame_idx, out.ctypes.data, out.size)
    if rc:
        _raise(rc, "decompress_frame")
    return out.reshape(h.value, w.value)


def mic2_bound(width: int, height: int, nframes: int) -> int:
    """MIC_HIP_MIC2_BOUND: the capacity that always suffices for a MIC2 file of either pipeline"""
    return 20 + nframes * (8 + _frame_bound(width * height))


def _mic2_stats(bs) -> dict:
    return dict(units=bs.units, slabs=bs.slabs, volumes_done=bs.volumes_done)


def mic2_batch_plan(whn, budget_bytes: int = 0, cap: Optional[int] = None) -> Tuple[np.ndarray, int]:
    """mic_hip_mic2_batch_plan: the sub-batch cuts [0, ..., units] over the units of the volumes whn = [(width, height, nframes)],
    volume by volume and frame by frame, and the number of units; a batch call over these volumes runs len(cuts) - 1 chains.
    budget_bytes 0: the default workspace ceiling.  Needs no device.  cap: room for that many cuts (default: as many as it takes);
    too few raises MicError (MIC_ERR_CAPACITY) whose ``ncuts`` and ``nunits`` attributes are the counts."""
    a = np.ascontiguousarray(np.asarray(whn, dtype=np.int64).reshape(-1, 3).astype(np.int32))
    nc, nu = C.c_uint64(0), C.c_uint64(0)
    if cap is None:
        rc = lib().mic_hip_mic2_batch_plan(a.ctypes.data, len(a), int(budget_bytes), None, 0, C.byref(nc), C.byref(nu))
        if rc not in (MIC_OK, MIC_ERR_CAPACITY):
            _raise(rc, "mic2_batch_plan")
        cap = nc.value
    cuts = np.zeros(max(cap, 1), dtype=np.uint32)
    rc = lib().mic_hip_mic2_batch_plan(a.ctypes.data, len(a), int(budget_bytes), cuts.ctypes.data, cap, C.byref(nc), C.byref(nu))
    if rc:
        e = MicError(rc, "mic2_batch_plan")
        e.ncuts, e.nunits = nc.value, nu.value
        raise e
    return cuts[: nc.value].copy(), nu.value


def compress_multi_frame_batch(volumes: Sequence, max_values, temporal, outs: Optional[Sequence[np.ndarray]] = None,
                               caps: Optional[Sequence[Optional[int]]] = None):
    """mic_hip_mic2_compress_batch: every volume -- an (nframes, height, width) uint16 array; None: a NULL pointer -- as
    compress_multi_frame writes it, independent or temporal per volume (`max_values` and `temporal`: one value, or one per volume),
    all through shared sub-batches of the unit codec.  outs: the callers' output buffers (e.g. from host_alloc); caps: a capacity
    per volume other than the buffer's.  A volume fails alone.
    -> ([(status, failed frame or -1, file bytes or None)], dict(units, slabs, volumes_done))"""
    n = len(volumes)
    maxv = list(max_values) if hasattr(max_values, "__len__") else [max_values] * n
    temp = list(temporal) if hasattr(temporal, "__len__") else [temporal] * n
    arrs = [None if v is None else _u16(v) for v in volumes]
    jobs = (Mic2EncJob * max(n, 1))()
    bufs = []
    for i, a in enumerate(arrs):
        nf, h, w = (a.shape if a is not None else (1, 1, 1))
        out = outs[i] if outs is not None else np.empty(mic2_bound(w, h, nf), dtype=np.uint8)
        bufs.append(out)
        cap = out.size if caps is None or caps[i] is None else caps[i]
        jobs[i] = Mic2EncJob(None if a is None else a.ctypes.data, w, h, nf, int(maxv[i]), int(bool(temp[i])), out.ctypes.data, cap, 0, 0, -1)
    bs = Mic2BatchStats()
    rc = lib().mic_hip_mic2_compress_batch(jobs, n, C.byref(bs))
    if rc:
        _raise(rc, "compress_multi_frame_batch")
    return [(jobs[i].status, jobs[i].failed_frame, bufs[i][: jobs[i].out_len].tobytes() if jobs[i].status == MIC_OK else None)
            for i in range(n)], _mic2_stats(bs)


def decompress_multi_frame_batch(files: Sequence, outs: Optional[Sequence[np.ndarray]] = None):
    """mic_hip_mic2_decompress_batch: every MIC2 file (None: a NULL pointer) as decompress_multi_frame reads it, both pipelines,
    all through shared sub-batches of the unit codec.  outs: the callers' uint16 output buffers (default: sized from the headers).
    A volume fails alone.
    -> ([(status, failed frame or -1, (width, height, nframes, temporal) of the header, (nframes, height, width) array or None)],
        dict(units, slabs, volumes_done))"""
    n = len(files)
    arrs = [None if f is None else _bytes_arr(f) for f in files]
    jobs = (Mic2DecJob * max(n, 1))()
    bufs = []
    for i, c in enumerate(arrs):
        px = 1
        if c is not None and outs is None:
            w, h, nf, t = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            if lib().mic_hip_mic2_info(c.ctypes.data, c.size, C.byref(w), C.byref(h), C.byref(nf), C.byref(t)) == MIC_OK:
                px = max(nf.value, 0) * max(w.value, 0) * max(h.value, 0)
        out = outs[i] if outs is not None else np.empty(max(px, 1), dtype=np.uint16)
        bufs.append(out)
        jobs[i] = Mic2DecJob(None if c is None else c.ctypes.data, 0 if c is None else c.size, out.ctypes.data, out.size)
    bs = Mic2BatchStats()
    rc = lib().mic_hip_mic2_decompress_batch(jobs, n, C.byref(bs))
    if rc:
        _raise(rc, "decompress_multi_frame_batch")
    res = []
    for i in range(n):
        j = jobs[i]
        px = j.nframes * j.height * j.width
        res.append((j.status, j.failed_frame, (j.width, j.height, j.nframes, j.temporal),
                    bufs[i][:px].reshape(j.nframes, j.height, j.width) if j.status == MIC_OK else None))
    return res, _mic2_stats(bs)


def _crop_xyz(xyz) -> np.ndarray:
    """(n, 3) crop origins (x, y, z) as the int32 triples the C calls take"""
    return np.ascontiguousarray(np.asarray(xyz, dtype=np.int64).reshape(-1, 3).astype(np.int32))


def mic2_crop_plan(width: int, height: int, nframes: int, temporal: bool, xyz, cw: int, ch: int, cd: int,
                   cap: Optional[int] = None) -> Tuple[np.ndarray, int]:
    """mic_hip_mic2_crop_plan: (frames whose streams the crops need entropy-decoded -- ascending, each once --, number of
    (crop, frame) pieces).  Needs no device.  cap: room for that many frames (default: as many as it takes); too few raises
    MicError (MIC_ERR_CAPACITY) whose ``nframes`` and ``pieces`` attributes are the counts."""
    a = _crop_xyz(xyz)
    nf, npc = C.c_uint64(0), C.c_uint64(0)
    if cap is None:
        rc = lib().mic_hip_mic2_crop_plan(width, height, nframes, int(bool(temporal)), a.ctypes.data, len(a), cw, ch, cd, None, 0,
                                          C.byref(nf), C.byref(npc))
        if rc not in (MIC_OK, MIC_ERR_CAPACITY):
            _raise(rc, "mic2_crop_plan")
        cap = nf.value
    frames = np.zeros(max(cap, 1), dtype=np.uint32)
    rc = lib().mic_hip_mic2_crop_plan(width, height, nframes, int(bool(temporal)), a.ctypes.data, len(a), cw, ch, cd,
                                      frames.ctypes.data, cap, C.byref(nf), C.byref(npc))
    if rc:
        e = MicError(rc, "mic2_crop_plan")
        e.nframes, e.pieces = nf.value, npc.value
        raise e
    return frames[: nf.value].copy(), npc.value


def _read_crops(call, xyz, d_out: int, out_cap: int):
    a = _crop_xyz(xyz)
    st = np.zeros(len(a), dtype=np.int32)
    cs = CropStats()
    rc = call(a.ctypes.data, len(a), int(d_out) or None, int(out_cap), st.ctypes.data, C.byref(cs))
    return rc, st, dict(frames_decoded=cs.frames_decoded, pieces=cs.pieces, slabs=cs.slabs)


def mic2_read_crops(compressed, xyz, cw: int, ch: int, cd: int, d_out: int, out_cap: int, spec=None):
    """mic_hip_mic2_read_crops: the cw x ch x cd crops at the (x, y, z) origins `xyz` of a MIC2 file (z = frame index), into the
    caller's device tensor d_out (an int: ``torch.empty((n, cd, ch, cw), dtype=torch.uint16, device="cuda").data_ptr()``, or pinned
    host memory) of out_cap bytes.  Samples outside the volume are 0.  -> (status per crop, dict(frames_decoded, pieces, slabs))."""
    c = _bytes_arr(compressed)
    rc, st, stats = _read_crops(lambda a, n, d, cap, s, p: _door("mic_hip_mic2_read_crops", spec)(
        c.ctypes.data, c.size, a, n, cw, ch, cd, d, cap, s, p), xyz, d_out, out_cap)
    if rc:
        _raise(rc, "mic2_read_crops")
    return st, stats


def _crop_xyzv(xyzv) -> np.ndarray:
    """(n, 4) crop origins and volume indices (x, y, z, volume) as the int32 quadruples the C calls take"""
    return np.ascontiguousarray(np.asarray(xyzv, dtype=np.int64).reshape(-1, 4).astype(np.int32))


def _volume_table(files):
    """_file_table of a list whose entries may be None (a volume no crop names): a NULL pointer of length 0"""
    arrs = [None if f is None else _bytes_arr(f) for f in files]
    ptrs = np.asarray([0 if a is None else a.ctypes.data for a in arrs], dtype=np.uintp)
    lens = np.asarray([0 if a is None else a.size for a in arrs], dtype=np.uintp)
    return arrs, ptrs, lens


def mic2_multi_crop_plan(files, xyzv, cw: int, ch: int, cd: int, cap: Optional[int] = None):
    """mic_hip_mic2_multi_crop_plan: ((n, 2) uint32 array of the (volume, frame) units the crops need entropy-decoded -- ascending by
    volume, then frame, each once --, number of (crop, frame) pieces, int32 status of each volume).  `files`: MIC2 files, or at least
    their headers and frame tables (an entry no crop names may be None).  Needs no device.  cap: room for that many units
    (default: as many as it takes); too few raises MicError (MIC_ERR_CAPACITY) whose ``nframes``, ``pieces`` and ``file_status``
    attributes are the counts and the volumes' codes."""
    arrs, ptrs, lens = _volume_table(files)
    a = _crop_xyzv(xyzv)
    nf, npc = C.c_uint64(0), C.c_uint64(0)
    fs = np.zeros(max(len(arrs), 1), dtype=np.int32)
    head = (ptrs.ctypes.data, lens.ctypes.data, len(arrs), a.ctypes.data, len(a), cw, ch, cd)
    if cap is None:
        rc = lib().mic_hip_mic2_multi_crop_plan(*head, None, None, 0, C.byref(nf), C.byref(npc), fs.ctypes.data)
        if rc not in (MIC_OK, MIC_ERR_CAPACITY):
            _raise(rc, "mic2_multi_crop_plan")
        cap = nf.value
    volume_of, frame_of = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint32)
    rc = lib().mic_hip_mic2_multi_crop_plan(*head, volume_of.ctypes.data, frame_of.ctypes.data, cap, C.byref(nf), C.byref(npc), fs.ctypes.data)
    if rc:
        e = MicError(rc, "mic2_multi_crop_plan")
        e.nframes, e.pieces, e.file_status = nf.value, npc.value, fs[: len(arrs)].copy()
        raise e
    return np.stack([volume_of[: nf.value], frame_of[: nf.value]], axis=1), npc.value, fs[: len(arrs)].copy()


def _read_multi_crops(call, xyzv, d_out: int, out_cap: int):
    a = _crop_xyzv(xyzv)
    st = np.zeros(len(a), dtype=np.int32)
    bad = np.full(len(a), -1, dtype=np.int32)
    cs = MultiCropStats()
    rc = call(a.ctypes.data, len(a), int(d_out) or None, int(out_cap), st.ctypes.data, bad.ctypes.data, C.byref(cs))
    return rc, st, bad, dict(frames_decoded=cs.frames_decoded, pieces=cs.pieces, slabs=cs.slabs, volumes_read=cs.volumes_read)


def mic2_multi_read_crops(files, xyzv, cw: int, ch: int, cd: int, d_out: int, out_cap: int, spec=None):
    """mic_hip_mic2_multi_read_crops: the cw x ch x cd crops (x, y, z, volume) `xyzv` of the MIC2 files `files` (host buffers;
    volume = an index into the list; an entry no crop names may be None), into the caller's device tensor d_out (an int:
    ``torch.empty((n, cd, ch, cw), dtype=torch.uint16, device="cuda").data_ptr()``, or pinned host memory) of out_cap bytes.  The
    volumes may differ in size, depth and pipeline; one that does not parse fails alone.  Samples outside a volume are 0.
    -> (status per crop, failed frame per crop (-1: none), dict(frames_decoded, pieces, slabs, volumes_read))."""
    arrs, ptrs, lens = _volume_table(files)
    rc, st, bad, stats = _read_multi_crops(lambda a, n, d, cap, s, b, p: _door("mic_hip_mic2_multi_read_crops", spec)(
        ptrs.ctypes.data, lens.ctypes.data, len(arrs), a, n, cw, ch, cd, d, cap, s, b, p), xyzv, d_out, out_cap)
    if rc:
        _raise(rc, "mic2_multi_read_crops")
    return st, bad, stats


# ------------------------------------------------------------------ strip files: many crops per call
def strips_head(file) -> bytes:
    """The header and strip table of a PICS or PICA file: its first 20 + 8 * num_strips / 16 + 16 * num_strips bytes -- what
    Session.strips_read_crops takes as `heads` while the file itself lies in device memory."""
    c = _bytes_arr(file)
    pica = c[:4].tobytes() == b"PICA"
    w, h, n = C.c_int(), C.c_int(), C.c_int()
    rc = (lib().mic_hip_pica_info(c.ctypes.data, c.size, C.byref(w), C.byref(h), C.byref(n)) if pica else
          lib().mic_hip_pics_info(c.ctypes.data, c.size, C.byref(w), C.byref(h), C.byref(n), None))
    if rc:
        _raise(rc, "strips_head")
    return c[: 16 + 16 * n.value if pica else 20 + 8 * n.value].tobytes()


def _crop_xyf(xyf) -> np.ndarray:
    """(n, 3) crop origins and file indices (x, y, file) as the int32 triples the C calls take"""
    return np.ascontiguousarray(np.asarray(xyf, dtype=np.int64).reshape(-1, 3).astype(np.int32))


def _file_table(files):
    """the (pointer, length) arrays of a list of host buffers, and the arrays that keep the buffers alive"""
    arrs = [_bytes_arr(f) for f in files]
    ptrs = np.asarray([a.ctypes.data for a in arrs], dtype=np.uintp)
    lens = np.asarray([a.size for a in arrs], dtype=np.uintp)
    return arrs, ptrs, lens


def strips_crop_plan(files, xyf, cw: int, ch: int, cap: Optional[int] = None):
    """mic_hip_strips_crop_plan: ((n, 2) uint32 array of the (file, strip) units the crops need entropy-decoded -- ascending by file,
    then strip, each once --, number of (crop, strip) pieces, int32 status of each file).  Needs no device.  cap: room for that many
    units (default: as many as it takes); too few raises MicError (MIC_ERR_CAPACITY) whose ``nstrips``, ``pieces`` and
    ``file_status`` attributes are the counts and the files' codes."""
    arrs, ptrs, lens = _file_table(files)
    a = _crop_xyf(xyf)
    ns, npc = C.c_uint64(0), C.c_uint64(0)
    fs = np.zeros(max(len(arrs), 1), dtype=np.int32)
    if cap is None:
        rc = lib().mic_hip_strips_crop_plan(ptrs.ctypes.data, lens.ctypes.data, len(arrs), a.ctypes.data, len(a), cw, ch, None, None, 0,
                                            C.byref(ns), C.byref(npc), fs.ctypes.data)
        if rc not in (MIC_OK, MIC_ERR_CAPACITY):
            _raise(rc, "strips_crop_plan")
        cap = ns.value
    file_of, strip_of = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint32)
    rc = lib().mic_hip_strips_crop_plan(ptrs.ctypes.data, lens.ctypes.data, len(arrs), a.ctypes.data, len(a), cw, ch,
                                        file_of.ctypes.data, strip_of.ctypes.data, cap, C.byref(ns), C.byref(npc), fs.ctypes.data)
    if rc:
        e = MicError(rc, "strips_crop_plan")
        e.nstrips, e.pieces, e.file_status = ns.value, npc.value, fs[: len(arrs)].copy()
        raise e
    return np.stack([file_of[: ns.value], strip_of[: ns.value]], axis=1), npc.value, fs[: len(arrs)].copy()


def _read_strip_crops(call, xyf, d_out: int, out_cap: int):
    a = _crop_xyf(xyf)
    st = np.zeros(len(a), dtype=np.int32)
    bad = np.full(len(a), -1, dtype=np.int32)
    cs = StripCropStats()
    rc = call(a.ctypes.data, len(a), int(d_out) or None, int(out_cap), st.ctypes.data, bad.ctypes.data, C.byref(cs))
    return rc, st, bad, dict(strips_decoded=cs.strips_decoded, strips_total=cs.strips_total, pieces=cs.pieces, slabs=cs.slabs)


def strips_read_crops(files, xyf, cw: int, ch: int, d_out: int, out_cap: int, spec=None):
    """mic_hip_strips_read_crops: the cw x ch crops at the (x, y, file) triples `xyf` of the PICS / PICA files `files` (host
    buffers; file = an index into the list), into the caller's device tensor d_out (an int:
    ``torch.empty((n, ch, cw), dtype=torch.uint16, device="cuda").data_ptr()``, or pinned host memory) of out_cap bytes.  Samples
    outside an image are 0.  Only the strips the crops overlap are uploaded and decoded.
    -> (status per crop, failed strip per crop (-1: none), dict(strips_decoded, strips_total, pieces, slabs))."""
    arrs, ptrs, lens = _file_table(files)
    rc, st, bad, stats = _read_strip_crops(lambda a, n, d, cap, s, b, p: _door("mic_hip_strips_read_crops", spec)(
        ptrs.ctypes.data, lens.ctypes.data, len(arrs), a, n, cw, ch, d, cap, s, b, p), xyf, d_out, out_cap)
    if rc:
        _raise(rc, "strips_read_crops")
    return st, bad, stats


# ------------------------------------------------------------------ single-frame RGB files: many crops per call
def rgb_files(files):
    """The mic_hip_rgb_file table of a list of RGB files, and the arrays that keep their bytes alive.  An entry is a MICR file
    (bytes-like: its header names the size), a CompressRGB blob as (blob, width, height), or (data, width, height, container)
    as the C struct has it; data None is a NULL pointer."""
    tab, keep = (RgbFile * max(len(files), 1))(), []
    for i, f in enumerate(files):
        data, w, h, c = (f, 0, 0, 1) if not isinstance(f, tuple) else (f[0], f[1], f[2], f[3] if len(f) > 3 else 0)
        a = None if data is None else _bytes_arr(data)
        keep.append(a)
        tab[i].data = None if a is None else a.ctypes.data
        tab[i].len = 0 if a is None else a.size
        tab[i].width, tab[i].height, tab[i].container = int(w), int(h), int(c)
    return tab, keep


def rgb_crop_plan(files, xyf, cw: int, ch: int, cap: Optional[int] = None):
    """mic_hip_rgb_crop_plan: (uint32 array of the files whose planes the crops need decoded -- ascending, each once --, their
    mode-2 planes, the crops with non-empty overlap, int32 status of each file).  files: as rgb_files takes them.  Needs no
    device.  cap: room for that many files (default: as many as it takes); too few raises MicError (MIC_ERR_CAPACITY) whose
    ``nfiles``, ``planes_coded``, ``pieces`` and ``file_status`` attributes are the counts and the files' codes."""
    tab, keep = rgb_files(files)
    a = _crop_xyf(xyf)
    nf, npl, npc = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    fs = np.zeros(max(len(files), 1), dtype=np.int32)
    if cap is None:
        rc = lib().mic_hip_rgb_crop_plan(tab, len(files), a.ctypes.data, len(a), cw, ch, None, 0,
                                         C.byref(nf), C.byref(npl), C.byref(npc), fs.ctypes.data)
        if rc not in (MIC_OK, MIC_ERR_CAPACITY):
            _raise(rc, "rgb_crop_plan")
        cap = nf.value
    file_of = np.zeros(max(cap, 1), dtype=np.uint32)
    rc = lib().mic_hip_rgb_crop_plan(tab, len(files), a.ctypes.data, len(a), cw, ch, file_of.ctypes.data, cap,
                                     C.byref(nf), C.byref(npl), C.byref(npc), fs.ctypes.data)
    if rc:
        e = MicError(rc, "rgb_crop_plan")
        e.nfiles, e.planes_coded, e.pieces, e.file_status = nf.value, npl.value, npc.value, fs[: len(files)].copy()
        raise e
    return file_of[: nf.value].copy(), npl.value, npc.value, fs[: len(files)].copy()


def _read_rgb_crops(call, xyf, d_out: int, out_cap: int):
    a = _crop_xyf(xyf)
    st = np.zeros(len(a), dtype=np.int32)
    bad = np.full(len(a), -1, dtype=np.int32)
    cs = RgbCropStats()
    rc = call(a.ctypes.data, len(a), int(d_out) or None, int(out_cap), st.ctypes.data, bad.ctypes.data, C.byref(cs))
    return rc, st, bad, dict(planes_decoded=cs.planes_decoded, planes_total=cs.planes_total, pieces=cs.pieces, slabs=cs.slabs)


def rgb_read_crops(files, xyf, cw: int, ch: int, d_out: int, out_cap: int, spec=None):
    """mic_hip_rgb_read_crops: the cw x ch crops at the (x, y, file) triples `xyf` of the CompressRGB blobs / MICR files `files`
    (as rgb_files takes them; file = an index into the list), into the caller's device tensor d_out (an int:
    ``torch.empty((n, ch, cw, 3), dtype=torch.uint8, device="cuda").data_ptr()``, or pinned host memory) of out_cap bytes.
    Samples outside an image are 0.  Only the files some crop overlaps are uploaded and decoded, and only their coded planes.
    -> (status per crop, failed plane per crop (-1: none), dict(planes_decoded, planes_total, pieces, slabs))."""
    tab, keep = rgb_files(files)
    rc, st, bad, stats = _read_rgb_crops(lambda a, n, d, cap, s, b, p: _door("mic_hip_rgb_read_crops", spec)(
        tab, len(files), a, n, cw, ch, d, cap, s, b, p), xyf, d_out, out_cap)
    if rc:
        _raise(rc, "rgb_read_crops")
    return st, bad, stats


# ------------------------------------------------------------------ WaveletV2
def wavelet_v2_compress(pixels, rows: int, cols: int, max_value: int, levels: int = 5) -> bytes:
    """WaveletV2RLEFSECompressU16 / WaveletV2SIMDRLEFSECompressU16 (waveletfsecompressu16.go:303, :374)."""
    px = _u16(pixels).reshape(-1)
    if px.size != rows * cols:
        raise MicError(MIC_ERR_ARGS, "pixel count does not match rows*cols")
    cap = px.size * 6 + 200000
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().mic_hip_wavelet_v2_compress(px.ctypes.data, rows, cols, max_value, levels, out.ctypes.data, cap, C.byref(n))
    if rc:
        _raise(rc, "wavelet_v2_compress")
    return out[: n.value].tobytes()


def wavelet_v2_compress_batch(frames, max_value: int, levels: int = 5) -> List[Tuple[int, bytes]]:
    """nframes x rows x cols frames of one shape in one launch chain: [(status, file)], each file as the single call writes it."""
    fr = np.ascontiguousarray(frames, dtype=np.uint16)
    nf, rows, cols = fr.shape
    stride = rows * cols * 6 + 200000
    out = np.empty(nf * stride, dtype=np.uint8)
    lens = (C.c_size_t * nf)(); st = (C.c_int32 * nf)()
    rc = lib().mic_hip_wavelet_v2_compress_batch(fr.ctypes.data, nf, rows, cols, max_value, levels, out.ctypes.data, stride, lens, st)
    if rc:
        _raise(rc, "wavelet_v2_compress_batch")
    return [(int(st[i]), out[i * stride: i * stride + lens[i]].tobytes() if st[i] == 0 else b"") for i in range(nf)]


def wavelet_v2_decompress_batch(files: Sequence[bytes]) -> Tuple[List[int], np.ndarray]:
    """files of ONE shape -> ([status], nframes x rows x cols uint16)."""
    cs = [_bytes_arr(b) for b in files]
    nf = len(cs)
    r, cc, mv, lv = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = lib().mic_hip_wavelet_v2_info(cs[0].ctypes.data, cs[0].size, C.byref(r), C.byref(cc), C.byref(mv), C.byref(lv))
    if rc:
        _raise(rc, "wavelet_v2_decompress_batch")
    out = np.zeros((nf, max(r.value, 0), max(cc.value, 0)), dtype=np.uint16)
    ptrs = (C.c_void_p * nf)(*[c.ctypes.data for c in cs]); lens = (C.c_size_t * nf)(*[c.size for c in cs]); st = (C.c_int32 * nf)()
    rc = lib().mic_hip_wavelet_v2_decompress_batch(ptrs, lens, nf, out.ctypes.data, out.size, st)
    if rc:
        _raise(rc, "wavelet_v2_decompress_batch")
    return [int(v) for v in st], out


def wavelet_v2_decompress(compressed) -> Tuple[np.ndarray, int, int]:
    """WaveletV2{,SIMD}RLEFSEDecompressU16 (:380, :493): returns (pixels, rows, cols)."""
    c = _bytes_arr(compressed)
    r, cc, mv, lv = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = lib().mic_hip_wavelet_v2_info(c.ctypes.data, c.size, C.byref(r), C.byref(cc), C.byref(mv), C.byref(lv))
    if rc:
        _raise(rc, "wavelet_v2_decompress")
    out = np.empty(max(r.value, 0) * max(cc.value, 0), dtype=np.uint16)
    rc = lib().mic_hip_wavelet_v2_decompress(c.ctypes.data, c.size, out.ctypes.data, out.size)
    if rc:
        _raise(rc, "wavelet_v2_decompress")
    return out.reshape(r.value, cc.value), r.value, cc.value


def wavelet_v2_level_info(compressed, level: int) -> Tuple[int, int]:
    """(rows, cols) of the image at resolution `level` of a WaveletV2 file: nr[0] = rows, nr[l + 1] = (nr[l] + 1) // 2, cols alike;
    0 <= level <= the header's level count (else MicError MIC_ERR_ARGS).  Host only."""
    c = _bytes_arr(compressed)
    r, cc = C.c_int(), C.c_int()
    rc = lib().mic_hip_wavelet_v2_level_info(c.ctypes.data, c.size, int(level), C.byref(r), C.byref(cc))
    if rc:
        _raise(rc, "wavelet_v2_level_info")
    return r.value, cc.value


def wavelet_v2_decompress_level(compressed, level: int) -> np.ndarray:
    """The image at resolution `level` (wavelet_v2_level_info): the LL band the forward transform holds after `level` levels,
    saturated to uint16 -- level 0 is wavelet_v2_decompress's image.  The tANS chain stops after the symbols that band needs, so a
    preview validates only the part of the stream it decodes."""
    c = _bytes_arr(compressed)
    r, cc = wavelet_v2_level_info(c, level)
    out = np.empty(r * cc, dtype=np.uint16)
    rc = lib().mic_hip_wavelet_v2_decompress_level(c.ctypes.data, c.size, int(level), out.ctypes.data, out.size)
    if rc:
        _raise(rc, "wavelet_v2_decompress_level")
    return out.reshape(r, cc)


def wavelet_v2_decompress_level_batch(files: Sequence[bytes], level: int, counts: bool = False):
    """files of ONE shape at resolution `level` -> ([status], nframes x nr x nc uint16), and with counts=True also the tANS symbols
    the chain decoded per frame (uint64; a frame decoded twice -- escape-heavy content -- counts both passes)."""
    cs = [_bytes_arr(b) for b in files]
    nf = len(cs)
    r, cc = wavelet_v2_level_info(cs[0], level)
    out = np.zeros((nf, r, cc), dtype=np.uint16)
    ptrs = (C.c_void_p * nf)(*[c.ctypes.data for c in cs]); lens = (C.c_size_t * nf)(*[c.size for c in cs]); st = (C.c_int32 * nf)()
    syms = np.zeros(nf, dtype=np.uint64)
    rc = lib().mic_hip_wavelet_v2_decompress_level_batch(ptrs, lens, nf, int(level), out.ctypes.data, out.size, st, syms.ctypes.data)
    if rc:
        _raise(rc, "wavelet_v2_decompress_level_batch")
    if counts:
        return [int(v) for v in st], out, syms
    return [int(v) for v in st], out


def _wv_stats(bs) -> dict:
    return dict(sub_batches=bs.sub_batches, chains=bs.chains, frames_done=bs.frames_done, redo_frames=bs.redo_frames)


def wavelet_v2_batch_plan(rc, budget_bytes: int = 0, cap: Optional[int] = None) -> np.ndarray:
    """mic_hip_wavelet_v2_batch_plan: the sub-batch cuts [0, ..., nframes] of the jobs calls over frames rc = [(rows, cols)]; a call
    over these frames runs len(cuts) - 1 sub-batches.  budget_bytes 0: the default workspace ceiling.  Needs no device.  cap: room
    for that many cuts (default: as many as it takes); too few raises MicError (MIC_ERR_CAPACITY) whose ``ncuts`` is the count."""
    a = np.ascontiguousarray(np.asarray(rc, dtype=np.int64).reshape(-1, 2).astype(np.int32))
    nc = C.c_uint64(0)
    if cap is None:
        r = lib().mic_hip_wavelet_v2_batch_plan(a.ctypes.data, len(a), int(budget_bytes), None, 0, C.byref(nc))
        if r not in (MIC_OK, MIC_ERR_CAPACITY):
            _raise(r, "wavelet_v2_batch_plan")
        cap = nc.value
    cuts = np.zeros(max(cap, 1), dtype=np.uint32)
    r = lib().mic_hip_wavelet_v2_batch_plan(a.ctypes.data, len(a), int(budget_bytes), cuts.ctypes.data, cap, C.byref(nc))
    if r:
        e = MicError(r, "wavelet_v2_batch_plan")
        e.ncuts = nc.value
        raise e
    return cuts[: nc.value].copy()


def wavelet_v2_compress_jobs(frames: Sequence, max_values, levels=5, outs: Optional[Sequence[np.ndarray]] = None,
                             caps: Optional[Sequence[Optional[int]]] = None):
    """mic_hip_wavelet_v2_compress_jobs: frames of ANY shapes -- each a (rows, cols) uint16 array; None: a NULL pointer -- in one
    call, every file as wavelet_v2_compress writes it (`max_values` and `levels`: one value, or one per frame).  outs: the callers'
    output buffers (e.g. from host_alloc); caps: a capacity per job instead of the buffer's size.
    -> ([(status, file bytes, levels applied)], stats dict: sub_batches, chains, frames_done, redo_frames); a job fails alone."""
    n = len(frames)
    mv = [int(max_values)] * n if np.isscalar(max_values) else [int(v) for v in max_values]
    lv = [int(levels)] * n if np.isscalar(levels) else [int(v) for v in levels]
    px = [None if f is None else np.ascontiguousarray(f, dtype=np.uint16) for f in frames]
    jobs = (WvEncJob * max(n, 1))()
    bufs = []
    for i in range(n):
        rows, cols = (0, 0) if px[i] is None else px[i].shape
        out = outs[i] if outs is not None else np.empty(rows * cols * 6 + 200000, dtype=np.uint8)
        bufs.append(out)
        cap = out.nbytes if caps is None or caps[i] is None else int(caps[i])
        jobs[i] = WvEncJob(None if px[i] is None else px[i].ctypes.data, rows, cols, mv[i], lv[i], out.ctypes.data, cap, 0, 0, 0)
    bs = WvBatchStats()
    rc = lib().mic_hip_wavelet_v2_compress_jobs(jobs, n, C.byref(bs))
    if rc:
        _raise(rc, "wavelet_v2_compress_jobs")
    res = [(int(jobs[i].status), bufs[i].view(np.uint8).reshape(-1)[: jobs[i].out_len].tobytes() if jobs[i].status == 0 else b"",
            int(jobs[i].levels_applied)) for i in range(n)]
    return res, _wv_stats(bs)


def wavelet_v2_decompress_jobs(files: Sequence, levels=None, outs: Optional[Sequence[np.ndarray]] = None):
    """mic_hip_wavelet_v2_decompress_jobs: WaveletV2 files of ANY shapes and level counts -- None: a NULL pointer -- in one call,
    job i at resolution levels[i] (None: all 0, the full images; wavelet_v2_decompress_level's band otherwise).  outs: the callers'
    uint16 buffers (default: one of the band's size per job).
    -> ([(status, (out_rows, out_cols) uint16 image or None, tANS symbols decoded)], stats dict); a job fails alone."""
    n = len(files)
    lv = [0] * n if levels is None else ([int(levels)] * n if np.isscalar(levels) else [int(v) for v in levels])
    cs = [None if f is None else _bytes_arr(f) for f in files]
    jobs = (WvDecJob * max(n, 1))()
    bufs = []
    for i in range(n):
        if outs is not None:
            out = outs[i]
        else:
            r = cc = 0
            if cs[i] is not None:
                a, b = C.c_int(), C.c_int()
                if lib().mic_hip_wavelet_v2_level_info(cs[i].ctypes.data, cs[i].size, lv[i], C.byref(a), C.byref(b)) == MIC_OK:
                    r, cc = max(a.value, 0), max(b.value, 0)
            out = np.zeros(max(r * cc, 1) if r * cc <= (1 << 27) else 1, dtype=np.uint16)
        bufs.append(out)
        jobs[i] = WvDecJob(None if cs[i] is None else cs[i].ctypes.data, 0 if cs[i] is None else cs[i].size, lv[i],
                           out.ctypes.data, out.size)
    bs = WvBatchStats()
    rc = lib().mic_hip_wavelet_v2_decompress_jobs(jobs, n, C.byref(bs))
    if rc:
        _raise(rc, "wavelet_v2_decompress_jobs")
    res = []
    for i in range(n):
        j = jobs[i]
        img = bufs[i].reshape(-1)[: j.out_rows * j.out_cols].reshape(j.out_rows, j.out_cols) if j.status == 0 else None
        res.append((int(j.status), img, int(j.symbols_decoded)))
    return res, _wv_stats(bs)


# ------------------------------------------------------------------ MIC3 / WSI
def compress_wsi(pixels, width: int, height: int, channels: int = 3, bits_per_sample: int = 8,
                 tile_w: int = 0, tile_h: int = 0, levels: int = 0) -> bytes:
    """CompressWSI (wsicompress.go:27): 8-bit RGB, or greyscale (channels=1) with 8 or 16 bits per sample.
    Like the reference, pixels is the raw byte image; a uint16 array is taken as little-endian 16-bit samples."""
    if not ((channels == 3 and bits_per_sample == 8) or (channels == 1 and bits_per_sample in (8, 16))):
        raise MicError(MIC_ERR_UNSUPPORTED, "compress_wsi: 8-bit RGB or 8/16-bit greyscale")
    arr = np.asarray(pixels)
    if arr.dtype == np.uint16:
        arr = arr.astype("<u2", copy=False)
    px = np.ascontiguousarray(arr).reshape(-1).view(np.uint8) if arr.dtype.itemsize == 2 else np.ascontiguousarray(arr, dtype=np.uint8).reshape(-1)
    bpp = channels * (2 if bits_per_sample == 16 else 1)
    if px.size != width * height * bpp:
        raise MicError(MIC_ERR_ARGS, "compress_wsi")
    cap = px.size * 3 + (1 << 20)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().mic_hip_wsi_compress_ex(px.ctypes.data, width, height, channels, bits_per_sample, tile_w, tile_h, levels,
                                       out.ctypes.data, cap, C.byref(n))
    if rc:
        _raise(rc, "compress_wsi")
    return out[: n.value].tobytes()


def read_wsi_header(compressed):
    """ReadWSIHeader (wsicompress.go:299): dict with the format and the level table."""
    c = _bytes_arr(compressed)
    w, h, tw, th, nl = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    tot = C.c_uint64()
    rc = lib().mic_hip_wsi_info(c.ctypes.data, c.size, C.byref(w), C.byref(h), C.byref(tw), C.byref(th), C.byref(nl), C.byref(tot))
    if rc:
        _raise(rc, "read_wsi_header")
    ch, bps, ct = C.c_int(), C.c_int(), C.c_int()
    lib().mic_hip_wsi_format(c.ctypes.data, c.size, C.byref(ch), C.byref(bps), C.byref(ct))
    levels = []
    for i in range(nl.value):
        lw, lh, tx, ty = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        lib().mic_hip_wsi_level_info(c.ctypes.data, c.size, i, C.byref(lw), C.byref(lh), C.byref(tx), C.byref(ty))
        levels.append(dict(width=lw.value, height=lh.value, tiles_x=tx.value, tiles_y=ty.value))
    return dict(width=w.value, height=h.value, tile_width=tw.value, tile_height=th.value, total_tiles=tot.value,
                channels=ch.value, bits_per_sample=bps.value, color_transform=bool(ct.value), levels=levels)


def _wsi_shape(hdr, out: np.ndarray, w: int, h: int) -> np.ndarray:
    """bytes -> (h, w, 3) uint8 for RGB, (h, w) uint8 / uint16 for greyscale (uint16ToBytes, wsicompress.go:589-603)."""
    if hdr["channels"] == 3:
        return out[: w * h * 3].reshape(h, w, 3)
    if hdr["bits_per_sample"] == 16:
        return out[: w * h * 2].view("<u2").reshape(h, w)
    return out[: w * h].reshape(h, w)


def _wsi_bpp(hdr) -> int:
    return hdr["channels"] * (2 if hdr["bits_per_sample"] == 16 else 1)


def decompress_wsi_tile(compressed, level: int, tile_x: int, tile_y: int) -> np.ndarray:
    """DecompressWSITile (wsicompress.go:175): the tile cropped at the level's edge."""
    c = _bytes_arr(compressed)
    hdr = read_wsi_header(c)
    out = np.empty(hdr["tile_width"] * hdr["tile_height"] * _wsi_bpp(hdr), dtype=np.uint8)
    ow, oh = C.c_int(), C.c_int()
    rc = lib().mic_hip_wsi_decompress_tile(c.ctypes.data, c.size, level, tile_x, tile_y, out.ctypes.data, out.size, C.byref(ow), C.byref(oh))
    if rc:
        _raise(rc, "decompress_wsi_tile")
    return _wsi_shape(hdr, out, ow.value, oh.value).copy()


def decompress_wsi_region(compressed, level: int, x: int, y: int, w: int, h: int) -> np.ndarray:
    """DecompressWSIRegion (wsicompress.go:219): the rectangle clamped to the level."""
    c = _bytes_arr(compressed)
    hdr = read_wsi_header(c)
    out = np.empty(max(w, 0) * max(h, 0) * _wsi_bpp(hdr), dtype=np.uint8)
    ow, oh = C.c_int(), C.c_int()
    rc = lib().mic_hip_wsi_decompress_region(c.ctypes.data, c.size, level, x, y, w, h, out.ctypes.data, out.size, C.byref(ow), C.byref(oh))
    if rc:
        _raise(rc, "decompress_wsi_region")
    return _wsi_shape(hdr, out, ow.value, oh.value)


def decompress_wsi_level(compressed, level: int = 0) -> np.ndarray:
    c = _bytes_arr(compressed)
    hdr = read_wsi_header(c)
    lv = hdr["levels"][level]
    out = np.empty(lv["width"] * lv["height"] * _wsi_bpp(hdr), dtype=np.uint8)
    rc = lib().mic_hip_wsi_decompress_level(c.ctypes.data, c.size, level, out.ctypes.data, out.size)
    if rc:
        _raise(rc, "decompress_wsi_level")
    return _wsi_shape(hdr, out, lv["width"], lv["height"])


def _patch_xy(xy) -> np.ndarray:
    """(n, 2) patch origins (x, y) as the int32 pairs the C calls take"""
    a = np.ascontiguousarray(np.asarray(xy, dtype=np.int64).reshape(-1, 2).astype(np.int32))
    return a


def wsi_patch_plan(level_w: int, level_h: int, tile_w: int, tile_h: int, xy, pw: int, ph: int, cap: Optional[int] = None
                   ) -> Tuple[np.ndarray, int]:
    """mic_hip_wsi_patch_plan: (tiles the patches touch -- ty * tiles_x + tx, ascending, each once --, number of patch-tile
    pieces).  Needs no device.  cap: room for that many tiles (default: as many as it takes); too few raises MicError
    (MIC_ERR_CAPACITY) whose ``ntiles`` attribute is the count."""
    a = _patch_xy(xy)
    nt, npc = C.c_uint64(0), C.c_uint64(0)
    if cap is None:
        rc = lib().mic_hip_wsi_patch_plan(level_w, level_h, tile_w, tile_h, a.ctypes.data, len(a), pw, ph, None, 0, C.byref(nt), C.byref(npc))
        if rc not in (MIC_OK, MIC_ERR_CAPACITY):
            _raise(rc, "wsi_patch_plan")
        cap = nt.value
    tiles = np.zeros(max(cap, 1), dtype=np.uint64)
    rc = lib().mic_hip_wsi_patch_plan(level_w, level_h, tile_w, tile_h, a.ctypes.data, len(a), pw, ph, tiles.ctypes.data, cap, C.byref(nt), C.byref(npc))
    if rc:
        e = MicError(rc, "wsi_patch_plan")
        e.ntiles = nt.value
        raise e
    return tiles[: nt.value].copy(), npc.value


def wsi_scaled_extent(pw: int, ph: int, scale) -> Tuple[int, int]:
    """mic_hip_wsi_scaled_extent: (sw, sh), the level pixels a pw x ph patch covers at scale = (num, den) -- what to plan a scaled
    call with (wsi_patch_plan, wsi_multi_patch_plan, tile_cache_plan); MicError(MIC_ERR_ARGS) for a scale the doors refuse.  Needs
    no device."""
    sw, sh = C.c_int(0), C.c_int(0)
    rc = lib().mic_hip_wsi_scaled_extent(pw, ph, int(scale[0]), int(scale[1]), C.byref(sw), C.byref(sh))
    if rc:
        _raise(rc, "wsi_scaled_extent")
    return sw.value, sh.value


def _read_patches(where: str, call, xy, d_out: int, out_cap: int):
    a = _patch_xy(xy)
    st = np.zeros(len(a), dtype=np.int32)
    ps = PatchStats()
    rc = call(a.ctypes.data, len(a), int(d_out) or None, int(out_cap), st.ctypes.data, C.byref(ps))
    return rc, st, dict(tiles_decoded=ps.tiles_decoded, pieces=ps.pieces, slabs=ps.slabs)


def wsi_read_patches(compressed, level: int, xy, pw: int, ph: int, d_out: int, out_cap: int, spec=None, scale=None):
    """mic_hip_wsi_read_patches: the pw x ph patches at the (x, y) origins `xy` of one level, into the caller's device tensor
    d_out (an int: ``torch.empty((n, ph, pw, C), dtype=torch.uint8, device="cuda").data_ptr()``; torch.uint16 for 16-bit
    greyscale) of out_cap bytes.  Pixels outside the level are 0.  -> (status per patch, dict(tiles_decoded, pieces, slabs)).
    scale=(num, den): mic_hip_wsi_read_patches_scaled -- every output pixel is the exact area average of num / den x num / den
    level pixels (1 <= num / den <= 16), resampled on the device; the patch covers wsi_scaled_extent(pw, ph, scale) level pixels."""
    c = _bytes_arr(compressed)
    rc, st, stats = _read_patches("wsi_read_patches", lambda a, n, d, cap, s, p: _door("mic_hip_wsi_read_patches", spec, scale)(
        c.ctypes.data, c.size, level, a, n, pw, ph, d, cap, s, p), xy, d_out, out_cap)
    if rc:
        _raise(rc, "wsi_read_patches")
    return st, stats


def _patch_xysl(xysl) -> np.ndarray:
    """(n, 4) patches (x, y, slide, level) as the int32 quadruples the C calls take"""
    return np.ascontiguousarray(np.asarray(xysl, dtype=np.int64).reshape(-1, 4).astype(np.int32))


def wsi_multi_patch_plan(files, xysl, pw: int, ph: int, channels: int = 3, bits_per_sample: int = 8, cap: Optional[int] = None):
    """mic_hip_wsi_multi_patch_plan: (uint32 slide of each tile the patches need entropy-decoded, uint64 global tile index of each
    -- ascending by slide, then tile, each once --, number of patch-tile pieces, int32 status of each file).  Needs no device.
    cap: room for that many tiles (default: as many as it takes); too few raises MicError (MIC_ERR_CAPACITY) whose ``ntiles``,
    ``pieces`` and ``file_status`` attributes are the counts and the files' codes."""
    arrs, ptrs, lens = _file_table(files)
    a = _patch_xysl(xysl)
    nt, npc = C.c_uint64(0), C.c_uint64(0)
    fs = np.zeros(max(len(arrs), 1), dtype=np.int32)
    head = (ptrs.ctypes.data, lens.ctypes.data, len(arrs), a.ctypes.data, len(a), pw, ph, channels, bits_per_sample)
    if cap is None:
        rc = lib().mic_hip_wsi_multi_patch_plan(*head, None, None, 0, C.byref(nt), C.byref(npc), fs.ctypes.data)
        if rc not in (MIC_OK, MIC_ERR_CAPACITY):
            _raise(rc, "wsi_multi_patch_plan")
        cap = nt.value
    slide_of, tile_of = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint64)
    rc = lib().mic_hip_wsi_multi_patch_plan(*head, slide_of.ctypes.data, tile_of.ctypes.data, cap, C.byref(nt), C.byref(npc), fs.ctypes.data)
    if rc:
        e = MicError(rc, "wsi_multi_patch_plan")
        e.ntiles, e.pieces, e.file_status = nt.value, npc.value, fs[: len(arrs)].copy()
        raise e
    return slide_of[: nt.value].copy(), tile_of[: nt.value].copy(), npc.value, fs[: len(arrs)].copy()


def _read_multi_patches(call, xysl, d_out: int, out_cap: int):
    a = _patch_xysl(xysl)
    st = np.zeros(len(a), dtype=np.int32)
    ps = MultiPatchStats()
    rc = call(a.ctypes.data, len(a), int(d_out) or None, int(out_cap), st.ctypes.data, C.byref(ps))
    return rc, st, dict(tiles_decoded=ps.tiles_decoded, pieces=ps.pieces, slabs=ps.slabs, slides_read=ps.slides_read)


def wsi_multi_read_patches(files, xysl, pw: int, ph: int, d_out: int, out_cap: int, channels: int = 3, bits_per_sample: int = 8, spec=None,
                           scale=None):
    """mic_hip_wsi_multi_read_patches: the pw x ph patches (x, y, slide, level) `xysl` of the MIC3 files `files` (host buffers;
    slide = an index into the list), into the caller's device tensor d_out (an int:
    ``torch.empty((n, ph, pw, C), dtype=torch.uint8, device="cuda").data_ptr()``; torch.uint16 for 16-bit greyscale; or pinned host
    memory) of out_cap bytes.  Every file must have the call's sample format; one that has not, or does not parse, fails alone.
    Pixels outside a level are 0.  -> (status per patch, dict(tiles_decoded, pieces, slabs, slides_read)).
    scale=(num, den): as in wsi_read_patches, one scale for the call."""
    arrs, ptrs, lens = _file_table(files)
    rc, st, stats = _read_multi_patches(lambda a, n, d, cap, s, p: _door("mic_hip_wsi_multi_read_patches", spec, scale)(
        ptrs.ctypes.data, lens.ctypes.data, len(arrs), a, n, pw, ph, channels, bits_per_sample, d, cap, s, p), xysl, d_out, out_cap)
    if rc:
        _raise(rc, "wsi_multi_read_patches")
    return st, stats


class _Callback:
    """A ctypes callback that never lets an exception pass as success: the first exception it meets is kept, the callback
    returns non-zero (the library then reports MIC_ERR_IO), and the caller re-raises it once the C call has returned.
    fn returning None or 0 is success, any other value a failure (the C convention)."""

    def __init__(self, fn, cfunctype):
        self.exc = None
        self._lock = threading.Lock()

        def tramp(user, offset, ptr, n):
            try:
                return 0 if fn(int(offset), ptr, int(n)) in (None, 0) else 1
            except BaseException as e:     # (ctypes would print it and return 0)
                with self._lock:
                    if self.exc is None:
                        self.exc = e
                return 1
        self.c = cfunctype(tramp)

    def check(self, rc: int, where: str):
        if self.exc is not None:
            e, self.exc = self.exc, None
            raise e
        if rc:
            _raise(rc, where)


class WsiWriter:
    """MIC3 streaming writer (mic_hip_wsi_writer_*): rows go in with push(), top to bottom, in pieces of any size; the sink
    receives the file compress_wsi writes for the same slide, byte for byte.  sink: a binary file object (seek + write) or a
    callable (offset, memoryview).  Level-0 tiles reach the sink as their band is coded; the rest of the file at finish()."""

    def __init__(self, sink, width: int, height: int, channels: int = 3, bits_per_sample: int = 8, tile_w: int = 0,
                 tile_h: int = 0, levels: int = 0, band_tile_rows: int = 0):
        if hasattr(sink, "seek") and hasattr(sink, "write"):
            def put(offset, data):
                sink.seek(offset)
                sink.write(data)
        else:
            put = sink
        self.width, self.height, self.bpp = width, height, channels * (2 if bits_per_sample == 16 else 1)
        self._cb = _Callback(lambda off, ptr, n: put(off, memoryview((C.c_uint8 * n).from_address(C.addressof(ptr.contents))).cast("B")),
                             _WRITE_FN)
        self._h = C.c_void_p()
        rc = lib().mic_hip_wsi_writer_open(width, height, channels, bits_per_sample, tile_w, tile_h, levels, band_tile_rows,
                                           self._cb.c, None, C.byref(self._h))
        self._cb.check(rc, "WsiWriter")

    def push(self, rows) -> None:
        """The next rows of the slide: (n, width, 3) / (n, width) arrays, or raw bytes of whole rows."""
        arr = np.asarray(rows)
        if arr.dtype == np.uint16:
            arr = arr.astype("<u2", copy=False)
        px = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        if px.size == 0 or px.size % (self.width * self.bpp):
            raise MicError(MIC_ERR_ARGS, "WsiWriter.push: whole rows")
        self._cb.check(lib().mic_hip_wsi_writer_push_rows(self._h, px.ctypes.data, px.size // (self.width * self.bpp)), "WsiWriter.push")

    def finish(self) -> int:
        """Writes the upper levels, the header and the tile index; returns the file's length."""
        n = C.c_uint64(0)
        self._cb.check(lib().mic_hip_wsi_writer_finish(self._h, C.byref(n)), "WsiWriter.finish")
        return n.value

    @property
    def device_bytes(self) -> int:
        n = C.c_uint64(0)
        self._cb.check(lib().mic_hip_wsi_writer_device_bytes(self._h, C.byref(n)), "WsiWriter.device_bytes")
        return n.value

    @property
    def stats(self):
        """dict(bands, band_rows, pyramid_ms, host_bytes_peak): bands coded, level-0 rows per band, device time of the band
        pyramid kernel over them, peak host bytes the writer held."""
        b, r, hp, ms = C.c_uint64(0), C.c_int(0), C.c_uint64(0), C.c_double(0)
        self._cb.check(lib().mic_hip_wsi_writer_stats(self._h, C.byref(b), C.byref(r), C.byref(ms), C.byref(hp)), "WsiWriter.stats")
        return dict(bands=b.value, band_rows=r.value, pyramid_ms=ms.value, host_bytes_peak=hp.value)

    def close(self) -> None:
        if self._h:
            lib().mic_hip_wsi_writer_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _read_source(source, file_len: Optional[int], where: str):
    """(get(offset, n) -> bytes-like, file_len) of a reader's source: bytes, a binary file object, or a callable"""
    if isinstance(source, (bytes, bytearray, memoryview, np.ndarray)):
        buf = memoryview(source).cast("B")
        get = lambda off, n: buf[off: off + n]
        file_len = len(buf) if file_len is None else file_len
    elif hasattr(source, "seek") and hasattr(source, "read"):
        def get(off, n):
            source.seek(off)
            return source.read(n)
        if file_len is None:
            file_len = source.seek(0, os.SEEK_END)
    else:
        get = source
    if file_len is None:
        raise MicError(MIC_ERR_ARGS, where + ": file_len")
    return get, int(file_len)


def tile_cache_slot_bytes(tile_w: int, tile_h: int, channels: int = 3, bits_per_sample: int = 8) -> int:
    """mic_hip_tile_cache_slot_bytes: device bytes of one slot of a TileCache of that format (a multiple of 256).  No device."""
    nb = C.c_uint64(0)
    rc = lib().mic_hip_tile_cache_slot_bytes(tile_w, tile_h, channels, bits_per_sample, C.byref(nb))
    if rc:
        _raise(rc, "tile_cache_slot_bytes")
    return nb.value


def tile_cache_plan(nslots: int, calls) -> Tuple[List[np.ndarray], int]:
    """mic_hip_tile_cache_plan: the cache's replacement policy alone, over a trace.  calls: a sequence of calls, each the ascending,
    distinct keys (global tile indices) of its tiles.  -> (per call a uint8 array: 0 hit, 1 miss (kept), 2 bypassed; evictions in
    all).  No device."""
    calls = [np.ascontiguousarray(np.asarray(c, dtype=np.uint64).reshape(-1)) for c in calls]
    keys = np.concatenate(calls) if calls else np.zeros(0, dtype=np.uint64)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    lens = np.asarray([len(c) for c in calls], dtype=np.uint32)
    out = np.zeros(max(len(keys), 1), dtype=np.uint8)
    ev = C.c_uint64(0)
    rc = lib().mic_hip_tile_cache_plan(int(nslots), keys.ctypes.data, lens.ctypes.data, len(calls), out.ctypes.data, C.byref(ev))
    if rc:
        _raise(rc, "tile_cache_plan")
    cuts = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
    return [out[cuts[k]: cuts[k + 1]].copy() for k in range(len(calls))], ev.value


class TileCache:
    """mic_hip_tile_cache: decoded MIC3 tiles kept in device memory, `slots` of them, for readers and sessions whose slides have
    this tile size and sample format (WsiReader.set_cache, Session.set_tile_cache).  A patch call of an owner with a cache decodes
    only the tiles that are not resident.  The arena (slots * tile_cache_slot_bytes) is allocated by the first call that uses it.
    Threads that share a cache serialise on it.  close() fails (MIC_ERR_ARGS) while a reader or session is still attached."""

    def __init__(self, tile_w: int, tile_h: int, channels: int = 3, bits_per_sample: int = 8, slots: int = 0):
        self._h = C.c_void_p()
        rc = lib().mic_hip_tile_cache_create(tile_w, tile_h, channels, bits_per_sample, int(slots), C.byref(self._h))
        if rc:
            _raise(rc, "TileCache")

    def stats(self) -> dict:
        st = TileCacheStats()
        rc = lib().mic_hip_tile_cache_get_stats(self._h, C.byref(st))
        if rc:
            _raise(rc, "TileCache.stats")
        return {f_: int(getattr(st, f_)) for f_, _ in TileCacheStats._fields_}

    def clear(self) -> None:
        rc = lib().mic_hip_tile_cache_clear(self._h)
        if rc:
            _raise(rc, "TileCache.clear")

    def close(self) -> None:
        if self._h:
            rc = lib().mic_hip_tile_cache_destroy(self._h)
            if rc:
                _raise(rc, "TileCache.close")
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def frame_cache_slot_bytes(width: int, height: int) -> int:
    """mic_hip_frame_cache_slot_bytes: device bytes of one slot of a FrameCache for frames of width x height (a multiple of 256).
    No device."""
    nb = C.c_uint64(0)
    rc = lib().mic_hip_frame_cache_slot_bytes(width, height, C.byref(nb))
    if rc:
        _raise(rc, "frame_cache_slot_bytes")
    return nb.value


class FrameCache(TileCache):
    """mic_hip_frame_cache_create: reconstructed MIC2 frames of width x height kept in device memory, `slots` of them, for readers
    of files of that frame size (Mic2Reader.set_cache).  A crop call of a reader with a cache decodes only the frames that are
    not resident; for a temporal file a resident frame is a key frame, and only the residuals behind the nearest one below a
    wanted frame are decoded.  The same object as a TileCache: stats, clear and close are its."""

    def __init__(self, width: int, height: int, slots: int = 0):
        self._h = C.c_void_p()
        rc = lib().mic_hip_frame_cache_create(width, height, int(slots), C.byref(self._h))
        if rc:
            _raise(rc, "FrameCache")


def _cache_probe(call, tiles, dtype=np.uint64) -> np.ndarray:
    t = np.ascontiguousarray(np.asarray(tiles, dtype=dtype).reshape(-1))
    res = np.zeros(max(len(t), 1), dtype=np.uint8)
    rc = call(t.ctypes.data, len(t), res.ctypes.data)
    if rc:
        _raise(rc, "cache_probe")
    return res[: len(t)].astype(bool)


class WsiReader:
    """MIC3 random-access reader (mic_hip_wsi_reader_*): reads the header and tile index at open, then only the blobs of the
    tiles a tile() or region() covers.  source: a binary file object (seek + read), bytes, or a callable (offset, n) -> bytes."""

    def __init__(self, source, file_len: Optional[int] = None):
        get, file_len = _read_source(source, file_len, "WsiReader")

        def fill(off, ptr, n):
            data = get(off, n)
            if len(data) != n:
                raise EOFError(f"WsiReader: {len(data)} of {n} bytes at {off}")
            C.memmove(ptr, bytes(data), n)
        self._cb = _Callback(fill, _READ_FN)
        self._h = C.c_void_p()
        self._cb.check(lib().mic_hip_wsi_reader_open(self._cb.c, None, int(file_len), C.byref(self._h)), "WsiReader")
        v = [C.c_int() for _ in range(7)]
        lib().mic_hip_wsi_reader_info(self._h, *[C.byref(x) for x in v])
        w, h, tw, th, nl, ch, bps = (x.value for x in v)
        self.info = dict(width=w, height=h, tile_width=tw, tile_height=th, levels=nl, channels=ch, bits_per_sample=bps)

    def tile(self, level: int, tile_x: int, tile_y: int) -> np.ndarray:
        """as decompress_wsi_tile on the whole file"""
        out = np.empty(self.info["tile_width"] * self.info["tile_height"] * _wsi_bpp(self.info), dtype=np.uint8)
        ow, oh = C.c_int(), C.c_int()
        self._cb.check(lib().mic_hip_wsi_reader_decompress_tile(self._h, level, tile_x, tile_y, out.ctypes.data, out.size,
                                                                C.byref(ow), C.byref(oh)), "WsiReader.tile")
        return _wsi_shape(self.info, out, ow.value, oh.value).copy()

    def region(self, level: int, x: int, y: int, w: int, h: int) -> np.ndarray:
        """as decompress_wsi_region on the whole file"""
        out = np.empty(max(w, 0) * max(h, 0) * _wsi_bpp(self.info), dtype=np.uint8)
        ow, oh = C.c_int(), C.c_int()
        self._cb.check(lib().mic_hip_wsi_reader_decompress_region(self._h, level, x, y, w, h, out.ctypes.data, out.size,
                                                                  C.byref(ow), C.byref(oh)), "WsiReader.region")
        return _wsi_shape(self.info, out, ow.value, oh.value)

    def read_patches(self, level: int, xy, pw: int, ph: int, d_out: int, out_cap: int, spec=None, scale=None):
        """as wsi_read_patches on the whole file; only the blobs of the tiles the patches touch are read, each once"""
        rc, st, stats = _read_patches("WsiReader.read_patches", lambda a, n, d, cap, s, p: _door("mic_hip_wsi_reader_read_patches", spec, scale)(
            self._h, level, a, n, pw, ph, d, cap, s, p), xy, d_out, out_cap)
        self._cb.check(rc, "WsiReader.read_patches")
        return st, stats

    def set_cache(self, cache: Optional["TileCache"]) -> None:
        """mic_hip_wsi_reader_set_cache: read_patches (and wsi_readers_read_patches) then decode only the tiles that are not
        resident in `cache`, and read only their blobs; None detaches and drops this reader's entries.  A cache of another tile
        size or sample format raises MicError(MIC_ERR_ARGS)."""
        rc = lib().mic_hip_wsi_reader_set_cache(self._h, cache._h if cache is not None else None)
        if rc:
            _raise(rc, "WsiReader.set_cache")
        self._cache = cache                            # (kept alive while attached)

    def cache_probe(self, tiles) -> np.ndarray:
        """bool per global tile index (level.first + ty * tiles_x + tx): resident in this reader's cache; changes no state"""
        return _cache_probe(lambda t, n, r: lib().mic_hip_wsi_reader_cache_probe(self._h, t, n, r), tiles)

    def close(self) -> None:
        if self._h:
            lib().mic_hip_wsi_reader_close(self._h)
            self._h = C.c_void_p()
            self._cache = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def wsi_readers_read_patches(readers, xysl, pw: int, ph: int, d_out: int, out_cap: int, channels: int = 3, bits_per_sample: int = 8, spec=None,
                             scale=None):
    """mic_hip_wsi_readers_read_patches: wsi_multi_read_patches over a sequence of WsiReader (slide = an index into it; an entry
    no patch names may be None and is never read).  Only the blobs of the tiles the patches touch are read, each once."""
    readers = list(readers)
    hs = np.asarray([(r._h.value or 0) if r is not None else 0 for r in readers], dtype=np.uintp)
    rc, st, stats = _read_multi_patches(lambda a, n, d, cap, s, p: _door("mic_hip_wsi_readers_read_patches", spec, scale)(
        hs.ctypes.data, len(readers), a, n, pw, ph, channels, bits_per_sample, d, cap, s, p), xysl, d_out, out_cap)
    for r in readers:                                  # an exception a source raised comes first
        if r is not None and r._cb.exc is not None:
            r._cb.check(rc, "wsi_readers_read_patches")
    if rc:
        _raise(rc, "wsi_readers_read_patches")
    return st, stats


class Mic2Reader:
    """MIC2 random-access reader (mic_hip_mic2_reader_*): reads the header and the frame table at open, then only the streams of
    the frames a read_crops() needs.  source: a binary file object (seek + read), bytes, or a callable (offset, n) -> bytes."""

    def __init__(self, source, file_len: Optional[int] = None):
        get, file_len = _read_source(source, file_len, "Mic2Reader")

        def fill(off, ptr, n):
            data = get(off, n)
            if len(data) != n:
                raise EOFError(f"Mic2Reader: {len(data)} of {n} bytes at {off}")
            C.memmove(ptr, bytes(data), n)
        self._cb = _Callback(fill, _READ_FN)
        self._h = C.c_void_p()
        self._cb.check(lib().mic_hip_mic2_reader_open(self._cb.c, None, file_len, C.byref(self._h)), "Mic2Reader")

    def info(self):
        """dict(width, height, nframes, temporal), as mic_hip_mic2_info of the whole file"""
        v = [C.c_int() for _ in range(4)]
        self._cb.check(lib().mic_hip_mic2_reader_info(self._h, *[C.byref(x) for x in v]), "Mic2Reader.info")
        w, h, n, t = (x.value for x in v)
        return dict(width=w, height=h, nframes=n, temporal=bool(t))

    def read_crops(self, xyz, cw: int, ch: int, cd: int, d_out: int, out_cap: int, spec=None):
        """as mic2_read_crops on the whole file; only the streams of the plan's frames are read, each once"""
        rc, st, stats = _read_crops(lambda a, n, d, cap, s, p: _door("mic_hip_mic2_reader_read_crops", spec)(
            self._h, a, n, cw, ch, cd, d, cap, s, p), xyz, d_out, out_cap)
        self._cb.check(rc, "Mic2Reader.read_crops")
        return st, stats

    def set_cache(self, cache: Optional["FrameCache"]) -> None:
        """mic_hip_mic2_reader_set_cache: read_crops (and mic2_readers_read_crops) then decode only the frames that are not
        resident in `cache`, and read only their streams; None detaches and drops this reader's entries.  A cache of another
        frame size raises MicError(MIC_ERR_ARGS)."""
        rc = lib().mic_hip_mic2_reader_set_cache(self._h, cache._h if cache is not None else None)
        if rc:
            _raise(rc, "Mic2Reader.set_cache")
        self._cache = cache                            # (kept alive while attached)

    def cache_probe(self, frames) -> np.ndarray:
        """bool per frame index: resident in this reader's cache; changes no state"""
        return _cache_probe(lambda t, n, r: lib().mic_hip_mic2_reader_cache_probe(self._h, t, n, r), frames, np.uint32)

    def set_timing(self, on) -> None:
        """mic_hip_mic2_reader_set_timing: read_crops then times its kernels (HIP events on the session it runs on)"""
        lib().mic_hip_mic2_reader_set_timing(self._h, int(bool(on)))

    def last_timings(self):
        """[(kernel name, device ms)] of the last timed read_crops, summed over its launch chains"""
        names = (C.c_char_p * 96)()
        ms = (C.c_float * 96)()
        k = lib().mic_hip_mic2_reader_last_timings(self._h, names, ms, 96)
        return [(names[i].decode(), float(ms[i])) for i in range(k)]

    def close(self) -> None:
        if self._h:
            lib().mic_hip_mic2_reader_close(self._h)
            self._h = C.c_void_p()
            self._cache = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def mic2_readers_read_crops(readers, xyzv, cw: int, ch: int, cd: int, d_out: int, out_cap: int, spec=None):
    """mic_hip_mic2_readers_read_crops: mic2_multi_read_crops over a sequence of Mic2Reader (volume = an index into it; an entry no
    crop names may be None and is never read).  Only the streams of the plan's frames are read, each once."""
    readers = list(readers)
    hs = np.asarray([(r._h.value or 0) if r is not None else 0 for r in readers], dtype=np.uintp)
    rc, st, bad, stats = _read_multi_crops(lambda a, n, d, cap, s, b, p: _door("mic_hip_mic2_readers_read_crops", spec)(
        hs.ctypes.data, len(readers), a, n, cw, ch, cd, d, cap, s, b, p), xyzv, d_out, out_cap)
    for r in readers:                                  # an exception a source raised comes first
        if r is not None and r._cb.exc is not None:
            r._cb.check(rc, "mic2_readers_read_crops")
    if rc:
        _raise(rc, "mic2_readers_read_crops")
    return st, bad, stats


# ------------------------------------------------------------------ gradient predictor, PICA
def compress_single_frame_grad(pixels, width: int, height: int, max_value: int) -> bytes:
    """CompressSingleFrameGrad (multiframecompress.go:111)."""
    px = np.ascontiguousarray(pixels, dtype=np.uint16).reshape(-1)
    if px.size != width * height:
        raise MicError(MIC_ERR_ARGS, "compress_single_frame_grad")
    cap = _frame_bound(px.size)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().mic_hip_compress_frame_grad(px.ctypes.data, width, height, max_value, out.ctypes.data, cap, C.byref(n))
    if rc:
        _raise(rc, "compress_single_frame_grad")
    return out[: n.value].tobytes()


def decompress_single_frame_grad(compressed, width: int, height: int) -> np.ndarray:
    """DecompressSingleFrameGrad (multiframecompress.go:132)."""
    c = _bytes_arr(compressed)
    out = np.empty(width * height, dtype=np.uint16)
    rc = lib().mic_hip_decompress_frame_grad(c.ctypes.data, c.size, out.ctypes.data, width, height)
    if rc:
        _raise(rc, "decompress_single_frame_grad")
    return out.reshape(height, width)


def _raise_strip(rc: int, where: str, strip: int):
    """a strip's error carries its index, as the reference's "pica: strip %d: %w" does: MicError.strip"""
    try:
        _raise(rc, where + (f": strip {strip}" if strip >= 0 else ""))
    except MicError as e:
        e.strip = strip
        raise


def pica_bound(width: int, height: int, num_strips: int) -> int:
    """MIC_HIP_PICA_BOUND"""
    ns = max(num_strips, 1)
    return 16 + 16 * ns + 4 * width * height + 135168 * ns


def compress_parallel_strips_adaptive(pixels, width: int, height: int, max_value: int, num_strips: int) -> bytes:
    """CompressParallelStripsAdaptive (parallelstripsadaptive.go:54); a strip's error carries its index (:110): MicError.strip."""
    px = np.ascontiguousarray(pixels, dtype=np.uint16).reshape(-1)
    if px.size != width * height:
        raise MicError(MIC_ERR_ARGS, "compress_parallel_strips_adaptive")
    cap = pica_bound(width, height, num_strips)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0); bad = C.c_int(-1)
    rc = lib().mic_hip_pica_compress_ex(px.ctypes.data, width, height, max_value, num_strips, out.ctypes.data, cap, C.byref(n), C.byref(bad))
    if rc:
        _raise_strip(rc, "compress_parallel_strips_adaptive", bad.value)
    return out[: n.value].tobytes()


def decompress_parallel_strips_adaptive(compressed) -> np.ndarray:
    """DecompressParallelStripsAdaptive (parallelstripsadaptive.go:141): (height, width) uint16."""
    c = _bytes_arr(compressed)
    w, h, n = C.c_int(), C.c_int(), C.c_int()
    rc = lib().mic_hip_pica_info(c.ctypes.data, c.size, C.byref(w), C.byref(h), C.byref(n))
    if rc:
        _raise(rc, "decompress_parallel_strips_adaptive")
    out = np.empty(w.value * h.value, dtype=np.uint16)
    bad = C.c_int(-1)
    rc = lib().mic_hip_pica_decompress_ex(c.ctypes.data, c.size, out.ctypes.data, w.value, h.value, C.byref(bad))
    if rc:
        _raise_strip(rc, "decompress_parallel_strips_adaptive", bad.value)
    return out.reshape(h.value, w.value)


def compress_parallel_strips_adaptive_batch(images: Sequence[np.ndarray], max_value, num_strips,
                                            outs: Optional[Sequence[np.ndarray]] = None) -> List[Tuple[int, "np.ndarray"]]:
    """Many images, one call (mic_hip_pica_compress_batch): [(status, file bytes as a uint8 view of its out buffer)].
    images: (height, width) uint16 arrays (ordinary or pinned memory); max_value, num_strips: one value, or one per image;
    outs: caller buffers of >= pica_bound bytes, or None."""
    jobs, outs = _encode_batch("compress_parallel_strips_adaptive_batch", "mic_hip_pica_compress_batch", PicaEncJob, images,
                               lambda i, a: pica_bound(a.shape[1], a.shape[0], num_strips[i] if np.ndim(num_strips) else num_strips), outs,
                               max_value=max_value, num_strips=num_strips)
    compress_parallel_strips_adaptive_batch.failed_strips = [j.failed_strip for j in jobs]   # (of the last call: index of each job's failing strip, -1)
    return [(j.status, o[: j.out_len]) for j, o in zip(jobs, outs)]


def decompress_parallel_strips_adaptive_batch(files: Sequence, dims: Sequence[Tuple[int, int]],
                                              outs: Optional[Sequence[np.ndarray]] = None) -> List[Tuple[int, "np.ndarray"]]:
    """Many PICA files, one call (mic_hip_pica_decompress_batch): [(status, (height, width) uint16 pixels)]; dims: (width, height)."""
    jobs, imgs = _decode_batch("decompress_parallel_strips_adaptive_batch", "mic_hip_pica_decompress_batch", PicaDecJob, files, dims, outs)
    decompress_parallel_strips_adaptive_batch.failed_strips = [j.failed_strip for j in jobs]
    return [(j.status, im) for j, im in zip(jobs, imgs)]


def pica_boundaries(pixels, num_strips: int, on_host: bool = False) -> List[int]:
    """adaptiveStripBoundaries (parallelstripsadaptive.go:222) of a (height, width) image: the device's partition kernel, or
    (on_host) the reference's float64 loop fed with the device's row costs."""
    px = _u16(pixels)
    h, w = px.shape
    starts = np.zeros(max(min(num_strips, h), 1), dtype=np.int32)
    n = C.c_int(0)
    rc = lib().mic_hip_pica_boundaries(px.ctypes.data, w, h, num_strips, 1 if on_host else 0, starts.ctypes.data, starts.size, C.byref(n))
    if rc:
        _raise(rc, "pica_boundaries")
    return [int(v) for v in starts[: n.value]]


# ------------------------------------------------------------------ single-frame RGB, MIC1 / MICR files
def compress_rgb(rgb, width: int, height: int, container: bool = False) -> bytes:
    """CompressRGB (rgbcompress.go:25); container=True wraps it as a MICR file (cmd/mic-compress/main.go:62-91)."""
    px = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1)
    if px.size != width * height * 3:
        raise MicError(MIC_ERR_ARGS, "compress_rgb")
    cap = px.size * 4 + 4096
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    fn = lib().mic_hip_micr_compress if container else lib().mic_hip_rgb_compress
    rc = fn(px.ctypes.data, width, height, out.ctypes.data, cap, C.byref(n))
    if rc:
        _raise(rc, "compress_rgb")
    return out[: n.value].tobytes()


def decompress_rgb(compressed, width: int = 0, height: int = 0) -> np.ndarray:
    """DecompressRGB (rgbcompress.go:31) when width / height are given, else a MICR file: (h, w, 3) uint8."""
    c = _bytes_arr(compressed)
    if width and height:
        out = np.empty(width * height * 3, dtype=np.uint8)
        rc = lib().mic_hip_rgb_decompress(c.ctypes.data, c.size, width, height, out.ctypes.data, out.size)
    else:
        w, h = C.c_int(), C.c_int()
        rc = lib().mic_hip_micr_info(c.ctypes.data, c.size, C.byref(w), C.byref(h))
        if rc:
            _raise(rc, "decompress_rgb")
        width, height = w.value, h.value
        out = np.empty(width * height * 3, dtype=np.uint8)
        rc = lib().mic_hip_micr_decompress(c.ctypes.data, c.size, out.ctypes.data, out.size)
    if rc:
        _raise(rc, "decompress_rgb")
    return out.reshape(height, width, 3)


def rgb_bound(width: int, height: int, container: bool = False) -> int:
    """MIC_HIP_RGB_BOUND: three raw planes behind the three lengths (+ the 12-byte header of a MICR file)"""
    return 12 + 3 * (1 + 2 * width * height) + (12 if container else 0)


def compress_rgb_batch(images: Sequence[np.ndarray], container=False,
                       outs: Optional[Sequence[np.ndarray]] = None) -> List[Tuple[int, "np.ndarray"]]:
    """Many RGB images, one call (mic_hip_rgb_compress_batch): [(status, CompressRGB blob / MICR file as a uint8 view of its out
    buffer)].  images: (height, width, 3) uint8 arrays of any sizes (ordinary or pinned memory); container: one value, or one per
    image; outs: caller buffers of >= rgb_bound bytes, or None.  compress_rgb_batch.failed_planes: of the last call, the plane
    each job's error is about (0 Y, 1 Co, 2 Cg; -1 none)."""
    n = len(images)
    arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a in images]
    for a in arrs:
        if a.ndim != 3 or a.shape[2] != 3:
            raise MicError(MIC_ERR_ARGS, "compress_rgb_batch")
    cont = [bool(c) for c in container] if np.ndim(container) else [bool(container)] * n
    if outs is None:
        outs = [np.empty(rgb_bound(a.shape[1], a.shape[0], c), dtype=np.uint8) for a, c in zip(arrs, cont)]
    jobs = (RgbEncJob * n)()
    for i, a in enumerate(arrs):
        jobs[i].rgb = a.ctypes.data; jobs[i].width = a.shape[1]; jobs[i].height = a.shape[0]; jobs[i].container = int(cont[i])
        jobs[i].out = outs[i].ctypes.data; jobs[i].out_cap = outs[i].size
    rc = lib().mic_hip_rgb_compress_batch(jobs, n)
    if rc:
        _raise(rc, "compress_rgb_batch")
    compress_rgb_batch.failed_planes = [j.failed_plane for j in jobs]
    return [(j.status, o[: j.out_len]) for j, o in zip(jobs, outs)]


def decompress_rgb_batch(files: Sequence, dims: Optional[Sequence] = None,
                         outs: Optional[Sequence[np.ndarray]] = None) -> List[Tuple[int, Optional["np.ndarray"]]]:
    """Many CompressRGB blobs / MICR files, one call (mic_hip_rgb_decompress_batch): [(status, (height, width, 3) uint8 pixels)].
    dims = None: every file is a MICR file; else dims[i] = (width, height) of blob i, or None for a MICR file.  A MICR file whose
    header cannot be read fails its job without a buffer (pixels None).  decompress_rgb_batch.failed_planes: as compress_rgb_batch."""
    n = len(files)
    cs = [_bytes_arr(f) for f in files]
    dims = list(dims) if dims is not None else [None] * n
    shape = []
    for c, d in zip(cs, dims):
        if d is None:
            w, h = C.c_int(), C.c_int()
            shape.append((w.value, h.value) if lib().mic_hip_micr_info(c.ctypes.data, c.size, C.byref(w), C.byref(h)) == 0 else None)
        else:
            shape.append((int(d[0]), int(d[1])))
    if outs is None:
        outs = [np.empty(max(sh[0] * sh[1] * 3, 1) if sh else 1, dtype=np.uint8) for sh in shape]
    jobs = (RgbDecJob * n)()
    for i in range(n):
        jobs[i].compressed = cs[i].ctypes.data; jobs[i].compressed_len = cs[i].size
        jobs[i].rgb_out = outs[i].ctypes.data; jobs[i].out_cap = outs[i].size
        jobs[i].container = 1 if dims[i] is None else 0
        jobs[i].width, jobs[i].height = (0, 0) if dims[i] is None else shape[i]
    rc = lib().mic_hip_rgb_decompress_batch(jobs, n)
    if rc:
        _raise(rc, "decompress_rgb_batch")
    decompress_rgb_batch.failed_planes = [j.failed_plane for j in jobs]
    return [(j.status, o[: sh[0] * sh[1] * 3].reshape(sh[1], sh[0], 3) if (sh and j.status == 0) else None) for j, o, sh in zip(jobs, outs, shape)]


def write_mic1(pixels, width: int, height: int, max_value: int, nstates: int = 2) -> bytes:
    """The CLI's single-frame .mic file (writeMicFile, cmd/mic-compress/main.go:26-59)."""
    px = np.ascontiguousarray(pixels, dtype=np.uint16).reshape(-1)
    if px.size != width * height:
        raise MicError(MIC_ERR_ARGS, "write_mic1")
    cap = _frame_bound(px.size) + 20
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    rc = lib().mic_hip_mic1_compress(px.ctypes.data, width, height, max_value, nstates, out.ctypes.data, cap, C.byref(n))
    if rc:
        _raise(rc, "write_mic1")
    return out[: n.value].tobytes()


def read_mic1(compressed) -> np.ndarray:
    c = _bytes_arr(compressed)
    w, h = C.c_int(), C.c_int()
    rc = lib().mic_hip_mic1_info(c.ctypes.data, c.size, C.byref(w), C.byref(h))
    if rc:
        _raise(rc, "read_mic1")
    out = np.empty(w.value * h.value, dtype=np.uint16)
    rc = lib().mic_hip_mic1_decompress(c.ctypes.data, c.size, out.ctypes.data, out.size)
    if rc:
        _raise(rc, "read_mic1")
    return out.reshape(h.value, w.value)


# ------------------------------------------------------------------ device-resident sessions
class Session:
    """mic_hip_session: encode/decode units that already live in HBM.  Device pointers are
    plain integers (e.g. ``torch.Tensor.data_ptr()``); torch itself is not needed here."""

    def __init__(self, max_units: int, max_px_per_unit: int, device: Optional[int] = None):
        """device = None: the default session's device (mic_hip_set_device); an int: that HIP device -- one host process can
        hold a session per GPU (mic_hip_session_create_on)."""
        self._h = C.c_void_p()
        if device is None:
            rc = lib().mic_hip_session_create(C.byref(self._h), max_units, max_px_per_unit)
        else:
            rc = lib().mic_hip_session_create_on(int(device), C.byref(self._h), max_units, max_px_per_unit)
        if rc:
            _raise(rc, "session_create")
        self._n = 0

    @property
    def device(self) -> int:
        return lib().mic_hip_session_device(self._h)

    def close(self):
        if self._h:
            lib().mic_hip_session_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return lib().mic_hip_session_stream(self._h) or 0

    def set_timing(self, on):
        """False / 0: off; True / 1: per-kernel HIP-event timing of the next launch chain; 2: summed over every launch chain
        until the next set_timing (calls that run several chains: slabs of a slide, a wavelet pass)."""
        lib().mic_hip_session_set_timing(self._h, int(on))

    def last_timings(self):
        names = (C.c_char_p * 96)()
        ms = (C.c_float * 96)()
        k = lib().mic_hip_session_last_timings(self._h, names, ms, 96)
        return [(names[i].decode(), float(ms[i])) for i in range(k)]

    @staticmethod
    def make_units(units: Sequence[Tuple[int, int, int, int, int]]):
        arr = (Unit * len(units))()
        for i, (off, w, h, mv, ns) in enumerate(units):
            arr[i].px_offset = off; arr[i].width = w; arr[i].height = h; arr[i].max_value = mv; arr[i].nstates = ns
        return arr

    def encode_enqueue(self, d_pixels: int, units):
        rc = lib().mic_hip_session_encode_enqueue(self._h, d_pixels, units, len(units))
        if rc:
            _raise(rc, "session_encode_enqueue")
        self._n = len(units)

    # (results land in numpy arrays the library writes straight into: building them element by element from ctypes arrays -- and the
    # offset table of decode_enqueue from a Python list -- was 0.4 ms of host time per step of 2304 units with the device idle)
    def encode_finish(self):
        n = self._n
        offs = np.empty(n + 1, dtype=np.uint64); st = np.empty(n, dtype=np.int32); ns = np.empty(n, dtype=np.int32)
        d = C.c_void_p()
        rc = lib().mic_hip_session_encode_finish(self._h, C.byref(d), offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 st.ctypes.data_as(C.POINTER(C.c_int32)), ns.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc:
            _raise(rc, "session_encode_finish")
        return d.value, offs, st, ns

    def decode_enqueue(self, d_blobs: int, offsets: np.ndarray, units, d_pixels_out: int):
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        if offs.size < len(units) + 1:
            raise ValueError("decode_enqueue: offsets must hold len(units) + 1 entries")
        rc = lib().mic_hip_session_decode_enqueue(self._h, d_blobs, offs.ctypes.data_as(C.POINTER(C.c_uint64)), units, len(units), d_pixels_out)
        if rc:
            _raise(rc, "session_decode_enqueue")
        self._n = len(units)

    def decode_finish(self) -> np.ndarray:
        st = np.empty(self._n, dtype=np.int32)
        rc = lib().mic_hip_session_decode_finish(self._h, st.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc:
            _raise(rc, "session_decode_finish")
        return st

    # ---- digests, verify, verified encode (include/mic_hip.h, "verified encode") -----------------------------------------
    def encode(self, d_pixels: int, units):
        """encode_enqueue + encode_finish: (d_blobs, offsets, status, nstates)"""
        self.encode_enqueue(d_pixels, units)
        return self.encode_finish()

    def decode(self, d_blobs: int, offsets: np.ndarray, units, d_pixels_out: int) -> np.ndarray:
        """decode_enqueue + decode_finish: status per unit"""
        self.decode_enqueue(d_blobs, offsets, units, d_pixels_out)
        return self.decode_finish()

    def digest(self, d_pixels: int, units) -> np.ndarray:
        """mic_hip_session_digest: the CRC-32 (zlib.crc32 of the little-endian bytes) of every unit's pixels, taken on the device"""
        crc = np.empty(len(units), dtype=np.uint32)
        rc = lib().mic_hip_session_digest(self._h, d_pixels, units, len(units), crc.ctypes.data)
        if rc:
            _raise(rc, "session_digest")
        return crc

    def verify(self, d_blobs: int, offsets: np.ndarray, units, d_pixels_ref: int) -> List[VerifyResult]:
        """mic_hip_session_verify: the streams decoded into the session's scratch and compared with the reference pixels"""
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        if offs.size < len(units) + 1:
            raise ValueError("verify: offsets must hold len(units) + 1 entries")
        res = (VerifyResult * len(units))()
        rc = lib().mic_hip_session_verify(self._h, d_blobs, offs.ctypes.data_as(C.POINTER(C.c_uint64)), units, len(units), d_pixels_ref, res)
        if rc:
            _raise(rc, "session_verify")
        return list(res)

    def encode_verified(self, d_pixels: int, units):
        """mic_hip_session_encode_verified: encode, then the packed streams decoded and compared with d_pixels --
        (d_blobs, offsets, nstates, [VerifyResult]); blobs, offsets and nstates are encode's, byte for byte."""
        n = len(units)
        offs = np.empty(n + 1, dtype=np.uint64); ns = np.empty(n, dtype=np.int32)
        res = (VerifyResult * n)()
        d = C.c_void_p()
        rc = lib().mic_hip_session_encode_verified(self._h, d_pixels, units, n, C.byref(d), offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   ns.ctypes.data_as(C.POINTER(C.c_int32)), res)
        if rc:
            _raise(rc, "session_encode_verified")
        self._n = n
        return d.value, offs, ns, list(res)

    # ---- RGB images on the device (rgbcompress.go:25-33) ----------------------------------------------------------------
    @staticmethod
    def make_rgb_images(images: Sequence[Tuple[int, int, int]]):
        """images: (byte offset of the image's RGB, width, height) each -> the mic_hip_rgb_image table"""
        arr = (RgbImage * len(images))()
        for i, (off, w, h) in enumerate(images):
            arr[i].rgb_off = off; arr[i].width = w; arr[i].height = h
        return arr

    def rgb_encode(self, d_rgb: int, images):
        """mic_hip_session_rgb_encode: images = make_rgb_images(...) (or the tuples), their RGB at d_rgb + offset on the session's
        device -> (device pointer of the CompressRGB blobs, offsets[n + 1], status[n], failed_plane[n]); the blobs stay in the
        session until its next call"""
        tab = images if isinstance(images, C.Array) else self.make_rgb_images(images)
        n = len(tab)
        offs = np.zeros(n + 1, dtype=np.uint64); st = np.zeros(n, dtype=np.int32); fp = np.full(n, -1, dtype=np.int32)
        d = C.c_void_p()
        rc = lib().mic_hip_session_rgb_encode(self._h, d_rgb, tab, n, C.byref(d), offs.ctypes.data, st.ctypes.data, fp.ctypes.data)
        if rc:
            _raise(rc, "session_rgb_encode")
        return d.value, offs, st, fp

    def rgb_decode(self, d_blobs: int, offsets: np.ndarray, images, d_rgb_out: int):
        """mic_hip_session_rgb_decode: blob i at d_blobs + offsets[i] .. offsets[i + 1] -> image i's pixels at d_rgb_out + its offset
        -> (status[n], failed_plane[n])"""
        tab = images if isinstance(images, C.Array) else self.make_rgb_images(images)
        n = len(tab)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        if offs.size < n + 1:
            raise ValueError("rgb_decode: offsets must hold len(images) + 1 entries")
        st = np.zeros(n, dtype=np.int32); fp = np.full(n, -1, dtype=np.int32)
        rc = lib().mic_hip_session_rgb_decode(self._h, d_blobs, offs.ctypes.data, tab, n, d_rgb_out, st.ctypes.data, fp.ctypes.data)
        if rc:
            _raise(rc, "session_rgb_decode")
        return st, fp

    def rgb_read_crops(self, d_blobs: int, offsets: np.ndarray, images, xyf, cw: int, ch: int, d_out: int, out_cap: int, spec=None):
        """rgb_read_crops of CompressRGB blobs that lie on the session's device as rgb_encode leaves them: file f at
        d_blobs + offsets[f] .. offsets[f + 1], images = make_rgb_images(...) (or the tuples; only width and height are read).
        The heads of the named blobs are read by a kernel and the blobs go device to device."""
        tab = images if isinstance(images, C.Array) else self.make_rgb_images(images)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        if offs.size < len(tab) + 1:
            raise ValueError("rgb_read_crops: offsets must hold len(images) + 1 entries")
        rc, st, bad, stats = _read_rgb_crops(lambda a, n, d, cap, s, b, p: _door("mic_hip_session_rgb_read_crops", spec)(
            self._h, int(d_blobs) or None, offs.ctypes.data, tab, len(tab), a, n, cw, ch, d, cap, s, b, p), xyf, d_out, out_cap)
        if rc:
            _raise(rc, "session_rgb_read_crops")
        return st, bad, stats

    # ---- WaveletV2 on device-resident frames (waveletfsecompressu16.go:303-534) -------------------------------------------
    def wavelet_v2_encode(self, d_frames: int, nframes: int, rows: int, cols: int, levels: int = 5):
        """-> (device pointer of the packed header-less streams, offsets[nframes + 1], status[nframes], levels applied)"""
        d = C.c_void_p(); offs = (C.c_uint64 * (nframes + 1))(); st = (C.c_int32 * nframes)(); ap = C.c_int(0)
        rc = lib().mic_hip_session_wavelet_v2_encode(self._h, d_frames, nframes, rows, cols, levels, C.byref(d), offs, st, C.byref(ap))
        if rc:
            _raise(rc, "session_wavelet_v2_encode")
        return d.value, np.array(offs[:], dtype=np.uint64), np.array(st[:], dtype=np.int32), ap.value

    def wavelet_v2_decode(self, d_streams: int, offsets: np.ndarray, nframes: int, rows: int, cols: int, levels: int, d_pixels_out: int) -> np.ndarray:
        offs = (C.c_uint64 * len(offsets))(*[int(v) for v in offsets]); st = (C.c_int32 * nframes)()
        rc = lib().mic_hip_session_wavelet_v2_decode(self._h, d_streams, offs, nframes, rows, cols, levels, d_pixels_out, st)
        if rc:
            _raise(rc, "session_wavelet_v2_decode")
        return np.array(st[:], dtype=np.int32)

    def wavelet_v2_decode_level(self, d_streams: int, offsets: np.ndarray, nframes: int, rows: int, cols: int, levels: int, level: int,
                                d_pixels_out: int):
        """wavelet_v2_decode at resolution `level`: frame i's nr x nc band (wavelet_v2_level_info) to d_pixels_out + i * nr * nc u16.
        -> (status[nframes], tANS symbols decoded per frame)"""
        offs = (C.c_uint64 * len(offsets))(*[int(v) for v in offsets]); st = (C.c_int32 * nframes)()
        syms = np.zeros(nframes, dtype=np.uint64)
        rc = lib().mic_hip_session_wavelet_v2_decode_level(self._h, d_streams, offs, nframes, rows, cols, levels, int(level), d_pixels_out, st,
                                                           syms.ctypes.data)
        if rc:
            _raise(rc, "session_wavelet_v2_decode_level")
        return np.array(st[:], dtype=np.int32), syms

    def wavelet_v2_encode_mixed(self, d_frames: int, px_offsets, rows_cols, levels: int = 5):
        """mic_hip_session_wavelet_v2_encode_mixed: frame i = rows_cols[i] uint16 at d_frames + px_offsets[i] elements, any shapes, ONE
        launch chain.  -> (device pointer of the packed header-less streams, offsets[n + 1], status[n], levels applied[n])"""
        rc_ = np.ascontiguousarray(np.asarray(rows_cols, dtype=np.int64).reshape(-1, 2).astype(np.int32))
        n = len(rc_)
        po = np.ascontiguousarray(px_offsets, dtype=np.uint64)
        if po.size < n:
            raise ValueError("wavelet_v2_encode_mixed: px_offsets must hold one entry per frame")
        d = C.c_void_p(); offs = np.zeros(n + 1, dtype=np.uint64); st = np.zeros(n, dtype=np.int32); ap = np.zeros(n, dtype=np.int32)
        rc = lib().mic_hip_session_wavelet_v2_encode_mixed(self._h, d_frames, po.ctypes.data, rc_.ctypes.data, n, int(levels), C.byref(d),
                                                           offs.ctypes.data, st.ctypes.data, ap.ctypes.data)
        if rc:
            _raise(rc, "session_wavelet_v2_encode_mixed")
        return d.value, offs, st, ap

    def wavelet_v2_decode_mixed(self, d_streams: int, offsets, rows_cols_levels, d_pixels_out: int, out_offsets, level=None):
        """mic_hip_session_wavelet_v2_decode_mixed: stream i (offsets[i] .. offsets[i + 1]) of a frame of rows_cols_levels[i], wanted at
        level[i] (None: all 0), to d_pixels_out + out_offsets[i] elements.  -> (status[n], tANS symbols decoded per frame)"""
        rcl = np.ascontiguousarray(np.asarray(rows_cols_levels, dtype=np.int64).reshape(-1, 3).astype(np.int32))
        n = len(rcl)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64); oo = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        if offs.size < n + 1 or oo.size < n:
            raise ValueError("wavelet_v2_decode_mixed: offsets must hold n + 1 entries, out_offsets n")
        lv = None if level is None else np.ascontiguousarray(level, dtype=np.int32)
        st = np.zeros(n, dtype=np.int32); syms = np.zeros(n, dtype=np.uint64)
        rc = lib().mic_hip_session_wavelet_v2_decode_mixed(self._h, d_streams, offs.ctypes.data, rcl.ctypes.data,
                                                           None if lv is None else lv.ctypes.data, n, d_pixels_out, oo.ctypes.data,
                                                           st.ctypes.data, syms.ctypes.data)
        if rc:
            _raise(rc, "session_wavelet_v2_decode_mixed")
        return st, syms

    # ---- MIC3 on a device-resident slide (wsicompress.go:27-171) ---------------------------------------------------------------
    def wsi_encode(self, d_pixels: int, width: int, height: int, channels: int = 3, bits_per_sample: int = 8,
                   tile_w: int = 0, tile_h: int = 0, levels: int = 0) -> Tuple[int, int]:
        """-> (tiles, size of the MIC3 file the coded planes make); the planes stay in the session"""
        tt = C.c_uint64(0); cb = C.c_uint64(0)
        rc = lib().mic_hip_session_wsi_encode(self._h, d_pixels, width, height, channels, bits_per_sample, tile_w, tile_h, levels, C.byref(tt), C.byref(cb))
        if rc:
            _raise(rc, "session_wsi_encode")
        self._wsi_bytes = cb.value
        return tt.value, cb.value

    def wsi_write(self, out: Optional[np.ndarray] = None):
        """WriteMIC3 around the session's coded planes: the file CompressWSI returns, as bytes -- or, with `out` (a uint8 array of
        the caller's, ordinary or pinned), written there: returns its length"""
        buf = out if out is not None else np.empty(self._wsi_bytes + 64, dtype=np.uint8)
        n = C.c_size_t(0)
        rc = lib().mic_hip_session_wsi_write(self._h, buf.ctypes.data, buf.size, C.byref(n))
        if rc:
            _raise(rc, "session_wsi_write")
        return n.value if out is not None else buf[: n.value].tobytes()

    def workspace_bytes(self) -> Tuple[int, bool]:
        """(device bytes the session holds, whether a batch has needed the tier-2 slabs)"""
        t = C.c_int(0)
        n = lib().mic_hip_session_workspace_bytes(self._h, C.byref(t))
        return int(n), bool(t.value)

    def wsi_payload(self, total_tiles: int) -> Tuple[int, int, np.ndarray]:
        """-> (device address of the container's payload, its size, tile lengths in container order); valid until the next wsi call"""
        d = C.c_void_p(0); nb = C.c_uint64(0); lens = np.zeros(max(total_tiles, 1), dtype=np.uint64)
        rc = lib().mic_hip_session_wsi_payload(self._h, C.byref(d), C.byref(nb), lens.ctypes.data, lens.size)
        if rc:
            _raise(rc, "session_wsi_payload")
        return d.value, nb.value, lens[:total_tiles].astype(np.int64)

    def wsi_levels(self) -> List[Tuple[int, int]]:
        n = C.c_int(0); w = (C.c_int * 32)(); h = (C.c_int * 32)()
        rc = lib().mic_hip_session_wsi_levels(self._h, C.byref(n), w, h, 32)
        if rc:
            _raise(rc, "session_wsi_levels")
        return [(w[i], h[i]) for i in range(n.value)]

    def wsi_decode_level(self, level: int, d_pixels_out: int, out_cap: int):
        rc = lib().mic_hip_session_wsi_decode_level(self._h, level, d_pixels_out, out_cap)
        if rc:
            _raise(rc, "session_wsi_decode_level")

    def wsi_read_patches(self, level: int, xy, pw: int, ph: int, d_out: int, out_cap: int, spec=None, scale=None):
        """wsi_read_patches from the slide wsi_encode left in the session (it stays in HBM); d_out on the session's device"""
        rc, st, stats = _read_patches("session_wsi_read_patches", lambda a, n, d, cap, s, p: _door("mic_hip_session_wsi_read_patches", spec, scale)(
            self._h, level, a, n, pw, ph, d, cap, s, p), xy, d_out, out_cap)
        if rc:
            _raise(rc, "session_wsi_read_patches")
        return st, stats

    def set_tile_cache(self, cache: Optional["TileCache"]) -> None:
        """mic_hip_session_set_tile_cache: wsi_read_patches then decodes only the tiles that are not resident in `cache`; every
        wsi_encode drops the session's entries (its slide is replaced).  None detaches."""
        rc = lib().mic_hip_session_set_tile_cache(self._h, cache._h if cache is not None else None)
        if rc:
            _raise(rc, "session_set_tile_cache")
        self._tile_cache = cache

    def tile_cache_probe(self, tiles) -> np.ndarray:
        """bool per global tile index of the session's slide: resident in its tile cache; changes no state"""
        return _cache_probe(lambda t, n, r: lib().mic_hip_session_tile_cache_probe(self._h, t, n, r), tiles)

    def mic2_read_crops(self, head, d_file: int, file_len: int, xyz, cw: int, ch: int, cd: int, d_out: int, out_cap: int, spec=None):
        """mic2_read_crops of a MIC2 file that lies on the session's device: head = its first 20 + 8 * nframes bytes (host),
        d_file = the whole file (file_len bytes) in device memory; the streams go device to device"""
        hd = _bytes_arr(head)
        rc, st, stats = _read_crops(lambda a, n, d, cap, s, p: _door("mic_hip_session_mic2_read_crops", spec)(
            self._h, hd.ctypes.data, hd.size, int(d_file) or None, int(file_len), a, n, cw, ch, cd, d, cap, s, p), xyz, d_out, out_cap)
        if rc:
            _raise(rc, "session_mic2_read_crops")
        return st, stats

    def mic2_multi_read_crops(self, heads, d_files, lens, xyzv, cw: int, ch: int, cd: int, d_out: int, out_cap: int, spec=None):
        """mic2_multi_read_crops of MIC2 files that lie on the session's device: heads[v] = the first 20 + 8 * nframes bytes of volume
        v (host; None for a volume no crop names), d_files[v] = the device address of the whole file (0 / None when none of its
        frames is needed), lens[v] its length.  The streams of the needed frames go device to device."""
        harrs, hptrs, hlens = _volume_table(heads)
        dptrs = np.asarray([int(p or 0) for p in d_files], dtype=np.uintp)
        flens = np.asarray([int(n) for n in lens], dtype=np.uintp)
        if not (len(harrs) == dptrs.size == flens.size):
            raise ValueError("heads, d_files and lens must name the same volumes")
        rc, st, bad, stats = _read_multi_crops(lambda a, n, d, cap, s, b, p: _door("mic_hip_session_mic2_multi_read_crops", spec)(
            self._h, hptrs.ctypes.data, hlens.ctypes.data, dptrs.ctypes.data, flens.ctypes.data, len(harrs), a, n, cw, ch, cd, d, cap, s, b, p),
            xyzv, d_out, out_cap)
        if rc:
            _raise(rc, "session_mic2_multi_read_crops")
        return st, bad, stats

    def mic2_encode(self, d_frames: int, vols, heads: bool = True):
        """mic_hip_session_mic2_encode: the volumes vols = [(px_off, width, height, nframes, max_value, temporal)] that lie at
        d_frames + px_off (uint16 units) on the session's device, each to a complete MIC2 file that stays there.
        -> (d_files: the device address of the files, back to back, valid until the session's next call; offsets: uint64 array of
            len(vols) + 1, file v at offsets[v] .. offsets[v + 1], empty for a failed volume; heads: per volume the first
            20 + 8 * nframes bytes of its file, None for a failed one (all None with heads=False); status and failed frame per
            volume; dict(units, slabs, volumes_done))"""
        n = len(vols)
        va = (Mic2Volume * max(n, 1))()
        for i, v in enumerate(vols):
            va[i] = Mic2Volume(int(v[0]), int(v[1]), int(v[2]), int(v[3]), int(v[4]), int(bool(v[5])))
        offs = np.zeros(n + 1, dtype=np.uint64)
        st = np.zeros(max(n, 1), dtype=np.int32)
        bad = np.full(max(n, 1), -1, dtype=np.int32)
        hb = np.zeros(sum(20 + 8 * max(int(v[3]), 0) for v in vols) + 1, dtype=np.uint8) if heads else None
        d = C.c_void_p()
        bs = Mic2BatchStats()
        rc = lib().mic_hip_session_mic2_encode(self._h, int(d_frames) or None, va, n, C.byref(d), offs.ctypes.data,
                                               None if hb is None else hb.ctypes.data, 0 if hb is None else hb.size - 1,
                                               st.ctypes.data, bad.ctypes.data, C.byref(bs))
        if rc:
            _raise(rc, "session_mic2_encode")
        hs, at = [], 0
        for i, v in enumerate(vols):
            if hb is None or st[i] != MIC_OK:
                hs.append(None)
                continue
            hs.append(hb[at: at + 20 + 8 * int(v[3])].tobytes())
            at += 20 + 8 * int(v[3])
        return d.value or 0, offs, hs, st[:n].copy(), bad[:n].copy(), _mic2_stats(bs)

    def mic2_decode(self, heads, d_files, lens, d_frames_out: int, px_off, out_cap_px: int):
        """mic_hip_session_mic2_decode: the MIC2 files that lie on the session's device -- heads[v] = the first 20 + 8 * nframes
        bytes of volume v (host), d_files[v] = the device address of the whole file, at any byte alignment, lens[v] its length --
        each to d_frames_out + px_off[v] (uint16 units) of a device buffer of out_cap_px samples.
        -> (status per volume, failed frame per volume, dict(units, slabs, volumes_done))"""
        harrs, hptrs, hlens = _volume_table(heads)
        dptrs = np.asarray([int(p or 0) for p in d_files], dtype=np.uintp)
        flens = np.asarray([int(n) for n in lens], dtype=np.uintp)
        offs = np.asarray([int(o) for o in px_off], dtype=np.uint64)
        n = len(harrs)
        if not (n == dptrs.size == flens.size == offs.size):
            raise ValueError("heads, d_files, lens and px_off must name the same volumes")
        st = np.zeros(max(n, 1), dtype=np.int32)
        bad = np.full(max(n, 1), -1, dtype=np.int32)
        bs = Mic2BatchStats()
        rc = lib().mic_hip_session_mic2_decode(self._h, hptrs.ctypes.data, hlens.ctypes.data, dptrs.ctypes.data, flens.ctypes.data, n,
                                               int(d_frames_out) or None, offs.ctypes.data, int(out_cap_px),
                                               st.ctypes.data, bad.ctypes.data, C.byref(bs))
        if rc:
            _raise(rc, "session_mic2_decode")
        return st[:n].copy(), bad[:n].copy(), _mic2_stats(bs)

    def strips_read_crops(self, heads, d_files, lens, xyf, cw: int, ch: int, d_out: int, out_cap: int, spec=None):
        """strips_read_crops of PICS / PICA files that lie on the session's device: heads[f] = strips_head(file f) (host),
        d_files[f] = the device address of the whole file, lens[f] its length.  The streams of the needed strips go device to
        device."""
        harrs, hptrs, hlens = _file_table(heads)
        dptrs = np.asarray([int(p) for p in d_files], dtype=np.uintp)
        flens = np.asarray([int(n) for n in lens], dtype=np.uintp)
        if not (len(harrs) == dptrs.size == flens.size):
            raise ValueError("heads, d_files and lens must name the same files")
        rc, st, bad, stats = _read_strip_crops(lambda a, n, d, cap, s, b, p: _door("mic_hip_session_strips_read_crops", spec)(
            self._h, hptrs.ctypes.data, hlens.ctypes.data, dptrs.ctypes.data, flens.ctypes.data, len(harrs), a, n, cw, ch, d, cap, s, b, p),
            xyf, d_out, out_cap)
        if rc:
            _raise(rc, "session_strips_read_crops")
        return st, bad, stats
