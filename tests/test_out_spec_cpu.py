"""The output description of the typed patch and crop readers, without a device: mic_hip_out_spec_check's refusals and sample
sizes, OutSpec's shapes, and the host reference (out_spec_ref.py) against hand-written values."""
import ctypes as C

import numpy as np
import pytest

import out_spec_ref as R


def _refused(mic, spec, channels=1, bits=16, nsources=1):
    with pytest.raises(mic.MicError) as e:
        mic.out_spec_check(spec, channels, bits, nsources)
    return e.value.code == mic.MIC_ERR_ARGS


def _raw(mic, **fields):
    """an OutSpec whose struct fields are overwritten as given (what the constructor would not build)"""
    s = mic.OutSpec("f32")
    for k, v in fields.items():
        setattr(s.struct, k, v)
    return s


def test_sample_bytes_for_each_dtype_and_source_format(mic):
    for dtype, nb in R.SAMPLE_BYTES.items():
        for channels, bits in ((1, 16), (1, 8), (3, 8)):
            assert mic.out_spec_check(mic.OutSpec(dtype), channels, bits) == nb, (dtype, channels, bits)
            assert mic.OutSpec(dtype).sample_bytes(channels, bits) == nb
    native = mic.OutSpec("native")
    assert mic.out_spec_check(native, 1, 16) == 2 and mic.out_spec_check(native, 1, 8) == 1 and mic.out_spec_check(native, 3, 8) == 1


def test_every_refusal(mic):
    assert _refused(mic, None)
    assert _refused(mic, _raw(mic, dtype=6)) and _refused(mic, _raw(mic, dtype=-1))
    assert _refused(mic, _raw(mic, flags=4)) and _refused(mic, _raw(mic, flags=0x80000001))
    two = [(0.5, 3.0), (2.0, -100.0)]
    assert _refused(mic, mic.OutSpec("f32", affine=two), 1, 16, 1)                  # 2 pairs: neither 1, C nor nsources * C
    assert _refused(mic, mic.OutSpec("f32", affine=two), 3, 8, 1)
    assert _refused(mic, mic.OutSpec("f32", affine=two * 2), 3, 8, 2)               # 4 of 3 or 6
    assert mic.out_spec_check(mic.OutSpec("f32", affine=two), 1, 16, 2) == 4         # one per source
    assert mic.out_spec_check(mic.OutSpec("f32", affine=two * 3), 3, 8, 2) == 4      # one per (source, channel)
    assert mic.out_spec_check(mic.OutSpec("f32", affine=two + two[:1]), 3, 8, 5) == 4   # one per channel
    assert mic.out_spec_check(mic.OutSpec("f32", affine=two[:1]), 3, 8, 5) == 4
    assert _refused(mic, _raw(mic, naffine=-1))
    assert _refused(mic, _raw(mic, naffine=1))                                       # NULL table with naffine > 0
    assert _refused(mic, mic.OutSpec("f32", clamp=(1.0, 1.0))) and _refused(mic, mic.OutSpec("f32", clamp=(2.0, 1.0)))
    assert mic.out_spec_check(mic.OutSpec("u8", clamp=(0.0, 255.0))) == 1
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert _refused(mic, mic.OutSpec("f32", affine=[(bad, 0.0)]))
        assert _refused(mic, mic.OutSpec("f32", affine=[(1.0, bad)]))
        assert _refused(mic, mic.OutSpec("f32", clamp=(bad, 1.0)))
        assert _refused(mic, mic.OutSpec("f32", clamp=(0.0, bad)))
        assert _refused(mic, mic.OutSpec("f32", pad=bad))
        assert _refused(mic, _raw(mic, clamp_lo=bad))                                 # judged with or without the CLAMP flag


def test_native_takes_nothing_else(mic):
    assert _refused(mic, mic.OutSpec("native", channels_first=True), 3, 8)
    assert _refused(mic, mic.OutSpec("native", clamp=(0.0, 1.0)))
    assert _refused(mic, mic.OutSpec("native", affine=[(1.0, 0.0)]))
    assert _refused(mic, mic.OutSpec("native", pad=1.0))
    assert _refused(mic, _raw(mic, dtype=0, clamp_hi=1.0))


def test_outspec_shape_and_struct(mic):
    s = mic.OutSpec("bf16", channels_first=True, affine=[(0.5, 3.0)] * 3, clamp=(-2.0, 2.0), pad=-1.0)
    assert s.shape(7, 5, 9, channels=3) == (7, 3, 5, 9)
    assert mic.OutSpec("bf16").shape(7, 5, 9, channels=3) == (7, 5, 9, 3)
    assert s.shape(7, 4, 5, 9) == (7, 4, 5, 9) and s.shape(2, 5, 9, channels=1) == (2, 5, 9)
    assert (s.struct.dtype, s.struct.flags, s.struct.naffine) == (4, 3, 3)
    assert (s.struct.clamp_lo, s.struct.clamp_hi, s.struct.pad) == (-2.0, 2.0, -1.0)
    table = np.ctypeslib.as_array(C.cast(s.struct.affine, C.POINTER(C.c_float)), (6,))
    assert table.tolist() == [0.5, 3.0] * 3
    assert C.sizeof(s.struct) == 32                                                  # the C struct's layout on LP64
    with pytest.raises(ValueError):
        mic.OutSpec("f64")


def test_reference_against_hand_written_values():
    for a, b in R.PAIRS:
        assert R.exact_pair(a, b), (a, b)
    assert not R.exact_pair(0.1, 0.0) and not R.exact_pair(1.0, 2.0 ** -40)
    # u8: ties to even, saturation at both ends
    v = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -7.0, 254.5, 255.5, 300.0], dtype=np.float32)
    assert R.to_bits(v, "u8").tolist() == [0, 2, 2, 4, 0, 0, 254, 255, 255]
    assert R.to_bits(np.array([65534.5, 65535.5, 70000.0, -1.0], dtype=np.float32), "u16").tolist() == [65534, 65535, 65535, 0]
    # bf16: 8 significant bits; 1 + 2^-8 is a tie and goes to the even neighbour 1.0, 1 + 3 * 2^-8 to 1 + 2^-6
    assert R.to_bits(np.array([1.0, 1.00390625, 1.01171875, -3.0], dtype=np.float32), "bf16").tolist() == [0x3F80, 0x3F80, 0x3F82, 0xC040]
    # f16: 65504 is the largest finite value; 65520 is the tie that goes to inf, and so does 65535
    assert R.to_bits(np.array([65504.0, 65519.0, 65520.0, 65535.0, -65535.0, 0.5], dtype=np.float32), "f16").tolist() == \
        [0x7BFF, 0x7BFF, 0x7C00, 0x7C00, 0xFC00, 0x3800]
    assert R.to_bits(np.array([1.0], dtype=np.float32), "f32").tolist() == [0x3F800000]
    # the affine: one rounding; the clamp behind it; pad where outside, with neither
    x = np.array([0, 1, 2048, 4095, 65535], dtype=np.uint16)
    assert R.affine_f32(x, 1.0 / 4096, -0.5).tolist() == [-0.5, -0.499755859375, 0.0, 0.499755859375, 15.499755859375]
    assert R.affine_f32(x, 0.0625, -8.0, clamp=(0.0, 255.0)).tolist() == [0.0, 0.0, 120.0, 247.9375, 255.0]
    got = R.convert(x, "u8", 0.0625, -8.0, clamp=(0.0, 255.0), pad=3.0, outside=np.array([1, 0, 0, 0, 0], dtype=bool))
    assert got.tolist() == [3, 0, 120, 248, 255]
    got = R.convert(x, "f16", pad=-3.0, outside=np.array([0, 0, 0, 0, 1], dtype=bool))
    assert got.tolist() == [0, 0x3C00, 0x6800, 0x6C00, 0xC200]                       # (4095 has twelve bits: rounds to 4096)
    R.assert_no_subnormals(got, "f16")
    with pytest.raises(AssertionError):
        R.assert_no_subnormals(np.array([0x0001], dtype=np.uint16), "f16")
    with pytest.raises(AssertionError):
        R.assert_no_subnormals(R.to_bits(np.array([1e-39], dtype=np.float32), "f32"), "f32")
