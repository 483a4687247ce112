"""Typed output of the strip-file crop readers (mic_hip_strips_read_crops_as, mic_hip_session_strips_read_crops_as; the kernels:
csrc/mic_gather.hip).  Strip files are the cheapest source, so the packing seams of every output type are tested here: the expected
tensor is the host reference (out_spec_ref.py) applied to the zero-padded sources (strip_crop_files.expected), pad where the
coordinates lie outside the image, and every comparison is array_equal on the raw bits."""
import numpy as np
import pytest

import out_spec_ref as R
import strip_crop_files as F

pytestmark = pytest.mark.gpu

PAIR = (3.0 / 256, -1.75)               # values up to 65535 (file B): u8 saturates, f16 stays finite, nothing is subnormal
WIDTHS, HEIGHTS = [1, 2, 17, 63, 64, 65], [1, 9]


@pytest.fixture(scope="module")
def files(mic, synth, gpu_ready):
    out = F.build(synth, lambda img, maxv, strips, states: mic.compress_parallel_strips(img, img.shape[1], img.shape[0], maxv, strips, states),
                  lambda img, maxv, strips: mic.compress_parallel_strips_adaptive(img, img.shape[1], img.shape[0], maxv, strips))
    for name, img, data in out:
        px = mic.decompress_parallel_strips(data)[0] if F.FILES[name][3] == "PICS" else mic.decompress_parallel_strips_adaptive(data)
        assert np.array_equal(np.asarray(px).reshape(img.shape), img), name
    return out


class Doors:
    """the file door and the session door over one list of files: call(xyf, cw, ch, d_out, out_cap, spec) -> (status, failed, stats)"""

    def __init__(self, mic, datas):
        import torch
        self.sess = mic.Session(4, 96 * 70)
        self.keep = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda() for d in datas]
        heads = [bytes(d[: F.StripFile(d).body]) if d[:4] in (b"PICS", b"PICA") else bytes(d[:64]) for d in datas]
        ptrs, lens = [t.data_ptr() for t in self.keep], [len(d) for d in datas]
        self.all = [("file", lambda xyf, cw, ch, d, cap, spec: mic.strips_read_crops(datas, xyf, cw, ch, d, cap, spec=spec)),
                    ("session", lambda xyf, cw, ch, d, cap, spec: self.sess.strips_read_crops(heads, ptrs, lens, xyf, cw, ch, d, cap, spec=spec))]

    def close(self):
        self.sess.close()


@pytest.fixture(scope="module")
def doors(mic, files):
    d = Doors(mic, [f[2] for f in files])
    yield d
    d.close()


def _pad(dtype):
    return 3.0 if dtype in ("u8", "u16") else -3.0


def _origins(files, cw, ch):
    """the helper's origins, a crop at an odd x, and one overhanging each edge of file B (odd width)"""
    h, w = files[1][1].shape
    return F.origins(files, cw, ch) + [(7, 3, 1), (-(cw // 2) - 1, 5, 1), (w - cw // 2, 5, 1), (5, -(ch // 2) - 1, 1), (5, h - ch // 2, 1)]


def _expected(files, xyf, cw, ch, dtype, a, b, clamp=None):
    """a, b: scalars, or one per crop"""
    x = F.expected(files, xyf, cw, ch)
    outside = R.outside_mask(xyf, lambda i: files[xyf[i][2]][1].shape[1], lambda i: files[xyf[i][2]][1].shape[0], cw, ch)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.ndim:
        a, b = a[:, None, None], b[:, None, None]
    want = R.convert(x, dtype, a, b, clamp=clamp, pad=_pad(dtype), outside=outside)
    R.assert_no_subnormals(want, dtype)
    return want


@pytest.mark.parametrize("cw", WIDTHS)
@pytest.mark.parametrize("ch", HEIGHTS)
def test_every_dtype_at_the_packing_seams(mic, files, doors, cw, ch):
    assert R.exact_pair(*PAIR)
    xyf = _origins(files, cw, ch)
    n = len(xyf)
    for dtype in R.DTYPES:
        want = _expected(files, xyf, cw, ch, dtype, *PAIR)
        spec = mic.OutSpec(dtype, affine=[PAIR], pad=_pad(dtype))
        for door, call in doors.all:
            buf = R.Buffer(n * ch * cw, dtype)
            st, bad, stats = call(xyf, cw, ch, buf.ptr, buf.nbytes, spec)
            got = buf.bits().reshape(n, ch, cw)
            for i in range(n):
                assert np.array_equal(got[i], want[i]), (door, dtype, cw, ch, xyf[i])
            assert (st == mic.MIC_OK).all() and (bad == -1).all() and stats["slabs"] >= 1, (door, dtype, st, stats)


@pytest.mark.parametrize("dtype", ["u16", "f16", "bf16"])
def test_a_base_two_bytes_off_the_dword(mic, files, doors, dtype):
    """the rows that store packed pairs are the other half"""
    for cw, ch in ((17, 9), (64, 9), (65, 9)):
        xyf = _origins(files, cw, ch)
        want = _expected(files, xyf, cw, ch, dtype, *PAIR)
        spec = mic.OutSpec(dtype, affine=[PAIR], pad=_pad(dtype))
        for door, call in doors.all:
            buf = R.Buffer(len(xyf) * ch * cw, dtype, skew=2)
            st, bad, stats = call(xyf, cw, ch, buf.ptr, buf.nbytes, spec)
            assert np.array_equal(buf.bits().reshape(want.shape), want), (door, dtype, cw, ch)
            assert (st == 0).all()


def test_a_misaligned_base_is_refused_before_anything_is_launched(mic, files, doors):
    cw, ch = 17, 9
    xyf = _origins(files, cw, ch)
    for dtype, skew in (("u16", 1), ("f16", 3), ("bf16", 1), ("f32", 1), ("f32", 2)):
        for door, call in doors.all:
            buf = R.Buffer(len(xyf) * ch * cw, dtype, skew=skew)
            with pytest.raises(mic.MicError) as e:
                call(xyf, cw, ch, buf.ptr, buf.nbytes, mic.OutSpec(dtype, pad=1.0))
            assert e.value.code == mic.MIC_ERR_ARGS and buf.untouched(), (door, dtype, skew)
    buf = R.Buffer(len(xyf) * ch * cw, "u8", skew=1)                       # one-byte samples go anywhere
    st, _, _ = doors.all[0][1](xyf, cw, ch, buf.ptr, buf.nbytes, mic.OutSpec("u8", affine=[PAIR], pad=3.0))
    assert np.array_equal(buf.bits().reshape(len(xyf), ch, cw), _expected(files, xyf, cw, ch, "u8", *PAIR))
    small = R.Buffer(len(xyf) * ch * cw, "f32")                             # out_cap is judged against the typed tensor
    with pytest.raises(mic.MicError) as e:
        doors.all[0][1](xyf, cw, ch, small.ptr, small.nbytes - 1, mic.OutSpec("f32"))
    assert e.value.code == mic.MIC_ERR_CAPACITY and small.untouched()


def test_native_spec_and_no_spec_are_the_native_door(mic, files, doors):
    cw, ch = 33, 9
    xyf = F.origins(files, cw, ch)
    want = F.expected(files, xyf, cw, ch)
    for door, call in doors.all:
        base = None
        for spec in (None, mic.OutSpec("native")):
            buf = R.Buffer(len(xyf) * ch * cw, "u16")
            st, bad, stats = call(xyf, cw, ch, buf.ptr, buf.nbytes, spec)
            got = buf.bits().reshape(want.shape)
            assert np.array_equal(got, want), door
            if base is None:
                base = (st.tolist(), bad.tolist(), stats)
            assert (st.tolist(), bad.tolist(), stats) == base, door
    with pytest.raises(mic.MicError) as e:                                  # NATIVE with a flag set
        doors.all[0][1](xyf, cw, ch, 0, 0, mic.OutSpec("native", clamp=(0.0, 1.0)))
    assert e.value.code == mic.MIC_ERR_ARGS


def test_one_pair_per_file_and_a_refused_file(mic, files):
    """every file its own pair; a file whose magic is damaged is refused: its crops are pad and carry its code, all others are exact"""
    cw, ch = 33, 9
    datas = [f[2] for f in files]
    datas[3] = b"XXXX" + datas[3][4:]
    pairs = [R.PAIRS[k % len(R.PAIRS)] for k in range(len(files))]
    assert all(R.exact_pair(*p) for p in pairs) and len(set(pairs)) == len(files)
    xyf = F.origins(files, cw, ch)
    fidx = np.array([q[2] for q in xyf])
    a, b = np.array([pairs[f][0] for f in fidx]), np.array([pairs[f][1] for f in fidx])
    d = Doors(mic, datas)
    try:
        for dtype in ("f32", "bf16", "u16"):
            want = _expected(files, xyf, cw, ch, dtype, a, b)
            want[fidx == 3] = R.to_bits(np.full(1, _pad(dtype), dtype=np.float32), dtype)[0]
            spec = mic.OutSpec(dtype, affine=pairs, pad=_pad(dtype))
            for door, call in d.all:
                buf = R.Buffer(len(xyf) * ch * cw, dtype)
                st, bad, stats = call(xyf, cw, ch, buf.ptr, buf.nbytes, spec)
                got = buf.bits().reshape(want.shape)
                for i in range(len(xyf)):
                    assert np.array_equal(got[i], want[i]), (door, dtype, xyf[i])
                assert (st[fidx == 3] != mic.MIC_OK).all() and len(set(st[fidx == 3].tolist())) == 1 and (st[fidx != 3] == 0).all(), (door, st)
    finally:
        d.close()


def test_window_to_u8_with_ties_and_u16_saturation(mic, files, doors):
    """a 12-bit file through a display window to u8: x / 16 - 8 is a tie wherever x % 16 == 8; and a pair that overshoots u16"""
    cw, ch = 64, 9
    xyf = [q for q in F.origins(files, cw, ch) if q[2] == 0]               # file A, 12 bits
    x = F.expected(files, xyf, cw, ch)
    assert x.max() <= 4095
    v = R.affine_f32(x, 0.0625, -8.0, clamp=(0.0, 255.0))
    assert ((v % 1.0) == 0.5).any(), "no tie in the expected tensor"
    want = _expected(files, xyf, cw, ch, "u8", 0.0625, -8.0, clamp=(0.0, 255.0))
    spec = mic.OutSpec("u8", affine=[(0.0625, -8.0)], clamp=(0.0, 255.0), pad=3.0)
    over = [q for q in F.origins(files, cw, ch) if q[2] == 1]              # file B: values up to 65535; 2 x - 100 passes both ends
    want16 = _expected(files, over, cw, ch, "u16", 2.0, -100.0)
    assert (want16 == 65535).any() and (want16 == 0).any()
    spec16 = mic.OutSpec("u16", affine=[(2.0, -100.0)], pad=3.0)
    for door, call in doors.all:
        buf = R.Buffer(len(xyf) * ch * cw, "u8")
        st, _, _ = call(xyf, cw, ch, buf.ptr, buf.nbytes, spec)
        assert np.array_equal(buf.bits().reshape(want.shape), want) and (st == 0).all(), door
        buf = R.Buffer(len(over) * ch * cw, "u16")
        st, _, _ = call(over, cw, ch, buf.ptr, buf.nbytes, spec16)
        assert np.array_equal(buf.bits().reshape(want16.shape), want16) and (st == 0).all(), door

