"""The host reference of the typed output of the patch and crop readers (mic_hip_out_spec, include/mic_hip.h), shared by
test_out_spec_cpu.py, the test_gpu_typed_*.py files and typed_chunking_check.py.  Nothing here calls the code under test.

The kernels compute v = fmaf(x, a, b) with one rounding.  Here x * a + b is computed in float64 and rounded once to float32, which is
the same value bit for bit whenever the float64 result is exact: x is an integer below 2^16, so pairs whose a and b have at most 12
significant bits and exponents a dozen or so apart keep every bit of the product and of the sum inside float64's 53 (exact_pair).
The clamp is float32's; f16 and bf16 are torch's CPU casts (round to nearest even from f32); u8 and u16 are np.rint (ties to even) and saturation."""
import numpy as np

# (a, b): at most 12 significant bits each, exponents close together
PAIRS = [(1.0 / 4096, -0.5), (0.0244140625, -1024.0), (3.0 / 256, -1.75), (0.0625, -8.0), (0.5, 3.0), (2.0, -100.0)]

DTYPES = ["u8", "u16", "f16", "bf16", "f32"]
SAMPLE_BYTES = {"u8": 1, "u16": 2, "f16": 2, "bf16": 2, "f32": 4}
BITS_DTYPE = {"u8": np.uint8, "u16": np.uint16, "f16": np.uint16, "bf16": np.uint16, "f32": np.uint32}


def exact_pair(a, b):
    """a and b have at most 12 significant bits, and from the lowest bit x * a or b can have (x an integer below 2^16) to the highest
    are at most 53 bits: float64 then holds x * a + b exactly"""
    def sig_exp(v):
        m, e = np.frexp(np.float64(v))
        return float(m) * 4096 == int(float(m) * 4096), int(e)
    (oka, ea), (okb, eb) = sig_exp(a), sig_exp(b)
    return oka and okb and (b == 0 or max(ea + 16, eb) - min(ea, eb) + 13 <= 53)


def affine_f32(x, a, b, clamp=None):
    """float32 array: x * a + b rounded once (a, b broadcast against x), clamped in float32"""
    v = (np.asarray(x, dtype=np.float64) * np.asarray(a, dtype=np.float64) + np.asarray(b, dtype=np.float64)).astype(np.float32)
    if clamp is not None:
        v = np.minimum(np.maximum(v, np.float32(clamp[0])), np.float32(clamp[1]))
    return v


def to_bits(v, dtype):
    """the float32 values v in the output type, as its raw bits (BITS_DTYPE[dtype])"""
    import torch
    v = np.ascontiguousarray(v, dtype=np.float32)
    if dtype == "f32":
        return v.view(np.uint32)
    if dtype == "f16":
        return torch.from_numpy(v).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    if dtype == "bf16":
        return torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    top = 255 if dtype == "u8" else 65535
    return np.clip(np.rint(v), 0, top).astype(BITS_DTYPE[dtype])


def convert(x, dtype, a=1.0, b=0.0, clamp=None, pad=0.0, outside=None):
    """the expected tensor's bits: the samples x through (a, b), the clamp and the type; where `outside` is set, pad instead
    (converted the same way, with no affine and no clamp)"""
    out = to_bits(affine_f32(x, a, b, clamp), dtype)
    if outside is not None:
        out = np.where(outside, to_bits(np.full(1, pad, dtype=np.float32), dtype)[0], out)
    return out


def assert_no_subnormals(bits, dtype):
    """no non-zero result is subnormal in the output type (denormal modes are not the feature's business)"""
    if dtype in ("u8", "u16"):
        return
    mask, shift = {"f16": (0x7C00, 0), "bf16": (0x7F80, 0), "f32": (0x7F800000, 0)}[dtype]
    b = np.asarray(bits).astype(np.uint32)
    mant = b & ~np.uint32(mask) & np.uint32(0x7FFF if dtype != "f32" else 0x7FFFFFFF)
    assert not (((b & mask) == 0) & (mant != 0)).any(), "a subnormal expected value: choose other pairs or inputs"


def torch_dtype(dtype):
    import torch
    return {"u8": torch.uint8, "u16": torch.int16, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[dtype]


def tensor_bits(t, dtype):
    """a device or host tensor of the output type (u16 held as int16) -> numpy array of its raw bits"""
    import torch
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[SAMPLE_BYTES[dtype]]
    return t.contiguous().view(view).cpu().numpy().view(BITS_DTYPE[dtype])


class Buffer:
    """a device byte buffer for `count` samples of `dtype`, pre-filled with 0xA5 (every byte must be overwritten), its tensor `skew`
    bytes behind a 256-byte-aligned address"""

    def __init__(self, count, dtype, skew=0):
        import torch
        self.dtype, self.count, self.skew = dtype, count, skew
        self.nbytes = count * SAMPLE_BYTES[dtype]
        self.raw = torch.full((self.nbytes + skew + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 256 == 0
        self.ptr = self.raw.data_ptr() + skew

    def bits(self):
        """the tensor's samples as raw bits (flat), and the bytes around it, which must still be 0xA5"""
        host = self.raw.cpu().numpy()
        assert (host[: self.skew] == 0xA5).all() and (host[self.skew + self.nbytes:] == 0xA5).all(), "wrote outside the tensor"
        return host[self.skew: self.skew + self.nbytes].copy().view(BITS_DTYPE[self.dtype])

    def untouched(self):
        return bool((self.raw == 0xA5).all().item())


def outside_mask(xy, w_of, h_of, cw, ch):
    """(len(xy), ch, cw) bool: sample (i, r, c) lies outside its image; xy[i] = (x, y, ...), w_of(i) / h_of(i) the image's size"""
    out = np.zeros((len(xy), ch, cw), dtype=bool)
    for i, q in enumerate(xy):
        cols, rows = np.arange(q[0], q[0] + cw), np.arange(q[1], q[1] + ch)
        out[i] = ((rows < 0) | (rows >= h_of(i)))[:, None] | ((cols < 0) | (cols >= w_of(i)))[None, :]
    return out
