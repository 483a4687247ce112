// mic_pieces.h -- what the readers of many rectangles per call share (MIC3 patches, MIC2 crops, strip-file crops): the piece record,
// the lane layout of a piece, the gather launcher (mic_gather.hip); and the zigzag of the MIC2 temporal pipeline.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <vector>
#include "../../include/mic_hip.h"

__device__ __forceinline__ uint32_t zigzag16(int32_t v) { const uint32_t x = (uint32_t)v & 0xFFFFu; return ((x << 1) ^ ((x & 0x8000u) ? 0xFFFFu : 0u)) & 0xFFFFu; }   // deltazigzagcompressu16.go:108-111
__device__ __forceinline__ uint32_t unzigzag16(uint32_t u) { return ((u >> 1) ^ ((u & 1u) ? 0xFFFFu : 0u)) & 0xFFFFu; }                                            // :113-116

// Lanes run along x of a piece row.  A piece narrower than a wave puts 64 / lw of its rows side by side in one (lw: the power of
// two >= w, at most 64), so a 17-pixel overlap keeps 32 + 17 lanes of 64 busy instead of 17.  grid = (pieces, row chunks).
struct PieceLanes { int col, lw, row, rstep; };
__device__ __forceinline__ PieceLanes piece_lanes(int w) {
    const int sh = min(6, 32 - __clz(w - 1));                                       // (w >= 1; __clz(0) = 32: one lane per row)
    return PieceLanes{ (int)threadIdx.x & ((1 << sh) - 1), 1 << sh, (int)(threadIdx.x >> sh) + (int)blockIdx.y * (256 >> sh), (256 >> sh) * (int)gridDim.y };
}
// rows of a piece per block pass = 256 / lanes per row; grid y cuts pieces of more than 16 passes (w, h: the largest piece of the launch)
inline unsigned row_chunks(int w, int h) {
    int lw = 1;
    while (lw < w && lw < 64) lw *= 2;
    const int passes = (h + 256 / lw - 1) / (256 / lw) * ((w + 63) / 64);
    return (unsigned)std::min(16, std::max(1, passes / 16));
}

// A piece, one overlap of a rectangle of the call with a decoded unit: w x h samples from `src` samples into the sub-batch's slab
// (rows sstride apart) to `dst` samples into the output tensor (pixels for the RGB tensor; rows dstride apart).  pstride: how far
// apart the unit's planes are, which only the RGB kernel reads.  The host plans and multiplies out both places (64 bits: crop x
// depth x rows x columns passes 2^31); the kernels multiply nothing but y * stride.
// source: the rectangle's source as the multi doors index it (slide, volume, strip file; 0 in the one-source doors), which only the
// typed kernels read, to pick the affine pair.
// A piece of a tile the MIC3 tile cache holds (the kGatherPx kinds) has its source in a pixel slot instead: src is then a BYTE
// offset into the cache's arena -- slot * slot bytes + the overlap's first pixel --, sstride the tile's width in pixels, pstride unused.
struct GatherPiece { uint64_t src, dst; int32_t sstride, dstride, w, h, pstride, source; };
// A freshly decoded tile on its way into a slot of the tile cache: its planes src samples into the slab (npx each, back to back),
// the slot at device address dst.
struct CacheFill { uint64_t src, dst; uint32_t npx, pad; };

// Where the mode-aware RGB gather (RGB file crops: mic_rgb_crops.hip) finds the three planes of piece q: record q of the reader's
// own records, which lie behind the gather list.  A plane is the decoded one in the slab (at: samples from the slab's start to the
// piece's first sample), a constant that nobody materialises (value), or the raw little-endian samples of the blob where they lie in
// the compressed-input buffer (at: bytes from that buffer's start to the piece's first sample, any alignment).  Rows are the piece's
// sstride samples apart in both; the kernel reads neither src nor pstride of the piece.
enum RgbPlaneKind : uint8_t { kPlaneConst = 0, kPlaneSlab = 1, kPlaneRaw = 2 };
struct RgbPlaneSrc { uint64_t at[3]; uint16_t value[3]; uint8_t kind[3]; uint8_t pad[7]; };
static_assert(sizeof(RgbPlaneSrc) == 40, "the records travel as five u64 per piece");

// What the typed kernels (mic_gather.hip) read of a call's output description: the pair of (source, channel) is
// pair source * src_mul + channel * ch_step of affine (a, b each); plane: samples between the channels of a pixel's destination (1: interleaved,
// ph * pw: channels first), multiplied out by the host.
struct OutParams { const float *affine; int32_t src_mul, ch_step; uint32_t clamp; float lo, hi; uint64_t plane; };

struct mic_hip_session;
namespace micapi {
// A door's output description as the core reads it: a mic_hip_out_spec that mic_hip_out_spec_check has accepted (make), for sources of
// `channels` samples a pixel.  sample: bytes of an output sample; table: the pairs the kernels read, (1, 0) where the spec has none.
struct OutFormat {
    int dtype = 0; uint32_t flags = 0; int channels = 1; size_t sample = 2;
    std::vector<float> table{ 1.f, 0.f }; int32_t src_mul = 0, ch_step = 0;
    float lo = 0, hi = 0, pad = 0;
    int make(const mic_hip_out_spec *spec, int channels, int bits_per_sample, int nsources);
    bool typed() const { return dtype != 0; }                                        // (MIC_HIP_OUT_NATIVE)
    bool planar() const { return channels > 1 && (flags & 1u); }                      // (MIC_HIP_OUT_CHANNELS_FIRST)
    size_t pixel() const { return sample * (typed() ? (size_t)channels : 1); }       // bytes of a pixel (NATIVE: sample is the pixel)
    size_t table_bytes() const { return table.size() * sizeof(float); }
    uint32_t pad_bits() const;                                                       // pad in the output type, repeated to fill a dword
    OutParams params(const void *d_table, size_t plane) const {
        return OutParams{ (const float *)d_table, src_mul, ch_step, flags & 2u, lo, hi, planar() ? plane : 1 };
    }
};
// a typed tensor's base must be aligned to its sample (checked with the pointer, before anything is launched)
inline bool out_aligned(const OutFormat &o, const void *d_out) { return !o.typed() || ((size_t)d_out & (o.sample - 1)) == 0; }
// every sample of the tensor = pad (hipMemsetAsync where its bits are all zero, else one fill kernel), behind what `stream` holds
int fill_pad(hipStream_t stream, const OutFormat &o, void *d_out, size_t bytes);
// n runs of w x h x d samples of a u16 staging tensor, laid out as the output tensor, into it as o's type (MIC2 temporal volumes);
// mw x mh x md: the largest of them
struct ConvertRun { uint64_t at; int32_t w, h, d, source; };
void launch_convert(hipStream_t stream, const OutFormat &o, const void *d_table, const uint16_t *stage, const ConvertRun *runs, size_t n,
                    int mw, int mh, int md, int cw, int ch, void *out);
// Scaled MIC3 patches (the _scaled doors, mic_api_ext.hip): patch i of a group lies as sh x sw native pixels, zero outside the level,
// at pixel i * sh * sw of the staging tensor.  Its record: the part of the source rectangle inside the level, [x0, x1) x [y0, y1) in
// source coordinates (empty: a patch that is all pad), and the source whose affine pair it takes.
struct ScaledPatch { int32_t x0, x1, y0, y1, source, pad; };
// one call's geometry: pw x ph output pixels a patch out of sw x sh source pixels at num / den; pad_bits: OutFormat::pad_bits
struct ScaledGeom { int32_t pw, ph, sw, sh, num, den; uint32_t pad_bits; };
// n patches of the staging tensor (channels x bits_per_sample: the slides' sample format) area-averaged into `out`, patch after patch
// as o lays them out, behind what `stream` holds: one launch per 2^31 - 1 patches
void launch_resample(hipStream_t stream, int channels, int bits_per_sample, const OutFormat &o, const void *d_table, const void *stage,
                     const ScaledPatch *recs, size_t n, const ScaledGeom &g, void *out);
// what a piece's samples become in the tensor: u16 as they are, u8 (uint16ToBytes), three YCoCg-R planes' RGB bytes, or the same
// from planes of three kinds (RgbPlaneSrc)
// ; or, out of pixel slots of the tile cache (`slab` is then the arena): u8, u16 or interleaved RGB pixels as they are
enum GatherKind { kGatherU16, kGatherU8, kGatherRGB, kGatherRGBModes, kGatherPxU8, kGatherPxU16, kGatherPxRGB };
// what kGatherRGBModes reads beside the slab: the buffer the raw planes lie in and the pieces' records (device; record q is piece q's)
struct RgbModeArgs { const uint8_t *raw; const RgbPlaneSrc *srcs; };
// np pieces (device) of a slab -> out, behind what `stream` holds; mw x mh: the largest of them.  The one place that picks the
// kernel, cuts the rows of tall pieces over grid y (row_chunks) and the pieces over launches of at most 2^31 - 1.  dtype
// MIC_HIP_OUT_NATIVE: the native kernels, which read nothing of op; else the typed ones (one plane: kGatherU16 and kGatherU8 alike).
// modes: what kGatherRGBModes reads further, cut over the launches with the pieces.
void launch_gather(hipStream_t stream, GatherKind kind, const uint16_t *slab, const GatherPiece *pieces, size_t np, int mw, int mh, void *out,
                   int dtype = 0, const OutParams &op = OutParams{ nullptr, 0, 0, 0, 0, 0, 1 }, const RgbModeArgs &modes = RgbModeArgs{ nullptr, nullptr });
// n freshly decoded tiles (device records) of a slab into their slots, in one launch behind what `stream` holds; kind: the kGatherPx
// kind of the cache's pixels; max_px: the largest tile's pixels
void launch_cache_fill(hipStream_t stream, GatherKind kind, const uint16_t *slab, const CacheFill *fills, size_t n, size_t max_px);
// d_out of the patch and crop calls must be memory the session's device can write `need` bytes of: an allocation of that device, or
// pinned host memory (mic_hip_host_alloc, hipHostMalloc / hipHostRegister).  Asked of the runtime before anything is launched;
// *d_out becomes the address the device uses.
int patch_pointer(const mic_hip_session *s, void **d_out, size_t need);
}  // namespace micapi
