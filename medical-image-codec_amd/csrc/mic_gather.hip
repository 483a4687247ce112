// mic_gather.hip -- what the readers of many rectangles per call share (MIC3 patches: mic_api_ext.hip, MIC2 crops: mic_mic2_crops.hip,
// strip-file crops: mic_strip_crops.hip, RGB file crops: mic_rgb_crops.hip).  Each of them plans on the host, decodes the touched
// units in sub-batches into a slab and copies the pieces, the (rectangle, unit) overlaps, out of the slab into the output tensor.
// Here: the kernels that copy and their launcher, the judgement of the output pointer, the crop doors' way to a session, and the
// packing of a sub-batch's streams; and the typed output of the _as doors (mic_hip_out_spec): its one judgement, the typed gather
// kernels, the pad fill and the convert kernel of the MIC2 temporal staging tensor; and the kernels of the MIC3 tile cache
// (mic_tile_cache.h): the fill of freshly decoded tiles into pixel slots and the gathers that read pieces out of them; and the
// resample kernel of the scaled MIC3 patch doors, which area-averages a staging tensor of native patches into the output tensor.
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>
#include <cmath>
#include <type_traits>
#include "mic_session.h"
#include "mic_pieces.h"
#include "mic_px_copy.h"

namespace {

// The piece's samples as T.  grid = (pieces, row chunks); lanes along x (piece_lanes).  16-bit samples: a row whose source and
// destination are both 4-byte aligned moves as dwords (the odd sample behind them as u16), any other row as u16 -- with an odd
// unit or rectangle width every second row is such a row.  8-bit samples: uint16ToBytes (wsicompress.go:589-603).
template <typename T>
__global__ void __launch_bounds__(256) k_gather_pieces(const uint16_t *slab, const GatherPiece *pieces, T *out) {
    const GatherPiece pc = pieces[blockIdx.x];
    const PieceLanes ln = piece_lanes(pc.w);
    const uint16_t *src = slab + pc.src;
    T *dst = out + pc.dst;
    for (int y = ln.row; y < pc.h; y += ln.rstep) {
        const mic_gp<const uint16_t> s = mic_g(src + (size_t)y * pc.sstride);
        const mic_gp<T> d = mic_g(dst + (size_t)y * pc.dstride);
        if (sizeof(T) == 2 && (((size_t)s | (size_t)d) & 3) == 0) {
            const mic_gp<const uint32_t> s2 = (mic_gp<const uint32_t>)s;
            const mic_gp<uint32_t> d2 = (mic_gp<uint32_t>)d;
            for (int x = ln.col; x < (pc.w >> 1); x += ln.lw) d2[x] = s2[x];
            if ((pc.w & 1) && ln.col == 0) d[pc.w - 1] = (T)s[pc.w - 1];
        } else
            for (int x = ln.col; x < pc.w; x += ln.lw) d[x] = (T)s[x];
    }
}

// ---- the RGB gathers: the pixel's arithmetic, the planes a piece's pixels come from, one row loop ---------------------------------
// UnZigZag of Co and Cg (deltazigzagcompressu16.go:113-116) and YCoCgRInverse (asm_amd64.go:106-121), as k_wsi_planes_to_rgb does
// them: the pixel every RGB gather writes (its channels' low bytes)
struct RgbPx { int r, g, b; };
__device__ __forceinline__ RgbPx ycocg_rgb(int yv, uint32_t uco, uint32_t ucg) {
    const int co = (int)(int16_t)((uco >> 1) ^ (uint16_t)(-(int)(uco & 1)));
    const int cg = (int)(int16_t)((ucg >> 1) ^ (uint16_t)(-(int)(ucg & 1)));
    const int t = yv - (cg >> 1);
    const int g = cg + t;
    const int b = t - (co >> 1);
    return RgbPx{ co + b, g, b };
}
// The three planes of a piece in a slab of whole units: the piece in plane 0, the other two pstride samples on each.
struct SlabPlanes {
    mic_gp<const uint16_t> py, pco, pcg;
    __device__ __forceinline__ SlabPlanes(const uint16_t *slab, const GatherPiece &pc) : py(mic_g(slab + pc.src)), pco(py + pc.pstride), pcg(pco + pc.pstride) {}
    __device__ __forceinline__ uint32_t y(size_t i) const { return py[i]; }
    __device__ __forceinline__ uint32_t co(size_t i) const { return pco[i]; }
    __device__ __forceinline__ uint32_t cg(size_t i) const { return pcg[i]; }
    __device__ __forceinline__ RgbPx px(size_t i) const { return ycocg_rgb((int)y(i), co(i), cg(i)); }
};
// The three planes of a piece by its record (RgbPlaneSrc): each the decoded plane in the slab, a constant, or the blob's raw samples
// in `raw` -- little-endian at any byte address (a Y plane's always start at an odd one), two byte loads a sample as k_rgb_batch_fill
// reads them.  The kind is the whole piece's, so a block's branches on it are uniform.
struct ModePlanes {
    struct Plane { mic_gp<const uint16_t> slab; mic_gp<const uint8_t> raw; uint32_t kind, value; };
    Plane p[3];
    __device__ __forceinline__ ModePlanes(const uint16_t *slab, const uint8_t *raw, const RgbPlaneSrc &r) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            p[k].kind = r.kind[k]; p[k].value = r.value[k];
            p[k].slab = mic_g(slab) + (r.kind[k] == kPlaneSlab ? r.at[k] : 0);
            p[k].raw = mic_g(raw) + (r.kind[k] == kPlaneRaw ? r.at[k] : 0);
        }
    }
    __device__ __forceinline__ uint32_t sample(const Plane &q, size_t i) const {
        if (q.kind == kPlaneSlab) return q.slab[i];
        if (q.kind == kPlaneRaw) return (uint32_t)q.raw[2 * i] | ((uint32_t)q.raw[2 * i + 1] << 8);
        return q.value;
    }
    __device__ __forceinline__ uint32_t y(size_t i) const { return sample(p[0], i); }
    __device__ __forceinline__ uint32_t co(size_t i) const { return sample(p[1], i); }
    __device__ __forceinline__ uint32_t cg(size_t i) const { return sample(p[2], i); }
    __device__ __forceinline__ RgbPx px(size_t i) const { return ycocg_rgb((int)y(i), co(i), cg(i)); }
};
// The pixels of a piece in a slot of the tile cache: interleaved RGB bytes, the inverse transform done when the slot was filled.
// pc.src: BYTES from the arena's start to the piece's first pixel; rows sstride pixels apart.
struct SlotPixels {
    mic_gp<const uint8_t> p;
    __device__ __forceinline__ SlotPixels(const uint8_t *arena, const GatherPiece &pc) : p(mic_g(arena + pc.src)) {}
    __device__ __forceinline__ RgbPx px(size_t i) const { return RgbPx{ p[3 * i], p[3 * i + 1], p[3 * i + 2] }; }
};
// The piece's pixels through put(d, pixel), d = y * dstride + x * px samples from the piece's place in the tensor.  Lanes along x of
// a piece row: a wave reads 64 neighbouring samples of each plane and writes 64 neighbouring pixels.
template <class Planes, class Put>
__device__ __forceinline__ void gather_rgb_rows(const GatherPiece &pc, const Planes &pl, size_t dstride, int px, Put &&put) {
    const PieceLanes ln = piece_lanes(pc.w);
    for (int y = ln.row; y < pc.h; y += ln.rstep) {
        const size_t si = (size_t)y * pc.sstride, di = (size_t)y * dstride;
        for (int x = ln.col; x < pc.w; x += ln.lw) put(di + (size_t)x * px, pl.px(si + x));
    }
}
// out: u8, three a pixel: three byte stores per pixel at whatever byte offset the tensor's row has, 192 neighbouring bytes a wave
template <class Planes>
__device__ __forceinline__ void gather_rgb_native(const GatherPiece &pc, const Planes &pl, uint8_t *out) {
    const mic_gp<uint8_t> o = mic_g(out + pc.dst * 3);
    gather_rgb_rows(pc, pl, (size_t)pc.dstride * 3, 3, [&](size_t d, RgbPx v) { o[d] = (uint8_t)v.r; o[d + 1] = (uint8_t)v.g; o[d + 2] = (uint8_t)v.b; });
}

__global__ void __launch_bounds__(256) k_gather_pieces_rgb(const uint16_t *slab, const GatherPiece *pieces, uint8_t *out) {
    const GatherPiece pc = pieces[blockIdx.x];
    gather_rgb_native(pc, SlabPlanes(slab, pc), out);
}
// ... of RGB files (CompressRGB blobs), whose slab holds the coded planes alone: no plane is filled in for a constant or a raw one
__global__ void __launch_bounds__(256) k_gather_modes_rgb(const uint16_t *slab, const uint8_t *raw, const GatherPiece *pieces, const RgbPlaneSrc *srcs, uint8_t *out) {
    const GatherPiece pc = pieces[blockIdx.x];
    gather_rgb_native(pc, ModePlanes(slab, raw, srcs[blockIdx.x]), out);
}

// ---- typed output (mic_hip_out_spec) ------------------------------------------------------------------------------------------
// The value of an output sample (include/mic_hip.h): v = fmaf(x, a, b), one rounding; clamped in f32 when the spec says so; then
// the output type's conversion of that f32 value -- round to nearest even for f16 and bf16 (overflow to inf), rintf and saturation
// for u8 and u16.  DT: the spec's dtype; its samples are stored as their bits (u8, u16 or a dword).
template <int DT> struct OutBits { typedef uint16_t type; };
template <> struct OutBits<MIC_HIP_OUT_U8> { typedef uint8_t type; };
template <> struct OutBits<MIC_HIP_OUT_F32> { typedef uint32_t type; };
template <int DT> __device__ __forceinline__ typename OutBits<DT>::type out_bits(float v) {
    if (DT == MIC_HIP_OUT_F32) return (typename OutBits<DT>::type)__float_as_uint(v);
    if (DT == MIC_HIP_OUT_F16) return (typename OutBits<DT>::type)__half_as_ushort(__float2half_rn(v));
    if (DT == MIC_HIP_OUT_BF16) return (typename OutBits<DT>::type)__bfloat16_as_ushort(__float2bfloat16(v));   // (RNE; gfx950: v_cvt_pk_bf16_f32)
    const float top = DT == MIC_HIP_OUT_U8 ? 255.f : 65535.f;
    return (typename OutBits<DT>::type)(uint32_t)fminf(fmaxf(rintf(v), 0.f), top);
}
struct Pair { float x, y; };
__device__ __forceinline__ Pair out_pair(const OutParams &o, size_t i) { const mic_gp<const float> g = mic_g(o.affine); return Pair{ g[2 * i], g[2 * i + 1] }; }
template <int DT> __device__ __forceinline__ typename OutBits<DT>::type out_sample(uint32_t x, Pair ab, const OutParams &o) {
    float v = __fmaf_rn((float)x, ab.x, ab.y);
    if (o.clamp) v = fminf(fmaxf(v, o.lo), o.hi);
    return out_bits<DT>(v);
}

// A row of w one-plane samples as DT: the lanes of piece_lanes.  2-byte outputs keep the native kernel's trick: a row whose
// destination is 4-byte aligned stores packed pairs as dwords (the odd sample behind them as one 2-byte store), any other row
// 2-byte samples; f32 is one dword per lane.
template <int DT, typename S = uint16_t>
__device__ __forceinline__ void typed_row(mic_gp<const S> s, mic_gp<typename OutBits<DT>::type> d, int w, const PieceLanes &ln, Pair ab, const OutParams &o) {
    typedef typename OutBits<DT>::type T;
    if (sizeof(T) == 2 && ((size_t)d & 3) == 0) {
        const mic_gp<uint32_t> d2 = (mic_gp<uint32_t>)d;
        for (int x = ln.col; x < (w >> 1); x += ln.lw)
            d2[x] = (uint32_t)out_sample<DT>(s[2 * x], ab, o) | ((uint32_t)out_sample<DT>(s[2 * x + 1], ab, o) << 16);
        if ((w & 1) && ln.col == 0) d[w - 1] = out_sample<DT>(s[w - 1], ab, o);
    } else
        for (int x = ln.col; x < w; x += ln.lw) d[x] = out_sample<DT>(s[x], ab, o);
}

// k_gather_pieces for a typed tensor: the same lanes and grid; the piece's pair is its source's (one plane: channel 0).  8-bit
// greyscale slides enter as the slab's u16 samples, like every other one-plane source.
template <int DT>
__global__ void __launch_bounds__(256) k_gather_typed(const uint16_t *slab, const GatherPiece *pieces, typename OutBits<DT>::type *out, const OutParams o) {
    const GatherPiece pc = pieces[blockIdx.x];
    const PieceLanes ln = piece_lanes(pc.w);
    const Pair ab = out_pair(o, (size_t)pc.source * o.src_mul);
    const uint16_t *src = slab + pc.src;
    typename OutBits<DT>::type *dst = out + pc.dst;
    for (int y = ln.row; y < pc.h; y += ln.rstep)
        typed_row<DT>(mic_g(src + (size_t)y * pc.sstride), mic_g(dst + (size_t)y * pc.dstride), pc.w, ln, ab, o);
}

// k_gather_pieces_rgb for a typed tensor: the same YCoCg-R inverse, then r, g and b through their channel's pair to the pixel's
// three places, o.plane samples apart: 1 in the interleaved tensor (pc.dst: the pixel's first sample), ph * pw in the
// channels-first one (pc.dst: the piece's place in plane 0, rows dstride samples apart).
template <int DT, class Planes>
__device__ __forceinline__ void gather_rgb_typed(const GatherPiece &pc, const Planes &pl, typename OutBits<DT>::type *out, const OutParams &o) {
    typedef typename OutBits<DT>::type T;
    const size_t a0 = (size_t)pc.source * o.src_mul;
    const Pair ar = out_pair(o, a0), ag = out_pair(o, a0 + o.ch_step), ab = out_pair(o, a0 + 2 * o.ch_step);
    const mic_gp<T> dr = mic_g(out + pc.dst), dg = dr + o.plane, db = dg + o.plane;
    gather_rgb_rows(pc, pl, (size_t)pc.dstride, o.plane == 1 ? 3 : 1, [&](size_t d, RgbPx v) {   // (px: samples from a pixel to the next of its row)
        dr[d] = out_sample<DT>((uint8_t)v.r, ar, o); dg[d] = out_sample<DT>((uint8_t)v.g, ag, o); db[d] = out_sample<DT>((uint8_t)v.b, ab, o);
    });
}
template <int DT>
__global__ void __launch_bounds__(256) k_gather_typed_rgb(const uint16_t *slab, const GatherPiece *pieces, typename OutBits<DT>::type *out, const OutParams o) {
    const GatherPiece pc = pieces[blockIdx.x];
    gather_rgb_typed<DT>(pc, SlabPlanes(slab, pc), out, o);
}
// k_gather_modes_rgb for a typed tensor
template <int DT>
__global__ void __launch_bounds__(256) k_gather_typed_modes_rgb(const uint16_t *slab, const uint8_t *raw, const GatherPiece *pieces, const RgbPlaneSrc *srcs,
                                                                typename OutBits<DT>::type *out, const OutParams o) {
    const GatherPiece pc = pieces[blockIdx.x];
    gather_rgb_typed<DT>(pc, ModePlanes(slab, raw, srcs[blockIdx.x]), out, o);
}

// ---- gathers out of pixel slots (the MIC3 tile cache, mic_tile_cache.h) -----------------------------------------------------------
// A slot holds a decoded tile as pixels of the slide's sample format, so a piece's src is a BYTE offset into the arena, its rows
// sstride pixels apart; dst and dstride count as in the slab kernels.  Native output is then a copy of w * BPP bytes per row at any
// byte alignment on both sides (mic_px_copy.h); typed output runs the arithmetic of the slab kernels on the slot's samples.
template <int BPP>
__global__ void __launch_bounds__(256) k_gather_px(const uint8_t *arena, const GatherPiece *pieces, uint8_t *out) {
    const GatherPiece pc = pieces[blockIdx.x];
    const int nb = pc.w * BPP;
    const PieceLanes ln = px_row_lanes(nb);
    const uint8_t *src = arena + pc.src;
    uint8_t *dst = out + pc.dst * BPP;
    for (int y = ln.row; y < pc.h; y += ln.rstep)
        px_row_dwords(mic_g(src + (size_t)y * pc.sstride * BPP), mic_g(dst + (size_t)y * pc.dstride * BPP), nb, ln);
}
// one plane of S samples (u8 or u16) to a typed tensor: k_gather_typed on a slot
template <int DT, typename S>
__global__ void __launch_bounds__(256) k_gather_px_typed(const uint8_t *arena, const GatherPiece *pieces, typename OutBits<DT>::type *out, const OutParams o) {
    const GatherPiece pc = pieces[blockIdx.x];
    const PieceLanes ln = piece_lanes(pc.w);
    const Pair ab = out_pair(o, (size_t)pc.source * o.src_mul);
    const S *src = (const S *)(arena + pc.src);
    typename OutBits<DT>::type *dst = out + pc.dst;
    for (int y = ln.row; y < pc.h; y += ln.rstep)
        typed_row<DT, S>(mic_g(src + (size_t)y * pc.sstride), mic_g(dst + (size_t)y * pc.dstride), pc.w, ln, ab, o);
}
// interleaved RGB bytes to a typed tensor: k_gather_typed_rgb on a slot
template <int DT>
__global__ void __launch_bounds__(256) k_gather_px_typed_rgb(const uint8_t *arena, const GatherPiece *pieces, typename OutBits<DT>::type *out, const OutParams o) {
    const GatherPiece pc = pieces[blockIdx.x];
    gather_rgb_typed<DT>(pc, SlotPixels(arena, pc), out, o);
}

// The planes of freshly decoded tiles into their slots, once, at insertion: tile blockIdx.x's npx pixels from its planes in the slab
// (src samples in, the RGB planes npx apart) to dst, the slot's device address.  P3: the YCoCg-R inverse of k_wsi_planes_to_rgb;
// else uint16ToBytes (T = u8) or the samples as they are (T = u16).  grid = (tiles, chunks).
template <typename T, bool P3>
__global__ void __launch_bounds__(256) k_cache_fill(const uint16_t *slab, const CacheFill *fills) {
    const CacheFill f = fills[blockIdx.x];
    const mic_gp<const uint16_t> p0 = mic_g(slab + f.src);
    const mic_gp<T> d = mic_g((T *)(uintptr_t)f.dst);
    for (uint32_t i = blockIdx.y * 256 + threadIdx.x; i < f.npx; i += gridDim.y * 256) {
        if (P3) {
            const RgbPx v = ycocg_rgb((int)p0[i], p0[(size_t)f.npx + i], p0[2 * (size_t)f.npx + i]);
            d[3 * (size_t)i] = (T)v.r; d[3 * (size_t)i + 1] = (T)v.g; d[3 * (size_t)i + 2] = (T)v.b;
        } else d[i] = (T)p0[i];
    }
}

// MIC2 temporal volumes: run = a crop's footprint, w x h samples of d slices from `at` of the u16 staging tensor (slices of ch x cw)
// to the same place of the typed one, through its volume's pair.  grid = (runs, row chunks, slices), the lanes of a piece: a run is
// as deep as its crop, so the slices go over grid z or a call of a few deep crops would leave most of the device idle.
template <int DT>
__global__ void __launch_bounds__(256) k_convert_runs(const uint16_t *stage, const ConvertRun *runs, typename OutBits<DT>::type *out, int cw, int ch, const OutParams o) {
    const ConvertRun rn = runs[blockIdx.x];
    const PieceLanes ln = piece_lanes(rn.w);
    const Pair ab = out_pair(o, (size_t)rn.source * o.src_mul);
    const size_t slice = (size_t)ch * cw;
    for (int z = (int)blockIdx.z; z < rn.d; z += (int)gridDim.z)
        for (int y = ln.row; y < rn.h; y += ln.rstep) {
            const size_t at = rn.at + (size_t)z * slice + (size_t)y * cw;
            typed_row<DT>(mic_g(stage + at), mic_g(out + at), rn.w, ln, ab, o);
        }
}

// ---- scaled MIC3 patches: the staging tensor's native pixels, area-averaged, to the tensor -----------------------------------------
// The value (include/mic_hip.h): output pixel (x, y) of a patch covers [x * num, (x + 1) * num) x [y * num, (y + 1) * num) in units of
// 1 / den of a source pixel, source pixel (k, l) covers [k * den, (k + 1) * den) x [l * den, (l + 1) * den); per channel
// S = sum_l wy * sum_k wx * p(k, l) over the overlaps' lengths and v = (S + num^2 / 2) / num^2.  The footprint's columns are k0 =
// x * num / den .. k1 = ((x + 1) * num - 1) / den: the first weighs (k0 + 1) * den - x * num, the last (x + 1) * num - k1 * den, every
// one between den (num >= den: a footprint never lies inside one source pixel unless it IS that pixel, num == den); rows alike.
// A row's sum stays below 1024 * 65535 < 2^26; S reaches 1024^2 * 65535 < 2^36, so 16-bit sources sum in 64 bits, 8-bit ones
// (below 2^28) in 32.  One division per output sample.
// grid = (patches, row chunks), the lanes of a piece (piece_lanes(pw)): lanes along output x.  Adjacent lanes' footprints are adjacent
// in the source row, so step t of the column loop reads addresses num / den pixels apart across the wave and the wave's whole
// span of each source row, 64 * num / den pixels, within k1 - k0 + 1 <= 17 steps: every byte of every line it touches is used, out of L1
// from the second step on.  The 3-byte source reads its bytes one by one: a lane's pixels are num / den * 3 bytes from its
// neighbour's, so no dword holds what two lanes need, and px_row_dwords' skewed dwords would be assembled per lane and pixel for
// three bytes each.  A pixel whose footprint misses the patch's part of the level is pad; the staging tensor is 0 where the level is not.
template <int DT, typename S> struct ScaledOut { typedef typename OutBits<DT>::type type; };
template <typename S> struct ScaledOut<MIC_HIP_OUT_NATIVE, S> { typedef S type; };
struct Footprint { int first, last, w_first, w_last; };     // source columns (rows) first .. last; the weights of the two ends (last > first)
__device__ __forceinline__ Footprint footprint(int j, int num, int den) {
    const int a = j * num, k0 = a / den, k1 = (a + num - 1) / den;
    return Footprint{ k0, k1, min((k0 + 1) * den, a + num) - a, a + num - k1 * den };
}
template <int DT, typename S, int C>
__global__ void __launch_bounds__(256) k_resample_patches(const S *stage, const ScaledPatch *recs, typename ScaledOut<DT, S>::type *out, const ScaledGeom g, const OutParams o) {
    typedef typename ScaledOut<DT, S>::type T;
    typedef typename std::conditional<sizeof(S) == 2, uint64_t, uint32_t>::type Acc;
    const ScaledPatch rp = recs[blockIdx.x];
    const PieceLanes ln = piece_lanes(g.pw);
    const mic_gp<const S> src = mic_g(stage + (size_t)blockIdx.x * (size_t)g.sh * (size_t)g.sw * C);
    const size_t area = (size_t)g.ph * (size_t)g.pw;
    const mic_gp<T> dst = mic_g(out + (size_t)blockIdx.x * area * C);
    const bool planar = C > 1 && DT != MIC_HIP_OUT_NATIVE && o.plane != 1;
    const size_t cstep = planar ? area : 1;
    Pair ab[C];
    if (DT != MIC_HIP_OUT_NATIVE) {
#pragma unroll
        for (int c = 0; c < C; c++) ab[c] = out_pair(o, (size_t)rp.source * o.src_mul + (size_t)c * o.ch_step);
    }
    const Acc nn = (Acc)g.num * (Acc)g.num, half = nn / 2;
    for (int x = ln.col; x < g.pw; x += ln.lw) {
        const Footprint fx = footprint(x, g.num, g.den);
        const bool x_in = fx.last >= rp.x0 && fx.first < rp.x1;
        for (int y = ln.row; y < g.ph; y += ln.rstep) {
            const Footprint fy = footprint(y, g.num, g.den);
            const size_t di = ((size_t)y * g.pw + x) * (planar ? 1 : C);
            if (!(x_in && fy.last >= rp.y0 && fy.first < rp.y1)) {
#pragma unroll
                for (int c = 0; c < C; c++) dst[di + c * cstep] = (T)g.pad_bits;
                continue;
            }
            Acc sum[C];
#pragma unroll
            for (int c = 0; c < C; c++) sum[c] = 0;
            for (int l = fy.first; l <= fy.last; l++) {
                const uint32_t wy = l == fy.first ? (uint32_t)fy.w_first : l == fy.last ? (uint32_t)fy.w_last : (uint32_t)g.den;
                const mic_gp<const S> row = src + ((size_t)l * g.sw + fx.first) * C;
                uint32_t mid[C], ends[C];
#pragma unroll
                for (int c = 0; c < C; c++) { ends[c] = (uint32_t)fx.w_first * row[c]; mid[c] = 0; }
                const int nk = fx.last - fx.first;
                for (int k = 1; k < nk; k++) {
#pragma unroll
                    for (int c = 0; c < C; c++) mid[c] += row[k * C + c];
                }
                if (nk > 0) {
#pragma unroll
                    for (int c = 0; c < C; c++) ends[c] += (uint32_t)fx.w_last * row[nk * C + c];
                }
#pragma unroll
                for (int c = 0; c < C; c++) sum[c] += (Acc)wy * (Acc)(ends[c] + mid[c] * (uint32_t)g.den);
            }
#pragma unroll
            for (int c = 0; c < C; c++) {
                const uint32_t v = (uint32_t)((sum[c] + half) / nn);
                if (DT == MIC_HIP_OUT_NATIVE) dst[di + c * cstep] = (T)v;
                else dst[di + c * cstep] = (T)out_sample<DT>(v, ab[c], o);
            }
        }
    }
}

// n dwords of `bits` from d (4-byte aligned)
__global__ void __launch_bounds__(256) k_fill_dwords(uint32_t *d, size_t n, uint32_t bits) {
    const mic_gp<uint32_t> g = mic_g(d);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) g[i] = bits;
}

// the host's copy of out_bits, for pad: the same conversions (round to nearest even is the host's rounding mode too)
uint32_t host_bits(int dtype, float v) {
    uint32_t u; memcpy(&u, &v, 4);
    switch (dtype) {
    case MIC_HIP_OUT_F32: return u;
    case MIC_HIP_OUT_BF16: return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;                   // (v is finite)
    case MIC_HIP_OUT_F16: { const _Float16 h = (_Float16)v; uint16_t b; memcpy(&b, &h, 2); return b; }
    case MIC_HIP_OUT_U8: return (uint32_t)std::fmin(std::fmax(std::nearbyint(v), 0.f), 255.f);
    default: return (uint32_t)std::fmin(std::fmax(std::nearbyint(v), 0.f), 65535.f);
    }
}

}  // namespace

extern "C" int mic_hip_out_spec_check(const mic_hip_out_spec *spec, int channels, int bits_per_sample, int nsources, size_t *sample_bytes) {
    if (!spec || !sample_bytes || (channels != 1 && channels != 3) || (bits_per_sample != 8 && bits_per_sample != 16) || nsources < 1) return MIC_ERR_ARGS;
    if (spec->dtype < MIC_HIP_OUT_NATIVE || spec->dtype > MIC_HIP_OUT_F32) return MIC_ERR_ARGS;
    if (spec->flags & ~(MIC_HIP_OUT_CHANNELS_FIRST | MIC_HIP_OUT_CLAMP)) return MIC_ERR_ARGS;
    const int64_t na = spec->naffine;
    if (na != 0 && na != 1 && na != channels && na != (int64_t)nsources * channels) return MIC_ERR_ARGS;
    if (na > 0 && !spec->affine) return MIC_ERR_ARGS;
    for (int64_t i = 0; i < 2 * na; i++) if (!std::isfinite(spec->affine[i])) return MIC_ERR_ARGS;
    if (!std::isfinite(spec->clamp_lo) || !std::isfinite(spec->clamp_hi) || !std::isfinite(spec->pad)) return MIC_ERR_ARGS;
    if ((spec->flags & MIC_HIP_OUT_CLAMP) && !(spec->clamp_lo < spec->clamp_hi)) return MIC_ERR_ARGS;
    if (spec->dtype == MIC_HIP_OUT_NATIVE) {
        if (spec->flags || spec->affine || na || spec->clamp_lo != 0.f || spec->clamp_hi != 0.f || spec->pad != 0.f) return MIC_ERR_ARGS;
        *sample_bytes = bits_per_sample == 16 ? 2 : 1;
    } else
        *sample_bytes = spec->dtype == MIC_HIP_OUT_U8 ? 1 : spec->dtype == MIC_HIP_OUT_F32 ? 4 : 2;
    return MIC_OK;
}

namespace micapi {

int OutFormat::make(const mic_hip_out_spec *spec, int nch, int bits_per_sample, int nsources) {
    *this = OutFormat();
    channels = nch;
    sample = (size_t)nch * (bits_per_sample == 16 ? 2 : 1);                                 // (NATIVE: the pixel, as the native doors count it)
    if (!spec) return MIC_OK;
    size_t sb = 0;
    const int rc = mic_hip_out_spec_check(spec, nch, bits_per_sample, std::max(nsources, 1), &sb);
    if (rc || spec->dtype == MIC_HIP_OUT_NATIVE) return rc;
    dtype = spec->dtype; flags = spec->flags; sample = sb; lo = spec->clamp_lo; hi = spec->clamp_hi; pad = spec->pad;
    if (spec->naffine > 0) table.assign(spec->affine, spec->affine + 2 * (size_t)spec->naffine);
    if (spec->naffine > 1) { ch_step = nch > 1 ? 1 : 0; src_mul = spec->naffine == nch ? 0 : nch; }
    return MIC_OK;
}

uint32_t OutFormat::pad_bits() const {
    if (!typed()) return 0;
    const uint32_t b = host_bits(dtype, pad);
    return sample == 4 ? b : sample == 2 ? b * 0x10001u : b * 0x01010101u;
}

int fill_pad(hipStream_t stream, const OutFormat &o, void *d_out, size_t bytes) {
    const uint32_t bits = o.pad_bits();
    if (bits == 0 || bytes == 0) { HIP_TRY(hipMemsetAsync(d_out, 0, bytes, stream)); return MIC_OK; }
    // the tensor's base is aligned to its sample, so the dword pattern holds at any byte of it: bytes in front of the first whole
    // dword and behind the last one are set as bytes (the pattern of a 2-byte type has its two bytes wherever a dword starts)
    const size_t head = std::min(bytes, (size_t)(-(intptr_t)d_out & 3)), nd = (bytes - head) / 4, tail = bytes - head - nd * 4;
    const uint32_t rot = bits >> (8 * (unsigned)head) | (head ? bits << (32 - 8 * (unsigned)head) : 0);   // (little-endian; head 2: halves swap, equal anyway)
    for (size_t i = 0; i < head; i++) HIP_TRY(hipMemsetAsync((char *)d_out + i, (int)((bits >> (8 * i)) & 0xFF), 1, stream));
    if (nd) hipLaunchKernelGGL(k_fill_dwords, dim3((unsigned)std::min<size_t>((nd + 255) / 256, 4096)), dim3(256), 0, stream, (uint32_t *)((char *)d_out + head), nd, rot);
    for (size_t i = 0; i < tail; i++) HIP_TRY(hipMemsetAsync((char *)d_out + head + nd * 4 + i, (int)((rot >> (8 * i)) & 0xFF), 1, stream));
    return MIC_OK;
}

void launch_convert(hipStream_t stream, const OutFormat &o, const void *d_table, const uint16_t *stage, const ConvertRun *runs, size_t n,
                    int mw, int mh, int md, int cw, int ch, void *out) {
    constexpr size_t kMaxGridX = 0x7FFFFFFF;
    const unsigned gy = row_chunks(mw, mh);
    const OutParams op = o.params(d_table, 1);
    for (size_t q = 0; q < n; q += kMaxGridX) {
        const dim3 grid((unsigned)std::min(n - q, kMaxGridX), gy, (unsigned)std::min(std::max(md, 1), 64)), block(256);
        switch (o.dtype) {
        case MIC_HIP_OUT_U8: hipLaunchKernelGGL(k_convert_runs<MIC_HIP_OUT_U8>, grid, block, 0, stream, stage, runs + q, (uint8_t *)out, cw, ch, op); break;
        case MIC_HIP_OUT_U16: hipLaunchKernelGGL(k_convert_runs<MIC_HIP_OUT_U16>, grid, block, 0, stream, stage, runs + q, (uint16_t *)out, cw, ch, op); break;
        case MIC_HIP_OUT_F16: hipLaunchKernelGGL(k_convert_runs<MIC_HIP_OUT_F16>, grid, block, 0, stream, stage, runs + q, (uint16_t *)out, cw, ch, op); break;
        case MIC_HIP_OUT_BF16: hipLaunchKernelGGL(k_convert_runs<MIC_HIP_OUT_BF16>, grid, block, 0, stream, stage, runs + q, (uint16_t *)out, cw, ch, op); break;
        default: hipLaunchKernelGGL(k_convert_runs<MIC_HIP_OUT_F32>, grid, block, 0, stream, stage, runs + q, (uint32_t *)out, cw, ch, op); break;
        }
    }
}

namespace {
// the launches of one source format: S samples, C a pixel
template <typename S, int C>
void resample_as(hipStream_t stream, const dim3 &grid, int dtype, const OutParams &op, const void *stage, const ScaledPatch *recs, const ScaledGeom &g, void *out) {
    const dim3 block(256);
    const S *st = (const S *)stage;
    switch (dtype) {
    case MIC_HIP_OUT_NATIVE: hipLaunchKernelGGL((k_resample_patches<MIC_HIP_OUT_NATIVE, S, C>), grid, block, 0, stream, st, recs, (S *)out, g, op); break;
    case MIC_HIP_OUT_U8: hipLaunchKernelGGL((k_resample_patches<MIC_HIP_OUT_U8, S, C>), grid, block, 0, stream, st, recs, (uint8_t *)out, g, op); break;
    case MIC_HIP_OUT_U16: hipLaunchKernelGGL((k_resample_patches<MIC_HIP_OUT_U16, S, C>), grid, block, 0, stream, st, recs, (uint16_t *)out, g, op); break;
    case MIC_HIP_OUT_F16: hipLaunchKernelGGL((k_resample_patches<MIC_HIP_OUT_F16, S, C>), grid, block, 0, stream, st, recs, (uint16_t *)out, g, op); break;
    case MIC_HIP_OUT_BF16: hipLaunchKernelGGL((k_resample_patches<MIC_HIP_OUT_BF16, S, C>), grid, block, 0, stream, st, recs, (uint16_t *)out, g, op); break;
    default: hipLaunchKernelGGL((k_resample_patches<MIC_HIP_OUT_F32, S, C>), grid, block, 0, stream, st, recs, (uint32_t *)out, g, op); break;
    }
}
}  // namespace

void launch_resample(hipStream_t stream, int channels, int bits_per_sample, const OutFormat &o, const void *d_table, const void *stage,
                     const ScaledPatch *recs, size_t n, const ScaledGeom &g, void *out) {
    constexpr size_t kMaxGridX = 0x7FFFFFFF;
    const unsigned gy = row_chunks(g.pw, g.ph);
    const OutParams op = o.params(d_table, (size_t)g.ph * (size_t)g.pw);
    const size_t spx = (size_t)channels * (bits_per_sample == 16 ? 2 : 1);                 // bytes of a staged pixel
    for (size_t q = 0; q < n; q += kMaxGridX) {
        const dim3 grid((unsigned)std::min(n - q, kMaxGridX), gy);
        const void *st = (const char *)stage + q * (size_t)g.sh * (size_t)g.sw * spx;
        void *dq = (char *)out + q * (size_t)g.ph * (size_t)g.pw * o.pixel();
        if (channels == 3) resample_as<uint8_t, 3>(stream, grid, o.dtype, op, st, recs + q, g, dq);
        else if (bits_per_sample == 16) resample_as<uint16_t, 1>(stream, grid, o.dtype, op, st, recs + q, g, dq);
        else resample_as<uint8_t, 1>(stream, grid, o.dtype, op, st, recs + q, g, dq);
    }
}

void launch_gather(hipStream_t stream, GatherKind kind, const uint16_t *slab, const GatherPiece *pieces, size_t np, int mw, int mh, void *out,
                   int dtype, const OutParams &op, const RgbModeArgs &modes) {
    constexpr size_t kMaxGridX = 0x7FFFFFFF;
    const unsigned gy = row_chunks(mw, mh);
    for (size_t q = 0; q < np; q += kMaxGridX) {
        const dim3 grid((unsigned)std::min(np - q, kMaxGridX), gy), block(256);
        const GatherPiece *pq = pieces + q;
        const RgbPlaneSrc *sq = modes.srcs + q;
        const uint8_t *arena = (const uint8_t *)slab;
        if (kind == kGatherPxRGB) switch (dtype) {
            case MIC_HIP_OUT_NATIVE: hipLaunchKernelGGL(k_gather_px<3>, grid, block, 0, stream, arena, pq, (uint8_t *)out); break;
            case MIC_HIP_OUT_U8: hipLaunchKernelGGL(k_gather_px_typed_rgb<MIC_HIP_OUT_U8>, grid, block, 0, stream, arena, pq, (uint8_t *)out, op); break;
            case MIC_HIP_OUT_U16: hipLaunchKernelGGL(k_gather_px_typed_rgb<MIC_HIP_OUT_U16>, grid, block, 0, stream, arena, pq, (uint16_t *)out, op); break;
            case MIC_HIP_OUT_F16: hipLaunchKernelGGL(k_gather_px_typed_rgb<MIC_HIP_OUT_F16>, grid, block, 0, stream, arena, pq, (uint16_t *)out, op); break;
            case MIC_HIP_OUT_BF16: hipLaunchKernelGGL(k_gather_px_typed_rgb<MIC_HIP_OUT_BF16>, grid, block, 0, stream, arena, pq, (uint16_t *)out, op); break;
            default: hipLaunchKernelGGL(k_gather_px_typed_rgb<MIC_HIP_OUT_F32>, grid, block, 0, stream, arena, pq, (uint32_t *)out, op); break;
        } else if (kind == kGatherPxU16) switch (dtype) {
            case MIC_HIP_OUT_NATIVE: hipLaunchKernelGGL(k_gather_px<2>, grid, block, 0, stream, arena, pq, (uint8_t *)out); break;
            case MIC_HIP_OUT_U8: hipLaunchKernelGGL((k_gather_px_typed<MIC_HIP_OUT_U8, uint16_t>), grid, block, 0, stream, arena, pq, (uint8_t *)out, op); break;
            case MIC_HIP_OUT_U16: hipLaunchKernelGGL((k_gather_px_typed<MIC_HIP_OUT_U16, uint16_t>), grid, block, 0, stream, arena, pq, (uint16_t *)out, op); break;
            case MIC_HIP_OUT_F16: hipLaunchKernelGGL((k_gather_px_typed<MIC_HIP_OUT_F16, uint16_t>), grid, block, 0, stream, arena, pq, (uint16_t *)out, op); break;
            case MIC_HIP_OUT_BF16: hipLaunchKernelGGL((k_gather_px_typed<MIC_HIP_OUT_BF16, uint16_t>), grid, block, 0, stream, arena, pq, (uint16_t *)out, op); break;
            default: hipLaunchKernelGGL((k_gather_px_typed<MIC_HIP_OUT_F32, uint16_t>), grid, block, 0, stream, arena, pq, (uint32_t *)out, op); break;
        } else if (kind == kGatherPxU8) switch (dtype) {
            case MIC_HIP_OUT_NATIVE: hipLaunchKernelGGL(k_gather_px<1>, grid, block, 0, stream, arena, pq, (uint8_t *)out); break;
            case MIC_HIP_OUT_U8: hipLaunchKernelGGL((k_gather_px_typed<MIC_HIP_OUT_U8, uint8_t>), grid, block, 0, stream, arena, pq, (uint8_t *)out, op); break;
            case MIC_HIP_OUT_U16: hipLaunchKernelGGL((k_gather_px_typed<MIC_HIP_OUT_U16, uint8_t>), grid, block, 0, stream, arena, pq, (uint16_t *)out, op); break;
            case MIC_HIP_OUT_F16: hipLaunchKernelGGL((k_gather_px_typed<MIC_HIP_OUT_F16, uint8_t>), grid, block, 0, stream, arena, pq, (uint16_t *)out, op); break;
            case MIC_HIP_OUT_BF16: hipLaunchKernelGGL((k_gather_px_typed<MIC_HIP_OUT_BF16, uint8_t>), grid, block, 0, stream, arena, pq, (uint16_t *)out, op); break;
            default: hipLaunchKernelGGL((k_gather_px_typed<MIC_HIP_OUT_F32, uint8_t>), grid, block, 0, stream, arena, pq, (uint32_t *)out, op); break;
        } else if (kind == kGatherRGBModes) switch (dtype) {
            case MIC_HIP_OUT_NATIVE: hipLaunchKernelGGL(k_gather_modes_rgb, grid, block, 0, stream, slab, modes.raw, pq, sq, (uint8_t *)out); break;
            case MIC_HIP_OUT_U8: hipLaunchKernelGGL(k_gather_typed_modes_rgb<MIC_HIP_OUT_U8>, grid, block, 0, stream, slab, modes.raw, pq, sq, (uint8_t *)out, op); break;
            case MIC_HIP_OUT_U16: hipLaunchKernelGGL(k_gather_typed_modes_rgb<MIC_HIP_OUT_U16>, grid, block, 0, stream, slab, modes.raw, pq, sq, (uint16_t *)out, op); break;
            case MIC_HIP_OUT_F16: hipLaunchKernelGGL(k_gather_typed_modes_rgb<MIC_HIP_OUT_F16>, grid, block, 0, stream, slab, modes.raw, pq, sq, (uint16_t *)out, op); break;
            case MIC_HIP_OUT_BF16: hipLaunchKernelGGL(k_gather_typed_modes_rgb<MIC_HIP_OUT_BF16>, grid, block, 0, stream, slab, modes.raw, pq, sq, (uint16_t *)out, op); break;
            default: hipLaunchKernelGGL(k_gather_typed_modes_rgb<MIC_HIP_OUT_F32>, grid, block, 0, stream, slab, modes.raw, pq, sq, (uint32_t *)out, op); break;
        } else if (dtype == MIC_HIP_OUT_NATIVE) {
            if (kind == kGatherRGB) hipLaunchKernelGGL(k_gather_pieces_rgb, grid, block, 0, stream, slab, pq, (uint8_t *)out);
            else if (kind == kGatherU16) hipLaunchKernelGGL(k_gather_pieces<uint16_t>, grid, block, 0, stream, slab, pq, (uint16_t *)out);
            else hipLaunchKernelGGL(k_gather_pieces<uint8_t>, grid, block, 0, stream, slab, pq, (uint8_t *)out);
        } else if (kind == kGatherRGB) switch (dtype) {
            case MIC_HIP_OUT_U8: hipLaunchKernelGGL(k_gather_typed_rgb<MIC_HIP_OUT_U8>, grid, block, 0, stream, slab, pq, (uint8_t *)out, op); break;
            case MIC_HIP_OUT_U16: hipLaunchKernelGGL(k_gather_typed_rgb<MIC_HIP_OUT_U16>, grid, block, 0, stream, slab, pq, (uint16_t *)out, op); break;
            case MIC_HIP_OUT_F16: hipLaunchKernelGGL(k_gather_typed_rgb<MIC_HIP_OUT_F16>, grid, block, 0, stream, slab, pq, (uint16_t *)out, op); break;
            case MIC_HIP_OUT_BF16: hipLaunchKernelGGL(k_gather_typed_rgb<MIC_HIP_OUT_BF16>, grid, block, 0, stream, slab, pq, (uint16_t *)out, op); break;
            default: hipLaunchKernelGGL(k_gather_typed_rgb<MIC_HIP_OUT_F32>, grid, block, 0, stream, slab, pq, (uint32_t *)out, op); break;
        } else switch (dtype) {
            case MIC_HIP_OUT_U8: hipLaunchKernelGGL(k_gather_typed<MIC_HIP_OUT_U8>, grid, block, 0, stream, slab, pq, (uint8_t *)out, op); break;
            case MIC_HIP_OUT_U16: hipLaunchKernelGGL(k_gather_typed<MIC_HIP_OUT_U16>, grid, block, 0, stream, slab, pq, (uint16_t *)out, op); break;
            case MIC_HIP_OUT_F16: hipLaunchKernelGGL(k_gather_typed<MIC_HIP_OUT_F16>, grid, block, 0, stream, slab, pq, (uint16_t *)out, op); break;
            case MIC_HIP_OUT_BF16: hipLaunchKernelGGL(k_gather_typed<MIC_HIP_OUT_BF16>, grid, block, 0, stream, slab, pq, (uint16_t *)out, op); break;
            default: hipLaunchKernelGGL(k_gather_typed<MIC_HIP_OUT_F32>, grid, block, 0, stream, slab, pq, (uint32_t *)out, op); break;
        }
    }
}

void launch_cache_fill(hipStream_t stream, GatherKind kind, const uint16_t *slab, const CacheFill *fills, size_t n, size_t max_px) {
    constexpr size_t kMaxGridX = 0x7FFFFFFF;
    const unsigned gy = (unsigned)std::min<size_t>(32, std::max<size_t>(1, (max_px + 2047) / 2048));   // (eight pixels a lane at least)
    for (size_t q = 0; q < n; q += kMaxGridX) {
        const dim3 grid((unsigned)std::min(n - q, kMaxGridX), gy), block(256);
        if (kind == kGatherPxRGB) hipLaunchKernelGGL((k_cache_fill<uint8_t, true>), grid, block, 0, stream, slab, fills + q);
        else if (kind == kGatherPxU16) hipLaunchKernelGGL((k_cache_fill<uint16_t, false>), grid, block, 0, stream, slab, fills + q);
        else hipLaunchKernelGGL((k_cache_fill<uint8_t, false>), grid, block, 0, stream, slab, fills + q);
    }
}

int patch_pointer(const mic_hip_session *s, void **d_out, size_t need) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, *d_out) != hipSuccess) { (void)hipGetLastError(); return MIC_ERR_ARGS; }   // (unregistered memory)
    if (at.type == hipMemoryTypeDevice) {
        if (at.device != s->device) return MIC_ERR_ARGS;
        hipDeviceptr_t b = nullptr; size_t sz = 0;
        if (hipMemGetAddressRange(&b, &sz, (hipDeviceptr_t)*d_out) != hipSuccess) { (void)hipGetLastError(); return MIC_ERR_ARGS; }
        if ((size_t)((char *)*d_out - (char *)b) + need > sz) return MIC_ERR_CAPACITY;     // (the allocation ends before out_cap does)
    } else if (at.type == hipMemoryTypeHost || at.type == hipMemoryTypeManaged) {
        if (at.devicePointer) *d_out = at.devicePointer;
    } else return MIC_ERR_ARGS;
    return MIC_OK;
}

int crop_door(mic_hip_session **s, DefaultLease &lease, void **d_out, size_t need, const OutFormat &o) {
    int rc;
    if (!*s) { if ((rc = lease.acquire())) return rc; *s = cur_default(); }
    else if ((rc = (*s)->activate())) return rc;
    rc = patch_pointer(*s, d_out, need);                                                    // judged before anything is launched
    if (rc == MIC_ERR_CAPACITY || (o.typed() ? !out_aligned(o, *d_out) : ((o.sample & 1) == 0 && ((size_t)*d_out & 1) != 0))) rc = MIC_ERR_ARGS;   // (u8 RGB: any address)
    return rc;
}

int pack_streams(mic_hip_session *s, int nb, const std::function<uint64_t(int)> &len, const std::function<const uint8_t *(int)> &src, bool device,
                 std::vector<uint64_t> &begins, std::vector<uint64_t> &ends) {
    begins.assign((size_t)nb, 0); ends.assign((size_t)nb, 0);
    uint64_t total = 0;
    for (int i = 0; i < nb; i++) { begins[(size_t)i] = total; total += len(i); ends[(size_t)i] = total; }
    const int rc = s->io_comp.reserve((size_t)total + 64);
    if (rc) return rc;
    for (int i = 0; i < nb;) {
        const uint8_t *p = src(i);
        int j = i + 1;
        while (j < nb && src(j) == p + (ends[(size_t)j - 1] - begins[(size_t)i])) j++;
        HIP_TRY(hipMemcpyAsync((uint8_t *)s->io_comp.p + begins[(size_t)i], p, (size_t)(ends[(size_t)j - 1] - begins[(size_t)i]),
                               device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream));
        i = j;
    }
    return MIC_OK;
}

}  // namespace micapi
