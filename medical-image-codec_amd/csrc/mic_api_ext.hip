// mic_api_ext.hip -- MIC3 / WSI on the GPU (wsicompress.go, wsiformat.go, wsipyramid.go, ycocgr.go).
// 8-bit RGB slides (three YCoCg-R planes per tile) and 8/16-bit greyscale slides (one plane per tile).
//
// CompressWSI = pyramid (2x2 box) -> zero-padded tiles -> YCoCg-R -> three planes per tile ->
// per plane: constant-zero / constant / CompressSingleFrame / raw fallback -> tile blobs -> MIC3.
// On the device: the pyramid, the tile extraction fused with the colour transform and the
// per-plane min/max (which decides the plane mode and the maxValue handed to the unit codec),
// and the unit codec itself over every non-constant plane of the slide in one batch.  The host
// writes the container around the plane blobs.  Decode mirrors it: one batch over the planes of
// the requested tiles, then inverse transform + crop on the device.
#include "mic_session.h"
#include "mic_wave.h"
#include "mic_rects.h"
#include "mic_tile_cache.h"

#include <memory>

static constexpr size_t kMaxGridX = 0x7FFFFFFF;
static constexpr size_t kMaxGridY = 65535;   // HIP grid limit in y and z: launches that put tiles there take at most this many per sub-batch

// One coded plane of a tile (compressWSIPlane, wsicompress.go:373-421): mode 0 constant zero, 1 constant `value`, 2 a unit-codec
// stream, 3 raw pixels; the bytes of modes 2 / 3 are `len` bytes at base + off on the device, the base being whatever buffer the
// records describe (the session's store, a slab of uploaded blobs; 0 -- absolute addresses -- for a slab just encoded).
struct WsiPlane { uint8_t mode; uint16_t value; uint64_t off, len; };

namespace {

// Downsample2xRGB (wsipyramid.go:10-32): (v00+v10+v01+v11+2)/4 per channel, odd edge dropped.
__global__ void __launch_bounds__(256) k_wsi_downsample(const uint8_t *src, int sw, uint8_t *dst, int dw, int dh) {
    const size_t n = (size_t)dw * dh * 3;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % 3); const size_t px = i / 3;
        const int x = (int)(px % dw), y = (int)(px / dw);
        const size_t a = ((size_t)(2 * y) * sw + 2 * x) * 3 + c, b = a + 3, d = a + (size_t)sw * 3, e = d + 3;
        dst[i] = (uint8_t)(((int)src[a] + src[b] + src[d] + src[e] + 2) / 4);
    }
}

// extractTileRGB (wsicompress.go:529-555) fused with YCoCgRForward (asm_amd64.go:88-104) and the
// constant / max scan of compressWSIPlane (wsicompress.go:375-385).  grid = (chunks, tiles).
// planes: [tile][3][tw*th] u16 ; stats: [tile][3] {min, max} as u32 pairs (pre-set to 0xFFFFFFFF / 0).
__global__ void __launch_bounds__(256) k_wsi_tile_planes(const uint8_t *img, int iw, int ih, int tw, int th, int tiles_x,
                                                       int tile_base, uint16_t *planes, uint32_t *stats) {
    const int tile = blockIdx.y;                                  // slab-local index into planes / stats
    const int tx = (tile + tile_base) % tiles_x, ty = (tile + tile_base) / tiles_x;
    const size_t npx = (size_t)tw * th;
    uint16_t *py = planes + (size_t)tile * 3 * npx, *pco = py + npx, *pcg = pco + npx;
    uint32_t mn[3] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu }, mx[3] = { 0, 0, 0 };
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % tw), y = (int)(i / tw);
        const int sx = tx * tw + x, sy = ty * th + y;
        int r = 0, g = 0, b = 0;
        if (sx < iw && sy < ih) { const uint8_t *p = img + ((size_t)sy * iw + sx) * 3; r = p[0]; g = p[1]; b = p[2]; }
        const int co = r - b;
        const int t = b + (co >> 1);
        const int cg = g - t;
        const int yv = t + (cg >> 1);
        const uint32_t v0 = (uint16_t)yv;
        const uint32_t v1 = (uint16_t)(((int16_t)co << 1) ^ ((int16_t)co >> 15));     // ZigZag, deltazigzagcompressu16.go:108-111
        const uint32_t v2 = (uint16_t)(((int16_t)cg << 1) ^ ((int16_t)cg >> 15));
        py[i] = (uint16_t)v0; pco[i] = (uint16_t)v1; pcg[i] = (uint16_t)v2;
        mn[0] = min(mn[0], v0); mx[0] = max(mx[0], v0);
        mn[1] = min(mn[1], v1); mx[1] = max(mx[1], v1);
        mn[2] = min(mn[2], v2); mx[2] = max(mx[2], v2);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        mn[k] = mic_wave_reduce_min(mn[k]); mx[k] = mic_wave_reduce_max(mx[k]);
        if ((threadIdx.x & 63) == 0) { atomicMin(&stats[((size_t)tile * 3 + k) * 2], mn[k]); atomicMax(&stats[((size_t)tile * 3 + k) * 2 + 1], mx[k]); }
    }
}

// YCoCgRInverse (asm_amd64.go:106-121) + cropTile (wsicompress.go:557-570): planes of tile `t` -> dst
// image region.  grid = (chunks, tiles).  place[t] = {dst x0, dst y0, crop w, crop h}.
__global__ void __launch_bounds__(256) k_wsi_planes_to_rgb(const uint16_t *planes, int tw, int th, const int4 *place,
                                                         uint8_t *dst, int dst_w) {
    const int tile = blockIdx.y;
    const int4 pl = place[tile];
    const size_t npx = (size_t)tw * th;
    const uint16_t *py = planes + (size_t)tile * 3 * npx, *pco = py + npx, *pcg = pco + npx;
    const size_t n = (size_t)pl.z * pl.w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % pl.z), y = (int)(i / pl.z);
        const size_t si = (size_t)y * tw + x;
        const int yv = py[si];
        const uint32_t uco = pco[si], ucg = pcg[si];
        const int co = (int)(int16_t)((uco >> 1) ^ (uint16_t)(-(int)(uco & 1)));       // UnZigZag, :113-116
        const int cg = (int)(int16_t)((ucg >> 1) ^ (uint16_t)(-(int)(ucg & 1)));
        const int t = yv - (cg >> 1);
        const int g = cg + t;
        const int b = t - (co >> 1);
        const int r = co + b;
        uint8_t *o = dst + ((size_t)(pl.y + y) * dst_w + (pl.x + x)) * 3;
        o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)b;
    }
}

// Greyscale slides (channels = 1, 8 or 16 bits per sample; T = the sample type, little-endian like bytesToUint16Slice,
// wsicompress.go:573-603).  Downsample2xGrey (wsipyramid.go:34-55) works on the samples widened to u16.
template <typename T>
__global__ void __launch_bounds__(256) k_wsi_downsample_grey(const T *src, int sw, T *dst, int dw, int dh) {
    const size_t n = (size_t)dw * dh;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % dw), y = (int)(i / dw);
        const size_t a = (size_t)(2 * y) * sw + 2 * x, d = a + (size_t)sw;
        dst[i] = (T)(((uint32_t)src[a] + src[a + 1] + src[d] + src[d + 1] + 2) / 4);
    }
}

// extractTileRGB for one channel + bytesToUint16Slice + the constant / max scan.  planes: [tile][tw*th] u16 ; stats: [tile] {min, max}
template <typename T>
__global__ void __launch_bounds__(256) k_wsi_tile_plane_grey(const T *img, int iw, int ih, int tw, int th, int tiles_x,
                                                           int tile_base, uint16_t *planes, uint32_t *stats) {
    const int tile = blockIdx.y;
    const int tx = (tile + tile_base) % tiles_x, ty = (tile + tile_base) / tiles_x;
    const size_t npx = (size_t)tw * th;
    uint16_t *pl = planes + (size_t)tile * npx;
    uint32_t mn = 0xFFFFFFFFu, mx = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % tw), y = (int)(i / tw);
        const int sx = tx * tw + x, sy = ty * th + y;
        const uint32_t v = (sx < iw && sy < ih) ? (uint32_t)img[(size_t)sy * iw + sx] : 0u;
        pl[i] = (uint16_t)v;
        mn = min(mn, v); mx = max(mx, v);
    }
    mn = mic_wave_reduce_min(mn); mx = mic_wave_reduce_max(mx);
    if ((threadIdx.x & 63) == 0) { atomicMin(&stats[(size_t)tile * 2], mn); atomicMax(&stats[(size_t)tile * 2 + 1], mx); }
}

// uint16ToBytes (wsicompress.go:589-603) + cropTile: the plane of tile `t` -> dst image region
template <typename T>
__global__ void __launch_bounds__(256) k_wsi_plane_to_grey(const uint16_t *planes, int tw, int th, const int4 *place, T *dst, int dst_w) {
    const int tile = blockIdx.y;
    const int4 pl = place[tile];
    const uint16_t *src = planes + (size_t)tile * tw * th;
    const size_t n = (size_t)pl.z * pl.w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % pl.z), y = (int)(i / pl.z);
        dst[(size_t)(pl.y + y) * dst_w + (pl.x + x)] = (T)src[(size_t)y * tw + x];
    }
}

// ---- patches: many rectangles of many tiles, gathered from the decoded planes into an n x ph x pw x C tensor -----------------------
// Tile u of a sub-batch has its P planes at a sample offset of its own in the slab (the prefix sum of P * tw * th over the
// sub-batch: tiles of different sizes share a slab), so a constant plane is a span of the slab ...
struct FillSpan { uint64_t off; uint32_t npx, value; };
// constant planes of a slab in one launch: grid = (chunks, spans)
__global__ void __launch_bounds__(256) k_fill_spans(uint16_t *slab, const FillSpan *fill) {
    const FillSpan f = fill[blockIdx.y];
    uint16_t *p = slab + f.off;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < f.npx; i += (size_t)gridDim.x * blockDim.x) p[i] = (uint16_t)f.value;
}
// ... and a piece, one patch-tile overlap, is a GatherPiece (mic_pieces.h): plane 0's first sample of the overlap in the slab, the
// tile's rows tw apart and its planes tw * th, to its place in the patch tensor.  The host plans them (plan_clip).

struct Level { int w, h, tx, ty, first; };

// autoLevelCount + computeLevels (wsiformat.go:244-285) with the truncation of wsicompress.go:47-77
std::vector<Level> plan_levels(int w, int h, int tw, int th, int req) {
    int n = req;
    if (n <= 0) { n = 1; int ww = w, hh = h; while (ww > tw || hh > th) { ww /= 2; hh /= 2; n++; if (ww <= 1 && hh <= 1) break; } }
    std::vector<Level> lv;
    int ww = w, hh = h;
    for (int i = 0; i < n; i++) {
        if (i > 0) { const int nw = lv[i - 1].w / 2, nh = lv[i - 1].h / 2; if (nw == 0 || nh == 0) break; ww = nw; hh = nh; }
        lv.push_back(Level{ ww, hh, (ww + tw - 1) / tw, (hh + th - 1) / th, 0 });
    }
    int idx = 0;
    for (auto &l : lv) { l.first = idx; idx += l.tx * l.ty; }
    return lv;
}

struct Mic3 {
    int w, h, tw, th, channels, bps, flags, nlev; uint64_t total; size_t data_off;
    std::vector<Level> lv;
    bool rgb() const { return channels == 3 && bps == 8; }                    // compressTileBlob / decompressTileBlob, wsicompress.go:312-317, :424-429
    bool grey() const { return channels == 1 && (bps == 8 || bps == 16); }
    bool supported() const { return (rgb() && (flags & 0x02)) || grey(); }
    int planes() const { return rgb() ? 3 : 1; }
    size_t bpp() const { return (size_t)channels * (bps == 16 ? 2 : 1); }  // bytesPerPixel, wsicompress.go:530-533
};
// ReadMIC3Header (wsiformat.go:169-227) in two steps, so that a reader that pulls the file through a callback can check the fixed
// 48 bytes against the file's length before it reads the level table and tile index: parse_mic3_fixed sees c[0 .. 48) only,
// parse_mic3_levels c[48 .. 48 + 20 * nlev).  len is the whole file's length either way.
int parse_mic3_fixed(const uint8_t *c, size_t len, Mic3 &m) {
    if (len < 48 || memcmp(c, "MIC3", 4) != 0) return MIC_ERR_CORRUPT;
    if (get_u32(c + 4) != 1) return MIC_ERR_CORRUPT;
    m.w = (int)get_u32(c + 8); m.h = (int)get_u32(c + 12); m.tw = (int)get_u32(c + 16); m.th = (int)get_u32(c + 20);
    m.channels = c[24] | (c[25] << 8); m.bps = c[26]; m.flags = c[27]; m.nlev = c[28] | (c[29] << 8); m.total = get_u64(c + 32);
    if (len < 48 + 20 * (size_t)m.nlev) return MIC_ERR_CORRUPT;
    if (m.total > (len - 48 - 20 * (size_t)m.nlev) / 16) return MIC_ERR_CORRUPT;
    m.data_off = 48 + 20 * (size_t)m.nlev + 16 * (size_t)m.total;
    return MIC_OK;
}
int parse_mic3_levels(const uint8_t *c, Mic3 &m) {
    m.lv.clear();
    for (int i = 0; i < m.nlev; i++) {
        const uint8_t *p = c + 48 + 20 * (size_t)i;
        m.lv.push_back(Level{ (int)get_u32(p), (int)get_u32(p + 4), (int)get_u32(p + 8), (int)get_u32(p + 12), (int)get_u32(p + 16) });
    }
    if (m.tw <= 0 || m.th <= 0 || (size_t)m.tw * m.th > ((size_t)1 << 26)) return MIC_ERR_CORRUPT;
    // the level table must be what computeLevels writes (wsiformat.go:244-271): positive dimensions, tile counts that are the
    // ceilings of dimension / tile size, tile ranges inside the tile table.  The decoders walk tx * ty tiles of a level, so a
    // descriptor that lies about them would drive the host loops (and int arithmetic) wherever the file says.
    for (const Level &l : m.lv) {
        if (l.w <= 0 || l.h <= 0 || l.first < 0) return MIC_ERR_CORRUPT;
        if ((int64_t)l.tx != ((int64_t)l.w + m.tw - 1) / m.tw || (int64_t)l.ty != ((int64_t)l.h + m.th - 1) / m.th) return MIC_ERR_CORRUPT;
        if ((uint64_t)l.first + (uint64_t)l.tx * (uint64_t)l.ty > m.total) return MIC_ERR_CORRUPT;
    }
    return MIC_OK;
}
int parse_mic3(const uint8_t *c, size_t len, Mic3 &m) {
    const int rc = parse_mic3_fixed(c, len, m);
    return rc ? rc : parse_mic3_levels(c, m);
}

// The slide formats compressTileBlob codes (wsicompress.go:312-317) with WSIOptions.defaults (wsiformat.go:86-96): fmt of a
// width x height slide, tile_w / tile_h 0 = 256.  What every MIC3 encode entry point checks first.
int wsi_options(int width, int height, int channels, int bits_per_sample, int tile_w, int tile_h, int levels, Mic3 &fmt) {
    fmt = Mic3();
    fmt.channels = channels; fmt.bps = bits_per_sample; fmt.flags = 0x01 | (channels == 3 ? 0x02 : 0);
    if (!fmt.supported()) return MIC_ERR_UNSUPPORTED;
    fmt.w = width; fmt.h = height; fmt.tw = tile_w ? tile_w : 256; fmt.th = tile_h ? tile_h : 256;
    if ((size_t)fmt.tw * fmt.th > ((size_t)1 << 26) || levels > 32) return MIC_ERR_UNSUPPORTED;
    return MIC_OK;
}

// ---- the kernels by slide format: each helper is the one place that picks the instantiation ------------------------------------
// tiles t0 .. t0 + nt - 1 of level L (image img) -> planes [nt][P][tw * th] and their {min, max} stats
void launch_tile_planes(hipStream_t st, const Mic3 &fmt, const void *img, const Level &L, size_t t0, size_t nt, uint16_t *planes, uint32_t *stats) {
    const dim3 grid(8, (unsigned)nt), block(256);
    if (fmt.planes() == 3)
        hipLaunchKernelGGL(k_wsi_tile_planes, grid, block, 0, st, (const uint8_t *)img, L.w, L.h, fmt.tw, fmt.th, L.tx, (int)t0, planes, stats);
    else if (fmt.bps == 16)
        hipLaunchKernelGGL(k_wsi_tile_plane_grey<uint16_t>, grid, block, 0, st, (const uint16_t *)img, L.w, L.h, fmt.tw, fmt.th, L.tx, (int)t0, planes, stats);
    else
        hipLaunchKernelGGL(k_wsi_tile_plane_grey<uint8_t>, grid, block, 0, st, (const uint8_t *)img, L.w, L.h, fmt.tw, fmt.th, L.tx, (int)t0, planes, stats);
}
// planes of nt tiles -> dst (dst_w pixels across) at place[k] (device)
void launch_planes_to_pixels(hipStream_t st, const Mic3 &m, const uint16_t *planes, const int4 *place, size_t nt, void *dst, int dst_w) {
    const dim3 grid(16, (unsigned)nt), block(256);
    if (m.planes() == 3)
        hipLaunchKernelGGL(k_wsi_planes_to_rgb, grid, block, 0, st, planes, m.tw, m.th, place, (uint8_t *)dst, dst_w);
    else if (m.bps == 16)
        hipLaunchKernelGGL(k_wsi_plane_to_grey<uint16_t>, grid, block, 0, st, planes, m.tw, m.th, place, (uint16_t *)dst, dst_w);
    else
        hipLaunchKernelGGL(k_wsi_plane_to_grey<uint8_t>, grid, block, 0, st, planes, m.tw, m.th, place, (uint8_t *)dst, dst_w);
}
// one level of the pyramid: Downsample2xRGB / Downsample2xGrey of src (sw samples across) into dst (dw x dh)
void launch_downsample(hipStream_t st, const Mic3 &fmt, const void *src, int sw, void *dst, int dw, int dh) {
    if (fmt.planes() == 3)
        hipLaunchKernelGGL(k_wsi_downsample, dim3(1024), dim3(256), 0, st, (const uint8_t *)src, sw, (uint8_t *)dst, dw, dh);
    else if (fmt.bps == 16)
        hipLaunchKernelGGL(k_wsi_downsample_grey<uint16_t>, dim3(1024), dim3(256), 0, st, (const uint16_t *)src, sw, (uint16_t *)dst, dw, dh);
    else
        hipLaunchKernelGGL(k_wsi_downsample_grey<uint8_t>, dim3(1024), dim3(256), 0, st, (const uint8_t *)src, sw, (uint8_t *)dst, dw, dh);
}

// ---- tile blobs ------------------------------------------------------------------------------------------------------------------
// Bytes of one plane in a tile blob: the mode byte, then the constant (mode 1) or the stream / raw pixels (modes 2, 3)
uint64_t plane_bytes(const WsiPlane &p) { return p.mode == 0 ? 1 : p.mode == 1 ? 3 : 1 + p.len; }

// compressTileBlob (wsicompress.go:334-364) on the device: tile blockIdx.x's planes, each with its mode byte in front (and its
// constant), to their places in the payload; for RGB the tile's three plane lengths in front of them.  src is a device address.
struct WsiRec { uint64_t src, dst; uint32_t len; uint32_t mode_value; };          // mode_value = mode | value << 8
__global__ void __launch_bounds__(256) k_wsi_assemble(const WsiRec *recs, int P, uint8_t *payload) {
    const size_t t = blockIdx.x;
    typedef uint32_t wv4 __attribute__((ext_vector_type(4)));
    typedef wv4 WQ __attribute__((aligned(1)));
    for (int p = 0; p < P; p++) {
        const WsiRec r = recs[t * (size_t)P + (size_t)p];
        const uint32_t mode = r.mode_value & 0xFFu, value = r.mode_value >> 8;
        uint8_t *d = payload + r.dst;
        const uint32_t plen = mode == 0 ? 1u : mode == 1 ? 3u : 1u + r.len;
        if (threadIdx.x == 0) {
            d[0] = (uint8_t)mode;
            if (mode == 1) { d[1] = (uint8_t)value; d[2] = (uint8_t)(value >> 8); }
            if (P == 3) {                                                               // [Y_len][Co_len][Cg_len], u32 LE, in front of the tile's planes
                uint8_t *h = payload + recs[t * 3].dst - 12 + 4 * p;
                h[0] = (uint8_t)plen; h[1] = (uint8_t)(plen >> 8); h[2] = (uint8_t)(plen >> 16); h[3] = (uint8_t)(plen >> 24);
            }
        }
        if (mode >= 2) {
            const uint8_t *sp = (const uint8_t *)(uintptr_t)r.src; uint8_t *dp = d + 1;
            const uint32_t nv = r.len / 16;
            for (uint32_t i = threadIdx.x; i < nv; i += 256) *(WQ *)(dp + (size_t)i * 16) = *(const WQ *)(sp + (size_t)i * 16);
            if (threadIdx.x < (r.len & 15u)) dp[(size_t)nv * 16 + threadIdx.x] = sp[(size_t)nv * 16 + threadIdx.x];
        }
    }
}

// The blobs of n tiles (P plane records each, bytes at base + off) back to back in `payload` on the device: the host lays them
// out from the records, one k_wsi_assemble launch writes them.  tlen[t] = bytes of tile t, *total = their sum.
int assemble_tiles(mic_hip_session *s, const WsiPlane *pl, size_t n, size_t P, uint64_t base, DevBuf &payload, DevBuf &d_recs,
                   uint64_t *tlen, uint64_t *total) {
    std::vector<WsiRec> recs(n * P);
    uint64_t off = 0;
    for (size_t t = 0; t < n; t++) {
        const uint64_t t0 = off;
        if (P == 3) off += 12;
        for (size_t p = 0; p < P; p++) {
            const WsiPlane &wp = pl[t * P + p];
            recs[t * P + p] = WsiRec{ base + wp.off, off, wp.mode >= 2 ? (uint32_t)wp.len : 0u, (uint32_t)wp.mode | ((uint32_t)wp.value << 8) };
            off += plane_bytes(wp);
        }
        tlen[t] = off - t0;
    }
    *total = off;
    int rc;
    if ((rc = payload.reserve((size_t)off + 64)) || (rc = d_recs.reserve(recs.size() * sizeof(WsiRec) + 64))) return rc;
    if (n) {
        HIP_TRY(hipMemcpyAsync(d_recs.p, recs.data(), recs.size() * sizeof(WsiRec), hipMemcpyHostToDevice, s->stream));
        hipLaunchKernelGGL(k_wsi_assemble, dim3((unsigned)n), dim3(256), 0, s->stream, (const WsiRec *)d_recs.p, (int)P, (uint8_t *)payload.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s->stream));                                       // (recs is a stack-scope vector)
    }
    return MIC_OK;
}

// WriteMIC3 (wsiformat.go:99-165) without the blobs: header, level table, tile index for blobs of the given lengths back to back
void put_mic3_index(uint8_t *out, const Mic3 &fmt, const std::vector<Level> &lv, const std::vector<uint64_t> &lens) {
    const int nlev = (int)lv.size();
    memset(out, 0, 48 + 20 * (size_t)nlev);
    memcpy(out, "MIC3", 4); put_u32(out + 4, 1); put_u32(out + 8, (uint32_t)fmt.w); put_u32(out + 12, (uint32_t)fmt.h);
    put_u32(out + 16, (uint32_t)fmt.tw); put_u32(out + 20, (uint32_t)fmt.th);
    out[24] = (uint8_t)fmt.channels; out[25] = 0; out[26] = (uint8_t)fmt.bps; out[27] = (uint8_t)fmt.flags;
    out[28] = (uint8_t)nlev; out[29] = (uint8_t)(nlev >> 8);
    put_u64(out + 32, (uint64_t)lens.size());
    for (int i = 0; i < nlev; i++) {
        uint8_t *ld = out + 48 + 20 * (size_t)i;
        put_u32(ld, (uint32_t)lv[(size_t)i].w); put_u32(ld + 4, (uint32_t)lv[(size_t)i].h); put_u32(ld + 8, (uint32_t)lv[(size_t)i].tx);
        put_u32(ld + 12, (uint32_t)lv[(size_t)i].ty); put_u32(ld + 16, (uint32_t)lv[(size_t)i].first);
    }
    uint64_t off = 0;
    for (size_t t = 0; t < lens.size(); t++) {
        uint8_t *e = out + 48 + 20 * (size_t)nlev + 16 * t;
        put_u64(e, off); put_u64(e + 8, lens[t]);
        off += lens[t];
    }
}

// ---- decode ----------------------------------------------------------------------------------------------------------------------
// decompressTileBlob (wsicompress.go:424-527) for the nq planes of a slab of tiles, from their records (bytes at base + off on the
// device) up to the planes: at(q) says where plane q lies in `slab` (samples) and how large its tile is.  Constant planes are spans
// filled by one launch (the list: s->wsi_fills), raw planes are copied, streams go through the unit codec in one chain.
// plane_status = NULL: the first unit that fails ends the call with its status; else plane_status[q] receives every plane's status
// and the call goes on.  The planes are complete on the session's stream on return, and the host has waited for the stream: the
// caller may reuse the bytes behind `base`, the next call the fill list.  (It waits even for a slab of raw planes only, where
// nothing of the host's is in flight: one rule, at the price of one wait the tile, region and level decoders did not have there.)
struct PlaneAt { uint64_t at; int32_t tw, th; };
template <class At>
int decode_plane_slab(mic_hip_session *s, const uint8_t *base, const WsiPlane *pl, size_t nq, At at, DevBuf &slab, size_t samples,
                      int32_t *plane_status) {
    int rc;
    if ((rc = slab.reserve(samples * 2 + 64))) return rc;
    uint16_t *dp = (uint16_t *)slab.p;
    std::vector<mic_hip_unit> units; std::vector<uint64_t> begins, ends; std::vector<FillSpan> fills; std::vector<size_t> unit_plane;
    for (size_t q = 0; q < nq; q++) {
        const WsiPlane &wp = pl[q];
        const PlaneAt a = at(q);
        const size_t npx = (size_t)a.tw * a.th;
        if (plane_status) plane_status[q] = MIC_OK;
        if (wp.mode <= 1) fills.push_back(FillSpan{ a.at, (uint32_t)npx, wp.mode ? wp.value : 0u });
        else if (wp.mode == 2) { units.push_back(mic_hip_unit{ a.at, a.tw, a.th, 0, 0 }); begins.push_back(wp.off); ends.push_back(wp.off + wp.len); unit_plane.push_back(q); }
        else HIP_TRY(hipMemcpyAsync(dp + a.at, base + wp.off, npx * 2, hipMemcpyDeviceToDevice, s->stream));
    }
    if (!fills.empty()) {
        if ((rc = s->wsi_fills.reserve(fills.size() * sizeof(FillSpan) + 64))) return rc;
        HIP_TRY(hipMemcpyAsync(s->wsi_fills.p, fills.data(), fills.size() * sizeof(FillSpan), hipMemcpyHostToDevice, s->stream));
        s->timer.reset(s->stream); s->timer.mark("k_fill_spans");
        for (size_t f0 = 0; f0 < fills.size(); f0 += kMaxGridY)
            hipLaunchKernelGGL(k_fill_spans, dim3(4, (unsigned)std::min<size_t>(kMaxGridY, fills.size() - f0)), dim3(256), 0, s->stream, dp, (const FillSpan *)s->wsi_fills.p + f0);
        HIP_TRY(hipGetLastError());
    }
    if (!units.empty()) {
        if ((rc = session_decode_enqueue_spans(s, base, begins.data(), ends.data(), units.data(), (int)units.size(), dp))) return rc;
        std::vector<int32_t> st(units.size());
        if ((rc = session_decode_finish(s, st.data()))) return rc;
        if (plane_status) for (size_t u = 0; u < st.size(); u++) plane_status[unit_plane[u]] = st[u];
        else for (int32_t v : st) if (v != MIC_OK) return v;
    } else HIP_TRY(hipStreamSynchronize(s->stream));                                        // (session_decode_finish waits otherwise)
    return MIC_OK;
}

// ... for nt tiles of one size, plane q at q * tw * th of `planes`, then YCoCg-R inverse / uint16ToBytes + crop into dst (dst_w
// pixels across), tile k at place[k] (host).  aux holds the place rectangles.
int decode_planes(mic_hip_session *s, const Mic3 &m, const uint8_t *base, const WsiPlane *pl, size_t nt, const int4 *place,
                  DevBuf &planes, DevBuf &aux, void *dst, int dst_w) {
    const size_t nq = nt * (size_t)m.planes(), npx = (size_t)m.tw * m.th;
    int rc;
    if ((rc = decode_plane_slab(s, base, pl, nq, [&](size_t q) { return PlaneAt{ q * npx, m.tw, m.th }; }, planes, nq * npx, nullptr))) return rc;
    if ((rc = aux.reserve(nt * sizeof(int4) + 64))) return rc;
    int4 *d_place = (int4 *)aux.p;
    HIP_TRY(hipMemcpyAsync(d_place, place, nt * sizeof(int4), hipMemcpyHostToDevice, s->stream));
    s->timer.reset(s->stream); s->timer.mark("k_wsi_planes_to_pixels");
    launch_planes_to_pixels(s->stream, m, (const uint16_t *)planes.p, d_place, nt, dst, dst_w);
    s->timer.mark("end");
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MIC_OK;
}

struct TileBlob { const uint8_t *p; size_t len; };
// one tile blob checked on the host (decompressTileBlob, wsicompress.go:424-527): its P plane records are appended to pl, the bytes
// of its streams and raw planes to `bytes` (the records' off: into it).  A blob that fails leaves fewer than P records behind.
int parse_tile_blob(const Mic3 &m, const uint8_t *blob, size_t bl, std::vector<WsiPlane> &pl, std::vector<uint8_t> &bytes) {
    const size_t P = (size_t)m.planes(), npx = (size_t)m.tw * m.th;
    size_t pl_off[3] = { 0, 0, 0 }, pl_len[3] = { (size_t)bl, 0, 0 };                      // greyscale: the blob is the plane, :477-484
    if (P == 3) {
        if (bl < 12) return MIC_ERR_CORRUPT;
        const size_t l0 = get_u32(blob), l1 = get_u32(blob + 4), l2 = get_u32(blob + 8);
        if (12 + l0 + l1 + l2 > bl) return MIC_ERR_CORRUPT;                                // wsicompress.go:440-442
        pl_off[0] = 12; pl_off[1] = 12 + l0; pl_off[2] = 12 + l0 + l1; pl_len[0] = l0; pl_len[1] = l1; pl_len[2] = l2;
    }
    for (size_t p = 0; p < P; p++) {                                                       // decompressWSIPlane, :487-527
        const uint8_t *d = blob + pl_off[p]; const size_t dl = pl_len[p];
        if (dl == 0) return MIC_ERR_CORRUPT;
        WsiPlane wp{ d[0], 0, bytes.size(), 0 };
        if (d[0] == 0) { }
        else if (d[0] == 1) { if (dl < 3) return MIC_ERR_CORRUPT; wp.value = (uint16_t)(d[1] | (d[2] << 8)); }
        else if (d[0] == 2) wp.len = dl - 1;
        else if (d[0] == 3) { if (dl < 1 + 2 * npx) return MIC_ERR_CORRUPT; wp.len = 2 * npx; }
        else return MIC_ERR_CORRUPT;
        if (wp.mode >= 2) bytes.insert(bytes.end(), d + 1, d + 1 + wp.len);
        pl.push_back(wp);
    }
    return MIC_OK;
}
// decode the given tiles (global indices) of one level into dst (an image of dst_w x dst_h pixels of the slide's format);
// place[k] = where tile k goes and how much of it is kept.  Slab by slab: the blobs are checked on the host, their planes' bytes
// go up in one copy, decode_planes does the rest.
int decode_blobs(const Mic3 &m, const std::vector<TileBlob> &tiles, const std::vector<int4> &place,
                 uint8_t *rgb_out, int dst_w, int dst_h) {
    if (!m.supported()) return MIC_ERR_UNSUPPORTED;
    mic_hip_session *s = cur_default();
    const size_t npx = (size_t)m.tw * m.th;
    const size_t ntile = tiles.size();
    const size_t P = (size_t)m.planes(), bpp = m.bpp();
    // per-tile chunking keeps the unit workspace bounded
    const size_t per = std::min<size_t>(kMaxGridY / P, batch_units_for(npx, P));   // (tiles are a launch's grid y)
    struct Bufs { DevBuf planes, aux, d_out; ~Bufs() { planes.release(); aux.release(); d_out.release(); } } bufs;   // freed on every return path
    int rc;
    if ((rc = bufs.d_out.reserve((size_t)dst_w * dst_h * bpp + 64))) return rc;
    if (tiles.empty()) HIP_TRY(hipMemsetAsync(bufs.d_out.p, 0, (size_t)dst_w * dst_h * bpp, s->stream));   // nothing will write it
    std::vector<WsiPlane> pl; std::vector<uint8_t> bytes;
    for (size_t t0 = 0; t0 < ntile && rc == MIC_OK; t0 += per) {
        const size_t nt = std::min(per, ntile - t0);
        pl.clear(); bytes.clear();
        for (size_t k = 0; k < nt && rc == MIC_OK; k++) rc = parse_tile_blob(m, tiles[t0 + k].p, tiles[t0 + k].len, pl, bytes);
        if (rc) break;
        if ((rc = s->ensure(1, npx)) || (rc = s->io_comp.reserve(bytes.size() + 64))) break;
        if (!bytes.empty()) HIP_TRY(hipMemcpyAsync(s->io_comp.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, s->stream));
        rc = decode_planes(s, m, (const uint8_t *)s->io_comp.p, pl.data(), nt, place.data() + t0, bufs.planes, bufs.aux, bufs.d_out.p, dst_w);
    }
    if (rc == MIC_OK) {
        hipError_t e = hipMemcpy(rgb_out, bufs.d_out.p, (size_t)dst_w * dst_h * bpp, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = MIC_ERR_DEVICE;
    }
    return rc;
}

// ExtractTileBlob (wsiformat.go:230-241) for the given tiles (global indices): a flat file in memory, or a streaming reader's callback
// (its bytes then live in `keep`).  decode_box asks one source from several threads at once.
typedef std::function<int(const std::vector<size_t> &tiles, std::vector<TileBlob> &blobs, std::vector<uint8_t> &keep)> BlobSource;
BlobSource flat_source(const uint8_t *c, size_t len, const Mic3 &m) {
    return [c, len, &m](const std::vector<size_t> &tiles, std::vector<TileBlob> &blobs, std::vector<uint8_t> &) -> int {
        for (size_t gi : tiles) {
            if (gi >= m.total) return MIC_ERR_CORRUPT;
            const uint8_t *e = c + 48 + 20 * (size_t)m.nlev + 16 * gi;
            const uint64_t bo = get_u64(e), bl = get_u64(e + 8);
            if (bo > len || bl > len || m.data_off + bo + bl > len) return MIC_ERR_CORRUPT;
            blobs.push_back(TileBlob{ c + m.data_off + bo, (size_t)bl });
        }
        return MIC_OK;
    };
}

// the given tiles (global indices) of a MIC3 container, then decode_blobs
int decode_tiles(const BlobSource &src, const Mic3 &m, const std::vector<size_t> &tiles, const std::vector<int4> &place,
                 uint8_t *rgb_out, int dst_w, int dst_h) {
    std::vector<TileBlob> blobs; std::vector<uint8_t> keep;
    const int rc = src(tiles, blobs, keep);
    if (rc) return rc;
    return decode_blobs(m, blobs, place, rgb_out, dst_w, dst_h);
}

// ---- encode ----------------------------------------------------------------------------------------------------------------------
// tiles per slab: within the grid's y limit, a sub-batch of the unit codec, at most `cap` bytes of planes
size_t slab_tiles(const Mic3 &fmt, size_t cap) {
    const size_t P = (size_t)fmt.planes(), npx = (size_t)fmt.tw * fmt.th;
    return std::min<size_t>(kMaxGridY / P, std::max<size_t>(1, std::min<size_t>(batch_units_for(npx, P), cap / (P * npx * 2))));
}

// One coded slab of tiles t0 .. t0 + nt - 1: P plane records per tile at absolute addresses -- a stream inside the slab's packed
// streams [streams, streams + stream_bytes), a raw plane inside the slab's plane buffer.  Valid until the next slab.
struct Slab { size_t t0, nt; std::vector<WsiPlane> planes; const uint8_t *streams; uint64_t stream_bytes; };

// every tile of level L (image d_img on the device) in slabs of `per` tiles: the tile extraction fused with the colour transform and
// the plane statistics, the plane modes (compressWSIPlane, wsicompress.go:373-421), the unit codec over the non-constant planes;
// then sink(slab).  planes / stats: the caller's buffers for a slab's planes and their {min, max}.
int encode_level(mic_hip_session *s, const Mic3 &fmt, const void *d_img, const Level &L, DevBuf &planes, DevBuf &stats, size_t per,
                 const std::function<int(const Slab &)> &sink) {
    const size_t P = (size_t)fmt.planes(), npx = (size_t)fmt.tw * fmt.th;
    const size_t ntl = (size_t)L.tx * L.ty;
    Slab sl;
    int rc;
    for (size_t t0 = 0; t0 < ntl; t0 += per) {
        const size_t nt = std::min(per, ntl - t0);
        if ((rc = planes.reserve(nt * P * npx * 2 + 64)) || (rc = stats.reserve(nt * P * 8 + 64))) return rc;
        std::vector<uint32_t> st(nt * P * 2);
        for (size_t k = 0; k < nt * P; k++) { st[2 * k] = 0xFFFFFFFFu; st[2 * k + 1] = 0; }
        HIP_TRY(hipMemcpyAsync(stats.p, st.data(), st.size() * 4, hipMemcpyHostToDevice, s->stream));
        s->timer.reset(s->stream); s->timer.mark("k_wsi_tile_planes");
        launch_tile_planes(s->stream, fmt, d_img, L, t0, nt, (uint16_t *)planes.p, (uint32_t *)stats.p);
        s->timer.mark("end");
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(st.data(), stats.p, st.size() * 4, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        std::vector<mic_hip_unit> units;                                               // a unit per non-constant plane
        for (size_t p = 0; p < nt * P; p++)
            if (st[2 * p] != st[2 * p + 1]) units.push_back(mic_hip_unit{ p * npx, fmt.tw, fmt.th, (uint16_t)std::max<uint32_t>(st[2 * p + 1], 255u), 2 });   // :398-402
        std::vector<uint64_t> offs(units.size() + 1, 0); std::vector<int32_t> ust(units.size()), uns(units.size());
        sl.streams = nullptr;
        if (!units.empty()) {
            if ((rc = session_encode_enqueue(s, (const uint16_t *)planes.p, units.data(), (int)units.size()))) return rc;
            if ((rc = session_encode_finish(s, &sl.streams, offs.data(), ust.data(), uns.data()))) return rc;
        }
        sl.t0 = t0; sl.nt = nt; sl.stream_bytes = offs.back();
        sl.planes.resize(nt * P);
        for (size_t p = 0, u = 0; p < nt * P; p++) {
            const uint32_t mn = st[2 * p], mx = st[2 * p + 1];
            WsiPlane &wp = sl.planes[p];
            if (mn == mx) { wp = WsiPlane{ (uint8_t)(mn == 0 ? 0 : 1), (uint16_t)mn, 0, 0 }; continue; }
            if (ust[u] == MIC_OK) wp = WsiPlane{ 2, 0, (uint64_t)(uintptr_t)sl.streams + offs[u], offs[u + 1] - offs[u] };
            else if (ust[u] == MIC_ERR_USE_RLE || ust[u] == MIC_ERR_INCOMPRESSIBLE)                   // raw fallback, :403-414
                wp = WsiPlane{ 3, 0, (uint64_t)(uintptr_t)((const uint16_t *)planes.p + p * npx), npx * 2 };
            else return ust[u];
            u++;
        }
        if ((rc = sink(sl))) return rc;
    }
    return MIC_OK;
}

// Tile blobs of one level that lie back to back in the file: tile `first` (global index) and the lens.size() tiles after it
struct TileRun { size_t first = 0; std::vector<uint8_t> bytes; std::vector<uint64_t> lens; };
struct SlabBufs {                                    // a slab's planes and stats, its assembled blobs and their records
    DevBuf planes, stats, payload, recs;
    void release() { planes.release(); stats.release(); payload.release(); recs.release(); }
    ~SlabBufs() { release(); }
};

// every tile of level L appended to `run` (the host-bound paths): each slab's blobs are assembled on the device and come to the
// host in one copy
int code_level(mic_hip_session *s, const Mic3 &fmt, const void *d_img, const Level &L, SlabBufs &b, size_t per, TileRun &run) {
    return encode_level(s, fmt, d_img, L, b.planes, b.stats, per, [&](const Slab &sl) -> int {
        const size_t n0 = run.lens.size(), b0 = run.bytes.size();
        uint64_t total = 0;
        run.lens.resize(n0 + sl.nt);
        int rc = assemble_tiles(s, sl.planes.data(), sl.nt, (size_t)fmt.planes(), 0, b.payload, b.recs, run.lens.data() + n0, &total);
        if (rc) return rc;
        run.bytes.resize(b0 + (size_t)total);
        if (total) HIP_TRY(hipMemcpy(run.bytes.data() + b0, b.payload.p, (size_t)total, hipMemcpyDeviceToHost));
        return MIC_OK;
    });
}

// ---- MIC3 over the devices of mic_hip_set_devices: the slide in bands of tile rows (parallel.wsi_band_plan) ----------------------
// A level-k tile covers 2^k tile rows of level 0, so a band of a multiple of tile_h << K rows holds whole tiles of levels 0..K and
// the 2x2 box filter never reaches across its edge: each band is coded as a slide of its own up to level K.  K is the largest level
// whose blocks of tile_h << K rows still give every shard one; shard b takes blocks [nb * b / shards, nb * (b + 1) / shards)
// (shard_range), clipped to the slide.  Returns K; row_first[0 .. shards] are the bands' first rows.
int band_plan(int height, int tile_h, int nlev, int shards, int *row_first) {
    auto blocks = [&](int k) { const int64_t a = (int64_t)tile_h << k; return ((int64_t)height + a - 1) / a; };
    int k = nlev - 1;
    while (k > 0 && blocks(k) < shards) k--;
    const int64_t a = (int64_t)tile_h << k, nb = blocks(k);
    for (int b = 0; b <= shards; b++) row_first[b] = (int)std::min<int64_t>(height, nb * b / shards * a);
    return k;
}

struct PinnedHost {                                  // staging for the rows that go from the bands to devices[0]
    void *p = nullptr;
    ~PinnedHost() { if (p) (void)hipHostFree(p); }
};

// mic_hip_wsi_compress_ex with shard b coding rows [row_first[b], row_first[b + 1]) on the b-th listed device (micapi::over_devices
// with the bands as its cut): levels 0..K of its band, each tile with the single-device tile path; the default device -- the first
// listed -- codes levels K + 1 .. L - 1 from the bands' rows of level K + 1 (of level K when
// tile_h is odd: a band of an odd number of level-K rows does not end on a row pair).  Within a level the tiles of band b are one
// contiguous run of the tile table, so the lengths scan into the file's offsets and each shard writes its own runs of `out`.
// One band (band_plan with one shard: K = L - 1) is the one-device slide.
int wsi_compress_bands(const uint8_t *px, const Mic3 &fmt, const std::vector<Level> &lv, int K, const std::vector<int> &row_first,
                       uint8_t *out, size_t out_cap, size_t *out_len) {
    const int nlev = (int)lv.size(), shards = (int)row_first.size() - 1, width = fmt.w, tile_h = fmt.th;
    const size_t bpp = fmt.bpp();
    size_t total_tiles = 0;
    for (const Level &l : lv) total_tiles += (size_t)l.tx * l.ty;
    const size_t hdr = 48 + 20 * (size_t)nlev + 16 * total_tiles;
    if (out_cap < hdr) return MIC_ERR_CAPACITY;
    int rc = ensure_device();
    if (rc) return rc;
    // the level the default device starts the top of the pyramid from: -1 none, 0 the caller's slide itself, else rows gathered from the bands
    const int top = nlev > K + 1 ? ((tile_h & 1) ? K : K + 1) : -1;
    PinnedHost stage;
    if (top > 0 && hipHostMalloc(&stage.p, (size_t)lv[(size_t)top].w * lv[(size_t)top].h * bpp + 64, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError(); return MIC_ERR_NOMEM;
    }
    std::vector<std::vector<TileRun>> runs((size_t)shards);                   // shard b's runs: levels 0..K of its band (band 0: + the top)
    // level L of an image on the device as one more run of `rs` (L.first: the level's first tile in the file)
    auto code_run = [&](mic_hip_session *s, const void *d_img, const Level &L, std::vector<TileRun> &rs) -> int {
        SlabBufs bufs;                                                          // (freed behind each level)
        rs.emplace_back();
        rs.back().first = (size_t)L.first;
        return code_level(s, fmt, d_img, L, bufs, slab_tiles(fmt, (size_t)8 << 30), rs.back());
    };
    rc = over_devices(row_first, [&](mic_hip_session *s, int y0, int y1) -> int {
        const int rows = y1 - y0;
        const size_t b = (size_t)(std::upper_bound(row_first.begin(), row_first.end(), y0) - row_first.begin()) - 1;   // the band that starts at y0
        std::vector<Level> bl;                                                  // the band's levels 0..K; first: global tile index
        for (int k = 0; k <= K; k++) {
            const int h = rows >> k;
            bl.push_back(Level{ lv[(size_t)k].w, h, lv[(size_t)k].tx, (h + tile_h - 1) / tile_h, lv[(size_t)k].first + (y0 >> k) / tile_h * lv[(size_t)k].tx });
        }
        int r = s->ensure(1, (size_t)fmt.tw * fmt.th);
        if (r) return r;
        struct Bufs { std::vector<DevBuf> img; ~Bufs() { for (auto &d : img) d.release(); } } bufs;   // freed on every return path
        std::vector<DevBuf> &img = bufs.img;
        img.resize((size_t)K + 2);
        if ((r = img[0].reserve((size_t)width * rows * bpp + 64))) return r;
        HIP_TRY(hipMemcpyAsync(img[0].p, px + (size_t)y0 * width * bpp, (size_t)width * rows * bpp, hipMemcpyHostToDevice, s->stream));
        for (int k = 1; k <= K; k++) {
            if ((r = img[(size_t)k].reserve((size_t)bl[(size_t)k].w * bl[(size_t)k].h * bpp + 64))) return r;
            launch_downsample(s->stream, fmt, img[(size_t)k - 1].p, bl[(size_t)k - 1].w, img[(size_t)k].p, bl[(size_t)k].w, bl[(size_t)k].h);
        }
        HIP_TRY(hipGetLastError());
        if (top > 0) {                                                          // this band's rows of level `top`, to their place in the stage
            const int th = rows >> top, tw = lv[(size_t)top].w;
            if (top == K + 1) {
                if ((r = img[(size_t)K + 1].reserve((size_t)tw * th * bpp + 64))) return r;
                launch_downsample(s->stream, fmt, img[(size_t)K].p, lv[(size_t)K].w, img[(size_t)K + 1].p, tw, th);
                HIP_TRY(hipGetLastError());
            }
            if (th > 0)
                HIP_TRY(hipMemcpyAsync((uint8_t *)stage.p + (size_t)(y0 >> top) * tw * bpp, img[(size_t)top].p, (size_t)tw * th * bpp,
                                       hipMemcpyDeviceToHost, s->stream));
            HIP_TRY(hipStreamSynchronize(s->stream));
        }
        for (int k = 0; k <= K && r == MIC_OK; k++) r = code_run(s, img[(size_t)k].p, bl[(size_t)k], runs[b]);
        return r;
    });
    if (rc) return rc;
    if (top >= 0) {                                                             // the top of the pyramid on the default device
        DefaultLease lease;
        if ((rc = lease.acquire())) return rc;
        mic_hip_session *s = lease.s;
        if ((rc = s->ensure(1, (size_t)fmt.tw * fmt.th))) return rc;
        struct Bufs { std::vector<DevBuf> img; ~Bufs() { for (auto &d : img) d.release(); } } bufs;
        std::vector<DevBuf> &img = bufs.img;
        img.resize((size_t)nlev);
        const Level &T = lv[(size_t)top];
        if ((rc = img[(size_t)top].reserve((size_t)T.w * T.h * bpp + 64))) return rc;
        HIP_TRY(hipMemcpyAsync(img[(size_t)top].p, top ? (const uint8_t *)stage.p : px, (size_t)T.w * T.h * bpp, hipMemcpyHostToDevice, s->stream));
        for (int i = top + 1; i < nlev; i++) {
            if ((rc = img[(size_t)i].reserve((size_t)lv[(size_t)i].w * lv[(size_t)i].h * bpp + 64))) return rc;
            launch_downsample(s->stream, fmt, img[(size_t)i - 1].p, lv[(size_t)i - 1].w, img[(size_t)i].p, lv[(size_t)i].w, lv[(size_t)i].h);
        }
        HIP_TRY(hipGetLastError());
        for (int i = K + 1; i < nlev && rc == MIC_OK; i++) rc = code_run(s, img[(size_t)i].p, lv[(size_t)i], runs[0]);
        if (rc) return rc;
    }
    // the container: every tile's length, the capacity check, the offsets; then each shard copies its runs to their place
    std::vector<uint64_t> lens(total_tiles, 0);
    for (const auto &rs : runs)
        for (const TileRun &run : rs) std::copy(run.lens.begin(), run.lens.end(), lens.begin() + (long)run.first);
    std::vector<uint64_t> off(total_tiles + 1, 0);
    for (size_t t = 0; t < total_tiles; t++) off[t + 1] = off[t] + lens[t];
    if (out_cap < hdr + off[total_tiles]) return MIC_ERR_CAPACITY;
    put_mic3_index(out, fmt, lv, lens);
    uint8_t *body = out + hdr;
    rc = run_parallel(shards, [&](int b) -> int {
        for (const TileRun &run : runs[(size_t)b]) memcpy(body + off[run.first], run.bytes.data(), run.bytes.size());
        return MIC_OK;
    });
    if (rc) return rc;
    *out_len = hdr + (size_t)off[total_tiles];
    return MIC_OK;
}

// Tiles [tx0, tx1] x [ty0, ty1] of level L into dst, an image of bw x bh pixels whose corner is the level's (bx, by = ty0 * th).
// One device, or -- when the box spans two tile rows or more, several devices are listed and the call is not nested -- one
// contiguous range of tile rows per device (micapi::over_devices, weighted by pixels), each decoded into its own rows of dst.
int decode_box(const BlobSource &src, const Mic3 &m, const Level &L, int tx0, int tx1, int ty0, int ty1, int bx, int bw, int bh,
               uint8_t *dst) {
    const int by = ty0 * m.th;
    const int nrows = ty1 - ty0 + 1;
    // tile row ty0 + r weighs its pixels; rows ty0 + r0 .. ty0 + r1 - 1 on one session
    return over_devices(nrows, [&](int r) { return (uint64_t)bw * (uint64_t)std::min(m.th, by + bh - (ty0 + r) * m.th); }, [&](mic_hip_session *, int r0, int r1) -> int {
        r0 += ty0; r1 += ty0;
        const int ys = r0 * m.th, hs = std::min(r1 * m.th, by + bh) - ys;
        std::vector<size_t> tiles; std::vector<int4> place;
        for (int ty = r0; ty < r1; ty++) for (int tx = tx0; tx <= tx1; tx++) {
            const int aw = std::min(m.tw, L.w - tx * m.tw), ah = std::min(m.th, L.h - ty * m.th);
            if (aw <= 0 || ah <= 0) continue;
            tiles.push_back((size_t)L.first + (size_t)ty * L.tx + tx);
            place.push_back(make_int4(tx * m.tw - bx, ty * m.th - ys, aw, ah));
        }
        return decode_tiles(src, m, tiles, place, dst + (size_t)(ys - by) * bw * m.bpp(), bw, hs);   // (on the session this thread now holds)
    });
}
int decode_box(const uint8_t *c, size_t len, const Mic3 &m, const Level &L, int tx0, int tx1, int ty0, int ty1, int bx, int bw, int bh,
               uint8_t *dst) {
    return decode_box(flat_source(c, len, m), m, L, tx0, tx1, ty0, ty1, bx, bw, bh, dst);
}

// DecompressWSITile on a parsed header, the blobs from `src` (mic_hip_wsi_decompress_tile: the flat file; the streaming reader)
int wsi_tile(const BlobSource &src, const Mic3 &m, int level, int tile_x, int tile_y, uint8_t *rgb_out, size_t out_cap, int *out_w, int *out_h) {
    int rc;
    if (level < 0 || level >= m.nlev) return MIC_ERR_ARGS;
    const Level &L = m.lv[(size_t)level];
    if (tile_x < 0 || tile_x >= L.tx || tile_y < 0 || tile_y >= L.ty) return MIC_ERR_ARGS;
    const int aw = std::min(m.tw, L.w - tile_x * m.tw), ah = std::min(m.th, L.h - tile_y * m.th);
    if (aw <= 0 || ah <= 0) return MIC_ERR_CORRUPT;
    if (!m.supported()) return MIC_ERR_UNSUPPORTED;
    if ((size_t)aw * ah * m.bpp() > out_cap) return MIC_ERR_CAPACITY;
    if (out_w) *out_w = aw; if (out_h) *out_h = ah;
    DefaultLease lease;
    if ((rc = lease.acquire())) return rc;
    std::vector<size_t> tiles(1, (size_t)L.first + (size_t)tile_y * L.tx + tile_x);
    std::vector<int4> place(1, make_int4(0, 0, aw, ah));
    return decode_tiles(src, m, tiles, place, rgb_out, aw, ah);
}

// DecompressWSIRegion on a parsed header, the blobs from `src`
int wsi_region(const BlobSource &src, const Mic3 &m, int level, int x, int y, int w, int h, uint8_t *rgb_out, size_t out_cap,
               int *out_w, int *out_h) {
    int rc;
    if (level < 0 || level >= m.nlev || x < 0 || y < 0) return MIC_ERR_ARGS;
    const Level &L = m.lv[(size_t)level];
    if (L.w <= 0 || L.h <= 0 || m.tw <= 0 || m.th <= 0) return MIC_ERR_CORRUPT;
    if ((size_t)L.tx * m.tw < (size_t)L.w || (size_t)L.ty * m.th < (size_t)L.h) return MIC_ERR_CORRUPT;
    if ((int64_t)x + w > L.w) w = L.w - x;                                                  // :232-237
    if ((int64_t)y + h > L.h) h = L.h - y;
    if (w <= 0 || h <= 0) return MIC_ERR_ARGS;                                              // "MIC3: empty region"
    if (!m.supported()) return MIC_ERR_UNSUPPORTED;
    const size_t bpp = m.bpp();
    if ((size_t)w * h * bpp > out_cap) return MIC_ERR_CAPACITY;
    const int tx0 = x / m.tw, ty0 = y / m.th, tx1 = (x + w - 1) / m.tw, ty1 = (y + h - 1) / m.th;
    const int bx = tx0 * m.tw, by = ty0 * m.th;
    const int bw = std::min((tx1 + 1) * m.tw, L.w) - bx, bh = std::min((ty1 + 1) * m.th, L.h) - by;
    std::vector<uint8_t> box((size_t)bw * bh * bpp);
    if ((rc = decode_box(src, m, L, tx0, tx1, ty0, ty1, bx, bw, bh, box.data()))) return rc;
    for (int r = 0; r < h; r++)
        memcpy(rgb_out + (size_t)r * w * bpp, box.data() + ((size_t)(y - by + r) * bw + (size_t)(x - bx)) * bpp, (size_t)w * bpp);
    if (out_w) *out_w = w;
    if (out_h) *out_h = h;
    return MIC_OK;
}

// ---- patches -----------------------------------------------------------------------------------------------------------------
// The plan of a patch call.  A unit is a tile to entropy-decode (slide: index into the call's slide list, 0 for the one-slide calls;
// tile: its index as the door counts it); a piece is one patch-tile overlap (RectPiece, mic_rects.h: rect = the patch).  units:
// ascending by slide, then tile, each once.  pieces: sorted by unit (stable: patch order inside a unit).
struct PatchUnit { uint32_t slide; uint64_t tile; };
struct PatchPlan { std::vector<PatchUnit> units; std::vector<RectPiece> pieces; };
struct PlanKey { PatchUnit u; RectPiece pc; };

// Patch i = [px, px + pw) x [py, py + ph) clipped to a level of level_w x level_h pixels and cut into its overlaps with the level's
// tiles (tw x th, tiles_x a row): one key per overlap, tile = first + ty * tiles_x + tx.  What lies outside the level has no piece.
void plan_clip(std::vector<PlanKey> &all, uint32_t slide, int level_w, int level_h, int64_t tw, int64_t th, int64_t tiles_x, int64_t first,
               int32_t i, int64_t px, int64_t py, int pw, int ph) {
    const int64_t x0 = std::max<int64_t>(px, 0), x1 = std::min<int64_t>(px + pw, level_w);
    const int64_t y0 = std::max<int64_t>(py, 0), y1 = std::min<int64_t>(py + ph, level_h);
    if (x0 >= x1 || y0 >= y1) return;
    for (int64_t ty = y0 / th; ty <= (y1 - 1) / th; ty++) for (int64_t tx = x0 / tw; tx <= (x1 - 1) / tw; tx++) {
        const int64_t ax = std::max(x0, tx * tw), bx = std::min(x1, (tx + 1) * tw), ay = std::max(y0, ty * th), by = std::min(y1, (ty + 1) * th);
        all.push_back(PlanKey{ PatchUnit{ slide, (uint64_t)(first + ty * tiles_x + tx) },
                               RectPiece{ i, 0, (int32_t)(ax - tx * tw), (int32_t)(ay - ty * th), (int32_t)(ax - px), (int32_t)(ay - py), (int32_t)(bx - ax), (int32_t)(by - ay) } });
    }
}
// the keys in unit order ...
int plan_sort(std::vector<PlanKey> &all) {
    if (all.size() > 0x7FFFFFFFu) return MIC_ERR_UNSUPPORTED;                              // (pieces are a launch's grid x)
    std::stable_sort(all.begin(), all.end(), [](const PlanKey &a, const PlanKey &b) { return a.u.slide != b.u.slide ? a.u.slide < b.u.slide : a.u.tile < b.u.tile; });
    return MIC_OK;
}
// ... and those of the slides that `keep` accepts as the plan
template <class Keep>
void plan_group(const std::vector<PlanKey> &all, PatchPlan &plan, Keep keep) {
    plan.units.clear(); plan.pieces.clear();
    for (const PlanKey &k : all) {
        if (!keep(k.u.slide)) continue;
        if (plan.units.empty() || plan.units.back().slide != k.u.slide || plan.units.back().tile != k.u.tile) plan.units.push_back(k.u);
        plan.pieces.push_back(k.pc);
        plan.pieces.back().unit = (uint32_t)(plan.units.size() - 1);
    }
}

// The plan of n patches of pw x ph pixels, patch i at (xy[2i], xy[2i + 1]), in one level of level_w x level_h pixels (tiles of
// tw x th): slide 0, tile = ty * tiles_x + tx inside the level.
int plan_patches(int level_w, int level_h, int tw, int th, const int32_t *xy, int n, int pw, int ph, PatchPlan &plan) {
    std::vector<PlanKey> all;
    for (int i = 0; i < n; i++) plan_clip(all, 0, level_w, level_h, tw, th, ((int64_t)level_w + tw - 1) / tw, 0, i, xy[2 * (size_t)i], xy[2 * (size_t)i + 1], pw, ph);
    const int rc = plan_sort(all);
    if (rc) return rc;
    plan_group(all, plan, [](uint32_t) { return true; });
    return MIC_OK;
}

// ---- scaled patches: the judgement of a scale -----------------------------------------------------------------------------------
// The scale of a _scaled door's call, num / den of a level pixel an output pixel: as the caller gave it, and behind judge() reduced,
// with sw x sh, the source rectangle of a pw x ph patch.  unit(): 1 / 1, the _as door itself.
struct Scale {
    int num = 1, den = 1, sw = 0, sh = 0;
    bool unit() const { return num == den; }
    // mic_hip_wsi_scaled_extent: the only place a scale is judged
    int judge(int pw, int ph) {
        if (pw <= 0 || ph <= 0 || num <= 0 || den <= 0) return MIC_ERR_ARGS;
        int a = num, b = den;
        while (b) { const int t = a % b; a = b; b = t; }
        num /= a; den /= a;
        if (den > num || (int64_t)num > 16 * (int64_t)den || num > 1024) return MIC_ERR_ARGS;
        // (the kernel's j * num, j <= pw, is 32 bits wide; a tensor that wide is nobody's patch)
        if (((int64_t)pw + 1) * num > 0x7FFFFFFF || ((int64_t)ph + 1) * num > 0x7FFFFFFF) return MIC_ERR_UNSUPPORTED;
        sw = (int)(((int64_t)pw * num + den - 1) / den); sh = (int)(((int64_t)ph * num + den - 1) / den);
        return MIC_OK;
    }
};

// What the three one-slide patch entry points check of their arguments before a device is touched; o = the output description,
// *need = bytes of the patch tensor.  sc (the _scaled doors): the call's scale, judged right behind pw, ph and n.
int patch_args(const Mic3 &m, int level, const int32_t *xy, int n, int pw, int ph, const mic_hip_out_spec *spec, OutFormat &o, size_t out_cap, size_t *need,
               Scale *sc = nullptr) {
    if (level < 0 || level >= m.nlev || pw <= 0 || ph <= 0 || n < 0 || (n > 0 && !xy)) return MIC_ERR_ARGS;
    if (sc) { const int src = sc->judge(pw, ph); if (src) return src; }
    if (!m.supported()) return MIC_ERR_UNSUPPORTED;
    const int orc = o.make(spec, m.channels, m.bps, 1);
    if (orc) return orc;
    const Level &L = m.lv[(size_t)level];
    if (L.w <= 0 || L.h <= 0 || m.tw <= 0 || m.th <= 0) return MIC_ERR_CORRUPT;
    if ((size_t)L.tx * m.tw < (size_t)L.w || (size_t)L.ty * m.th < (size_t)L.h) return MIC_ERR_CORRUPT;
    return tensor_bytes(n, 1, ph, pw, o.pixel(), out_cap, need);
}

// Where a call's tiles come from: the planes of units u0 .. u0 + nt - 1 of the plan as nt * P records over *base (device), and each
// tile's own host-side status: a tile that fails on the host (a blob that does not parse) still has its P records, constant zero.
typedef std::function<int(size_t u0, size_t nt, const uint8_t **base, std::vector<WsiPlane> &pl, int32_t *tile_status)> PatchSlabs;
// how many tiles a sub-batch may hold when its largest has npx pixels
typedef std::function<size_t(size_t npx)> SlabCeiling;
// ... for blobs through the unit codec's workspace (tiles are a launch's grid y)
SlabCeiling blob_ceiling(size_t P) { return [P](size_t npx) { return std::min<size_t>(kMaxGridY / P, batch_units_for(npx, P)); }; }

// ---- the tile cache in a patch call (mic_tile_cache.h) ----------------------------------------------------------------------------
// What a door with caches attached hands the core instead of its plan.  split() locks the caches of the call (address order, behind
// the readers' locks), lets each index judge its tiles -- hit, miss or bypassed -- and cuts the plan in two: `decode`, the units to
// entropy-decode (misses, bypassed, and tiles of owners without a cache) with the pieces of those that are NOT kept, which the core
// gathers from the slab as ever; and per cache the pieces of its hits and misses, gathered out of the arena in one launch behind
// the sub-batches.  A miss's planes go into its slot by one k_wsi_cache_fill launch behind its sub-batch's decode.  The locks are held
// until the object dies, which is behind the call's final synchronise; a call that fails before finish() is undone there.
struct CacheOwner { mic_hip_tile_cache *c; uint64_t owner; uint64_t first; };               // first: added to a unit's tile to make the global tile index
struct CachePlan {
    struct Use {
        mic_hip_tile_cache *c; bool usable = false, planned = false;
        std::vector<SlotIndex::Key> keys; std::vector<size_t> units;                        // its units of the full plan, plan order
        std::vector<uint8_t> outcome; std::vector<uint32_t> slot;
        std::vector<GatherPiece> pieces; int mw = 1, mh = 1;
        std::vector<uint32_t> written;                                                      // slots a fill launch of this call has been queued for
    };
    std::vector<Use> uses;
    std::vector<std::unique_lock<std::mutex>> locks;
    PatchPlan decode;
    std::vector<size_t> full_of;                                                            // decode unit -> unit of the full plan
    struct Kept { int32_t use; uint32_t slot; };                                            // use -1: not kept
    std::vector<Kept> kept;                                                                 // per decode unit
    std::vector<CacheFill> fills; std::vector<size_t> fill_first;                           // fills[fill_first[d] .. fill_first[d + 1]): decode unit d's (0 or 1)
    GatherKind kind = kGatherPxU8;
    mic_hip_session *s = nullptr; bool launched = false, done = false;
    size_t cached_pieces() const { size_t n = 0; for (const Use &u : uses) n += u.pieces.size(); return n; }
    size_t behind_bytes() const { return cached_pieces() * sizeof(GatherPiece) + fills.size() * sizeof(CacheFill); }

    // um[u]: unit u's header; who(u): its owner's cache (c NULL: none)
    template <class Who>
    int split(mic_hip_session *ses, const PatchPlan &plan, const std::vector<const Mic3 *> &um, int pw, int ph, const OutFormat &o, Who &&who) {
        s = ses;
        const size_t nu = plan.units.size();
        std::vector<mic_hip_tile_cache *> cs;
        std::vector<CacheOwner> ow(nu);
        for (size_t u = 0; u < nu; u++) { ow[u] = who(u); if (ow[u].c) cs.push_back(ow[u].c); }
        std::sort(cs.begin(), cs.end(), std::less<mic_hip_tile_cache *>());
        cs.erase(std::unique(cs.begin(), cs.end()), cs.end());
        uses.resize(cs.size());
        locks.reserve(cs.size());
        for (size_t k = 0; k < cs.size(); k++) { uses[k].c = cs[k]; locks.emplace_back(cs[k]->mu); }
        int rc;
        for (Use &us : uses) if ((rc = us.c->ensure_arena(s->device, &us.usable))) return rc;
        std::vector<int32_t> use_of(nu, -1); std::vector<size_t> at(nu, 0);
        for (size_t u = 0; u < nu; u++) {
            if (!ow[u].c) continue;
            const int32_t k = (int32_t)(std::lower_bound(cs.begin(), cs.end(), ow[u].c, std::less<mic_hip_tile_cache *>()) - cs.begin());
            use_of[u] = k; at[u] = uses[(size_t)k].units.size();
            uses[(size_t)k].units.push_back(u);
            uses[(size_t)k].keys.push_back(SlotIndex::Key{ ow[u].owner, ow[u].first + plan.units[u].tile });
        }
        for (Use &us : uses) {
            us.outcome.assign(us.keys.size(), SlotIndex::kBypass); us.slot.assign(us.keys.size(), SlotIndex::kNoSlot);
            if (us.usable) us.c->index.plan(us.keys.data(), us.keys.size(), us.outcome.data(), us.slot.data());
            else us.c->index.bypass_all(us.keys.size());
            us.planned = true;
        }
        if (!uses.empty()) kind = uses[0].c->channels == 3 ? kGatherPxRGB : uses[0].c->bps == 16 ? kGatherPxU16 : kGatherPxU8;
        // the plan in two
        std::vector<size_t> dec_of(nu, ~(size_t)0);
        fill_first.assign(1, 0);
        for (size_t u = 0; u < nu; u++) {
            const int32_t k = use_of[u];
            const uint8_t oc = k < 0 ? (uint8_t)SlotIndex::kBypass : uses[(size_t)k].outcome[at[u]];
            if (oc == SlotIndex::kHit) continue;
            dec_of[u] = decode.units.size();
            decode.units.push_back(plan.units[u]);
            full_of.push_back(u);
            kept.push_back(oc == SlotIndex::kMiss ? Kept{ k, uses[(size_t)k].slot[at[u]] } : Kept{ -1, SlotIndex::kNoSlot });
            if (oc == SlotIndex::kMiss) {
                const mic_hip_tile_cache *c = uses[(size_t)k].c;
                fills.push_back(CacheFill{ 0, (uint64_t)(uintptr_t)c->arena + (uint64_t)kept.back().slot * c->slot_bytes, (uint32_t)((size_t)um[u]->tw * um[u]->th), 0 });
            }
            fill_first.push_back(fills.size());
        }
        for (const RectPiece &p : plan.pieces) {
            const size_t u = p.unit;
            const int32_t k = use_of[u];
            const uint8_t oc = k < 0 ? (uint8_t)SlotIndex::kBypass : uses[(size_t)k].outcome[at[u]];
            if (oc == SlotIndex::kBypass) { decode.pieces.push_back(p); decode.pieces.back().unit = (uint32_t)dec_of[u]; continue; }
            Use &us = uses[(size_t)k];
            const uint64_t bpp = um[u]->bpp();
            const PieceDst pd = piece_dst(p, pw, ph, o);
            us.pieces.push_back(GatherPiece{ (uint64_t)us.slot[at[u]] * us.c->slot_bytes + ((uint64_t)p.sy * (uint64_t)um[u]->tw + (uint64_t)p.sx) * bpp, pd.dst,
                                             um[u]->tw, pd.dstride, p.w, p.h, 0, (int32_t)plan.units[u].slide });
            us.mw = std::max(us.mw, p.w); us.mh = std::max(us.mh, p.h);
        }
        return MIC_OK;
    }
    // the call has its statuses (tile_status: per decode unit) and the stream is idle: a failed tile is not kept; the rest stands
    void finish(const std::vector<int32_t> &tile_status) {
        for (size_t d = 0; d < kept.size(); d++)
            if (kept[d].use >= 0 && tile_status[d] != MIC_OK) {
                Use &us = uses[(size_t)kept[d].use];
                const size_t i = (size_t)(std::find(us.units.begin(), us.units.end(), full_of[d]) - us.units.begin());
                us.c->index.release(us.keys[i]);
            }
        for (Use &us : uses) us.c->index.commit();
        done = true;
    }
    ~CachePlan() {
        if (done) return;
        if (launched && s && s->stream) (void)hipStreamSynchronize(s->stream);             // (the slots are not let go while something may write them)
        for (Use &us : uses) {
            if (!us.planned) continue;
            us.c->index.rollback();
            for (uint32_t q : us.written) us.c->index.spoil(q);                             // (what a queued fill has overwritten is nobody's any more)
        }
    }
};

// The core of every patch call: the plan's pieces into d_out ([patch][ph][pw] pixels of the slides' format or of o's, an address s's
// device can write: patch_pointer; what no piece covers is 0, or o's pad) on a session the caller holds.  um[u]: the header unit u's tile is coded
// under (all of one sample format).  The skeleton is the one the strip and MIC2 crop readers run (mic_rects.h); here are the rule -- as
// many tiles as `ceiling` allows of the largest, a tile P * tw * th samples of the slab -- and the decode (decode_plane_slab).
// tile_status[u]: the source's code for the tile, else its first failing plane's; *nslab: sub-batches.
int read_patches(mic_hip_session *s, const PatchPlan &plan, const std::vector<const Mic3 *> &um, int pw, int ph, const OutFormat &o, const SlabCeiling &ceiling,
                 const PatchSlabs &source, void *d_out, size_t need, std::vector<int32_t> &tile_status, uint64_t *nslab, CachePlan *cr = nullptr) {
    const size_t nu = plan.units.size();
    int rc;
    if ((rc = s->ensure(1, 1))) return rc;                                                  // (the session's stream)
    if ((rc = fill_pad(s->stream, o, d_out, need))) return rc;                              // outside the levels, refused slides and patches
    tile_status.assign(nu, MIC_OK);
    *nslab = 0;
    if (nu == 0 && !(cr && cr->cached_pieces())) { HIP_TRY(hipStreamSynchronize(s->stream)); if (cr) cr->finish(tile_status); return MIC_OK; }
    const size_t P = nu ? (size_t)um[0]->planes() : 1;                                      // (cr: `plan` is what is left to decode, nothing when every tile hit)
    const GatherKind kind = P == 3 ? kGatherRGB : (nu && um[0]->bps == 16) ? kGatherU16 : kGatherU8;
    std::vector<size_t> px(nu);
    for (size_t u = 0; u < nu; u++) px[u] = (size_t)um[u]->tw * um[u]->th;
    std::vector<std::pair<size_t, size_t>> caps;                                            // (tile size -> tiles a sub-batch holds: the ceiling is asked once per size)
    auto cap = [&](size_t, size_t npx) {                                                    // (what a launch takes is inside the ceiling)
        for (const auto &c : caps) if (c.first == npx) return c.second;
        caps.emplace_back(npx, ceiling(npx));
        return caps.back().second;
    };
    const RectBatches L = rect_batches(nu, [&](size_t i0) { return next_sub_batch(i0, nu, [&](size_t u) { return px[u]; }, cap, CutRule{ ~(size_t)0 }); },
                                       [&](size_t u) { return P * px[u]; }, plan.pieces, pw, ph, [&](size_t u) { return UnitStride{ um[u]->tw, (int32_t)px[u] }; },
                                       [&](size_t u) { return plan.units[u].slide; }, o);
    if ((rc = s->wsi_planes.reserve(L.slab_max * 2 + 64))) return rc;
    // with caches: behind the gather list lie the pieces of the cached tiles, cache by cache, and the fill records of the kept ones
    const size_t behind = cr ? cr->behind_bytes() : 0;
    if ((rc = upload_gather(s, L, o, behind))) return rc;
    const GatherPiece *d_cached = (const GatherPiece *)((const char *)s->pieces.p + gather_bytes(L));
    const CacheFill *d_fills = cr ? (const CacheFill *)(d_cached + cr->cached_pieces()) : nullptr;
    if (cr) {
        for (size_t d = 0; d < nu; d++) if (cr->kept[d].use >= 0) cr->fills[cr->fill_first[d]].src = L.slab_off[d];
        const GatherPiece *at = d_cached;
        for (const CachePlan::Use &us : cr->uses) {
            if (!us.pieces.empty()) HIP_TRY(hipMemcpyAsync((void *)at, us.pieces.data(), us.pieces.size() * sizeof(GatherPiece), hipMemcpyHostToDevice, s->stream));
            at += us.pieces.size();
        }
        if (!cr->fills.empty()) HIP_TRY(hipMemcpyAsync((void *)d_fills, cr->fills.data(), cr->fills.size() * sizeof(CacheFill), hipMemcpyHostToDevice, s->stream));
    }
    std::vector<WsiPlane> pl; std::vector<int32_t> pst;
    for (size_t b = 0; b < L.subs(); b++, ++*nslab) {
        const size_t u0 = L.cuts[b], nt = L.cuts[b + 1] - u0;
        const uint8_t *base = nullptr;
        pl.clear();
        if ((rc = source(u0, nt, &base, pl, tile_status.data() + u0))) return rc;
        pst.assign(nt * P, MIC_OK);
        if ((rc = decode_plane_slab(s, base, pl.data(), nt * P, [&](size_t q) {
                const size_t u = u0 + q / P;
                return PlaneAt{ L.slab_off[u] + (q % P) * px[u], um[u]->tw, um[u]->th };
            }, s->wsi_planes, L.slab_max, pst.data()))) return rc;
        for (size_t q = 0; q < nt * P; q++) if (tile_status[u0 + q / P] == MIC_OK) tile_status[u0 + q / P] = pst[q];
        s->timer.reset(s->stream);                                                          // (every unit has a piece; no more than 2^31 - 1 in all: plan_sort)
        if (cr && cr->fill_first[u0 + nt] > cr->fill_first[u0]) {                           // the kept tiles of this sub-batch into their slots
            const size_t f0 = cr->fill_first[u0], nf = cr->fill_first[u0 + nt] - f0;
            size_t max_px = 0;
            for (size_t d = u0; d < u0 + nt; d++) if (cr->kept[d].use >= 0) { max_px = std::max(max_px, px[d]); cr->uses[(size_t)cr->kept[d].use].written.push_back(cr->kept[d].slot); }
            cr->launched = true;
            s->timer.mark("k_wsi_cache_fill");
            launch_cache_fill(s->stream, cr->kind, (const uint16_t *)s->wsi_planes.p, d_fills + f0, nf, max_px);
        }
        gather_units(s, "k_wsi_gather_patches", kind, s->wsi_planes.p, L, b, d_out, o, (size_t)ph * (size_t)pw, behind);
        s->timer.mark("end");
        HIP_TRY(hipGetLastError());                                                         // (the next sub-batch follows on the stream; decode_plane_slab has waited for this one's bytes)
    }
    if (cr && cr->cached_pieces()) {                                                        // hits and fresh tiles alike out of the arenas: one launch per cache
        if (L.subs() == 0) s->timer.reset(s->stream);
        const GatherPiece *at = d_cached;
        s->timer.mark("k_wsi_gather_cached");
        for (const CachePlan::Use &us : cr->uses) {
            if (us.pieces.empty()) continue;
            cr->launched = true;
            launch_gather(s->stream, cr->kind, (const uint16_t *)us.c->arena, at, us.pieces.size(), us.mw, us.mh, d_out, o.dtype,
                          o.params(out_table(s, L, behind), (size_t)ph * (size_t)pw));
            at += us.pieces.size();
        }
        s->timer.mark("end");
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (cr) cr->finish(tile_status);
    return MIC_OK;
}

// The source of the file and reader doors: blobs[u] (host) is the blob of unit u.  A sub-batch's blobs are checked on the host, each
// under its own header, and their planes' bytes go up in one copy (s->io_comp), as decode_blobs does it.
PatchSlabs blob_slabs(mic_hip_session *s, const std::vector<const Mic3 *> &um, const std::vector<TileBlob> &blobs) {
    return [s, &um, &blobs](size_t u0, size_t nt, const uint8_t **base, std::vector<WsiPlane> &pl, int32_t *tile_status) -> int {
        std::vector<uint8_t> &bytes = s->wsi_host_bytes;                                    // (the session's: no fresh pages per call)
        bytes.clear();
        for (size_t k = 0; k < nt; k++) {
            const size_t b0 = bytes.size(), P = (size_t)um[u0 + k]->planes();
            if ((tile_status[k] = parse_tile_blob(*um[u0 + k], blobs[u0 + k].p, blobs[u0 + k].len, pl, bytes)) != MIC_OK) {
                bytes.resize(b0);
                pl.resize(k * P);
                pl.resize((k + 1) * P, WsiPlane{ 0, 0, 0, 0 });
            }
        }
        const int rc = s->io_comp.reserve(bytes.size() + 64);
        if (rc) return rc;
        if (!bytes.empty()) HIP_TRY(hipMemcpyAsync(s->io_comp.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, s->stream));
        *base = (const uint8_t *)s->io_comp.p;
        return MIC_OK;
    };
}

// ---- patches of one level: what the three one-slide doors share ----------------------------------------------------------------------
// The plan of one level of `m` through the core.  status[i] (may be NULL): MIC_OK, or the first failing tile of patch i in tile
// order, with the code mic_hip_wsi_decompress_tile has for it (the blob's, else its first failing plane's).
int level_patches(mic_hip_session *s, const PatchPlan &plan, const std::vector<const Mic3 *> &um, int n, int pw, int ph, const OutFormat &o, const SlabCeiling &ceiling,
                  const PatchSlabs &source, void *d_out, size_t need, int32_t *status, mic_hip_patch_stats *stats,
                  CachePlan *cr = nullptr, const PatchPlan *full = nullptr) {
    std::vector<int32_t> tst;
    uint64_t nslab = 0;
    const int rc = read_patches(s, plan, um, pw, ph, o, ceiling, source, d_out, need, tst, &nslab, cr);
    if (rc) return rc;
    if (cr) {                                                                               // plan: what was left to decode of *full; a hit is MIC_OK
        std::vector<int32_t> all(full->units.size(), MIC_OK);
        for (size_t d = 0; d < tst.size(); d++) all[cr->full_of[d]] = tst[d];
        fold_unit_status(full->pieces, all, n, 1, status, nullptr, [](uint32_t) { return -1; });
        if (stats) { stats->tiles_decoded = plan.units.size(); stats->pieces = full->pieces.size(); stats->slabs = nslab; }
        return MIC_OK;
    }
    fold_unit_status(plan.pieces, tst, n, 1, status, nullptr, [](uint32_t) { return -1; });
    if (stats) { stats->tiles_decoded = plan.units.size(); stats->pieces = plan.pieces.size(); stats->slabs = nslab; }
    return MIC_OK;
}

// mic_hip_wsi_read_patches / mic_hip_wsi_reader_read_patches on a parsed header, on the session the thread holds: the blobs of
// the union's tiles from `src` in ONE request (a reader then pulls those blobs only, contiguous ones in one read); a tile whose
// index entry points outside the file fails the call with the source's code before anything is launched.
int wsi_patches(const BlobSource &src, const Mic3 &m, int level, const int32_t *xy, int n, int pw, int ph, const OutFormat &o, void *d_out, size_t need,
                int32_t *status, mic_hip_patch_stats *stats, CacheOwner co = CacheOwner{ nullptr, 0, 0 }) {
    mic_hip_session *s = cur_default();
    const Level &L = m.lv[(size_t)level];
    int rc;
    if ((rc = patch_pointer(s, &d_out, need))) return rc;
    if (!out_aligned(o, d_out)) return MIC_ERR_ARGS;
    PatchPlan plan;
    if ((rc = plan_patches(L.w, L.h, m.tw, m.th, xy, n, pw, ph, plan))) return rc;
    if (co.c) {                                                                             // the reader has a tile cache: only what is not resident is fetched and decoded
        co.first = (uint64_t)L.first;
        CachePlan cp;
        if ((rc = cp.split(s, plan, std::vector<const Mic3 *>(plan.units.size(), &m), pw, ph, o, [&](size_t) { return co; }))) return rc;
        std::vector<size_t> tiles(cp.decode.units.size());
        for (size_t u = 0; u < tiles.size(); u++) tiles[u] = (size_t)L.first + (size_t)cp.decode.units[u].tile;
        std::vector<TileBlob> blobs; std::vector<uint8_t> keep;
        if (!tiles.empty() && (rc = src(tiles, blobs, keep))) return rc;
        const std::vector<const Mic3 *> um(tiles.size(), &m);
        return level_patches(s, cp.decode, um, n, pw, ph, o, blob_ceiling((size_t)m.planes()), blob_slabs(s, um, blobs), d_out, need, status, stats, &cp, &plan);
    }
    std::vector<size_t> tiles(plan.units.size());
    for (size_t u = 0; u < tiles.size(); u++) tiles[u] = (size_t)L.first + (size_t)plan.units[u].tile;
    std::vector<TileBlob> blobs; std::vector<uint8_t> keep;
    if (!tiles.empty() && (rc = src(tiles, blobs, keep))) return rc;
    const std::vector<const Mic3 *> um(tiles.size(), &m);
    return level_patches(s, plan, um, n, pw, ph, o, blob_ceiling((size_t)m.planes()), blob_slabs(s, um, blobs), d_out, need, status, stats);
}

// ---- patches of many slides and levels ------------------------------------------------------------------------------------------
// A slide of the call: where its header, level table and tile index are read (host; a file in memory starts there) and what they
// said.  m: a header parsed before (a reader's), else `own` is parsed from head.
struct MultiSlide {
    const uint8_t *head = nullptr; uint64_t file_len = 0;
    const Mic3 *m = nullptr; Mic3 own;
    bool named = false;                     // some patch names it: only then is it looked at
    bool header_ok = false;                 // its header was accepted, the call's sample format included
    int32_t status = MIC_OK;
    const Mic3 &hdr() const { return m ? *m : own; }
};
struct MultiPlan : PatchPlan { std::vector<MultiSlide> slides; };                          // units[u].tile: global index, level.first + ty * tiles_x + tx

// the tile-index entry of global tile gi: false when it points outside the file (as flat_source and the reader's fetch judge it)
bool multi_tile_entry(const MultiSlide &sl, uint64_t gi, uint64_t *off, uint64_t *len) {
    const Mic3 &m = sl.hdr();
    if (gi >= m.total) return false;
    const uint8_t *e = sl.head + 48 + 20 * (size_t)m.nlev + 16 * (size_t)gi;
    const uint64_t bo = get_u64(e), bl = get_u64(e + 8);
    if (bo > sl.file_len || bl > sl.file_len || m.data_off + bo + bl > sl.file_len) return false;
    *off = m.data_off + bo; *len = bl;
    return true;
}

// The plan of n patches of pw x ph over the slides (head, file_len, m set by the caller), patch i = q[4i .. 4i + 3] = (x, y, slide,
// level), for a call whose sample format is channels / bps.  MIC_ERR_ARGS for a slide index outside the list; a slide that is refused
// keeps its code in slides[f].status and its patches have no pieces; nor has a patch whose level its slide does not have.
int multi_plan(MultiPlan &plan, const int32_t *q, int n, int pw, int ph, int channels, int bps) {
    const int ns = (int)plan.slides.size();
    plan.units.clear(); plan.pieces.clear();
    for (int i = 0; i < n; i++) {
        const int32_t f = q[4 * (size_t)i + 2];
        if (f < 0 || f >= ns) return MIC_ERR_ARGS;
        plan.slides[(size_t)f].named = true;
    }
    for (MultiSlide &sl : plan.slides) {
        if (!sl.named) continue;
        if (!sl.head) { sl.status = MIC_ERR_ARGS; continue; }
        if (!sl.m && (sl.status = parse_mic3(sl.head, (size_t)sl.file_len, sl.own)) != MIC_OK) continue;
        const Mic3 &m = sl.hdr();
        if (!m.supported()) sl.status = MIC_ERR_UNSUPPORTED;
        else if (m.channels != channels || m.bps != bps) sl.status = MIC_ERR_ARGS;
        sl.header_ok = sl.status == MIC_OK;
    }
    std::vector<PlanKey> all;
    for (int i = 0; i < n; i++) {
        const uint32_t f = (uint32_t)q[4 * (size_t)i + 2];
        const MultiSlide &sl = plan.slides[f];
        if (sl.status != MIC_OK) continue;
        const Mic3 &m = sl.hdr();
        const int32_t level = q[4 * (size_t)i + 3];
        if (level < 0 || level >= (int)m.lv.size()) continue;
        const Level &L = m.lv[(size_t)level];
        plan_clip(all, f, L.w, L.h, m.tw, m.th, L.tx, L.first, i, q[4 * (size_t)i], q[4 * (size_t)i + 1], pw, ph);
    }
    const int rc = plan_sort(all);
    if (rc) return rc;
    // a touched tile whose index entry points outside the file fails its slide
    uint64_t off, len;
    for (size_t k = 0; k < all.size(); k++)
        if ((k == 0 || all[k].u.slide != all[k - 1].u.slide || all[k].u.tile != all[k - 1].u.tile) && plan.slides[all[k].u.slide].status == MIC_OK &&
            !multi_tile_entry(plan.slides[all[k].u.slide], all[k].u.tile, &off, &len)) plan.slides[all[k].u.slide].status = MIC_ERR_CORRUPT;
    plan_group(all, plan, [&](uint32_t f) { return plan.slides[f].status == MIC_OK; });
    return MIC_OK;
}

// what the entry points check before a file is looked at; o = the output description of a call on nsources slides, *need = bytes of
// the patch tensor
int multi_args(const int32_t *xysl, int n, int pw, int ph, int channels, int bps, const mic_hip_out_spec *spec, int nsources, OutFormat &o,
               size_t out_cap, size_t *need, Scale *sc = nullptr) {
    if (pw <= 0 || ph <= 0 || n < 0 || (n > 0 && !xysl)) return MIC_ERR_ARGS;
    if (sc) { const int src = sc->judge(pw, ph); if (src) return src; }
    if (!((channels == 3 && bps == 8) || (channels == 1 && (bps == 8 || bps == 16)))) return MIC_ERR_UNSUPPORTED;   // (Mic3::supported)
    const int rc = o.make(spec, channels, bps, nsources);
    if (rc) return rc;
    return tensor_bytes(n, 1, ph, pw, o.pixel(), out_cap, need);
}

// slide `f`'s blobs of `tiles` (global indices, entries checked by the plan) through its reader; NULL: the slides are files in memory
typedef std::function<int(uint32_t f, const std::vector<size_t> &tiles, std::vector<TileBlob> &blobs, std::vector<uint8_t> &keep)> MultiFetch;

// a door's call on a plan whose slides are set: arguments judged (multi_args), then the plan, n == 0, the pointer, the blobs, the core
int multi_call(MultiPlan &plan, const MultiFetch &fetch, const int32_t *xysl, int n, int pw, int ph, int channels, int bps, const OutFormat &o,
               void *d_out, size_t need, int32_t *status, mic_hip_multi_patch_stats *stats,
               const std::function<CacheOwner(uint32_t f)> &cache_of = nullptr) {
    int rc = multi_plan(plan, xysl, n, pw, ph, channels, bps);
    if (rc) return rc;
    if (stats) *stats = mic_hip_multi_patch_stats{ 0, 0, 0, 0 };
    if (n == 0) return MIC_OK;
    if (!d_out) return MIC_ERR_ARGS;
    DefaultLease lease;
    if ((rc = lease.acquire())) return rc;
    mic_hip_session *s = cur_default();
    if ((rc = patch_pointer(s, &d_out, need))) return rc;                                   // judged before anything is launched
    if (o.typed() ? !out_aligned(o, d_out) : (bps == 16 && ((size_t)d_out & 1))) return MIC_ERR_ARGS;
    // readers with tile caches: what is resident is neither fetched nor decoded (dp: the units that are left)
    std::unique_ptr<CachePlan> cp;
    if (cache_of) {
        bool any = false;
        for (const PatchUnit &pu : plan.units) any = any || cache_of(pu.slide).c != nullptr;
        if (any) {
            std::vector<const Mic3 *> um_all(plan.units.size());
            for (size_t u = 0; u < um_all.size(); u++) um_all[u] = &plan.slides[plan.units[u].slide].hdr();
            cp.reset(new CachePlan());
            if ((rc = cp->split(s, plan, um_all, pw, ph, o, [&](size_t u) { return cache_of(plan.units[u].slide); }))) return rc;
        }
    }
    const PatchPlan &dp = cp ? cp->decode : (const PatchPlan &)plan;
    const size_t nu = dp.units.size();
    std::vector<TileBlob> blobs; blobs.reserve(nu);
    std::vector<const Mic3 *> um(nu);
    std::vector<std::vector<uint8_t>> keep;
    std::vector<size_t> tiles;
    for (size_t u = 0; u < nu;) {                                                           // each slide's blobs in one request
        const uint32_t f = dp.units[u].slide;
        size_t v = u;
        tiles.clear();
        for (; v < nu && dp.units[v].slide == f; v++) { tiles.push_back((size_t)dp.units[v].tile); um[v] = &plan.slides[f].hdr(); }
        if (fetch) {
            std::vector<TileBlob> got;
            keep.emplace_back();
            if ((rc = fetch(f, tiles, got, keep.back()))) return rc;
            if (got.size() != tiles.size()) return MIC_ERR_INTERNAL;
            blobs.insert(blobs.end(), got.begin(), got.end());
        } else {
            uint64_t off = 0, len = 0;
            for (size_t gi : tiles) {
                if (!multi_tile_entry(plan.slides[f], gi, &off, &len)) return MIC_ERR_INTERNAL;   // (the plan has checked it)
                blobs.push_back(TileBlob{ plan.slides[f].head + off, (size_t)len });
            }
        }
        u = v;
    }
    std::vector<int32_t> tst;
    uint64_t nslab = 0;
    if ((rc = read_patches(s, dp, um, pw, ph, o, blob_ceiling(channels == 3 ? 3 : 1), blob_slabs(s, um, blobs), d_out, need, tst, &nslab, cp.get()))) return rc;
    if (cp) {                                                                               // (a hit is MIC_OK)
        std::vector<int32_t> all(plan.units.size(), MIC_OK);
        for (size_t d = 0; d < tst.size(); d++) all[cp->full_of[d]] = tst[d];
        tst.swap(all);
    }
    fold_unit_status(plan.pieces, tst, n, 1, status, nullptr, [](uint32_t) { return -1; });
    container_codes(n, status, [&](int i) {                                                 // a refused slide's code; a level the slide does not have
        const MultiSlide &sl = plan.slides[(size_t)xysl[4 * (size_t)i + 2]]; const int32_t level = xysl[4 * (size_t)i + 3];
        return sl.status != MIC_OK ? sl.status : (level < 0 || level >= (int)sl.hdr().lv.size()) ? (int32_t)MIC_ERR_ARGS : (int32_t)MIC_OK;
    });
    if (stats) {
        uint64_t read = 0;
        for (const MultiSlide &sl : plan.slides) read += sl.header_ok ? 1 : 0;
        *stats = mic_hip_multi_patch_stats{ nu, plan.pieces.size(), nslab, read };
    }
    return MIC_OK;
}

// ---- scaled patches: groups of source rectangles through the native core, then the resample -----------------------------------------
// A call of a _scaled door whose scale is not 1 / 1, on a session the caller holds, d_out and its alignment judged.  An output
// pixel's footprint straddles tiles that may sit in different sub-batches or in cache slots, so the gather cannot average in one pass
// and stay exact; as with the MIC2 temporal crops there is a staging tensor instead: the door's own native call (`group`: plan,
// sub-batches, cache split, gather -- unchanged) reads the n rectangles of sw x sh into s->wsi_stage, and one launch of
// k_resample_patches writes every sample of d_out.  The staging tensor may take a quarter of the workspace ceiling; n patches that
// need more go as consecutive groups, each one native call and one resample launch.
// group(i0, ng, d_stage, bytes, status, t, recs): patches [i0, i0 + ng) into d_stage, their statuses, the native call's stats, and
// their records (what of each source rectangle lies inside its level; empty where the native door zeroes the patch).
// whole(t): the plan counts of the whole call at sw x sh (host only), asked when the call was cut: pieces and slides are the plan's;
// so are the tiles unless a tile cache is in play (cached), where they stay what the groups really decoded.
struct ScaledTotals { uint64_t tiles = 0, pieces = 0, slabs = 0, slides = 0; };
typedef std::function<int(int i0, int ng, void *d_stage, size_t bytes, int32_t *status, ScaledTotals &t, ScaledPatch *recs)> ScaledGroup;
typedef std::function<int(ScaledTotals &t)> ScaledWhole;

int scaled_patches(mic_hip_session *s, const Scale &sc, int channels, int bps, int n, int pw, int ph, const OutFormat &o, void *d_out,
                   int32_t *status, bool cached, const ScaledGroup &group, const ScaledWhole &whole, ScaledTotals &tot) {
    const size_t spx = (size_t)channels * (bps == 16 ? 2 : 1);                              // bytes of a native pixel
    const unsigned __int128 pb128 = (unsigned __int128)(unsigned)sc.sw * (unsigned)sc.sh * spx;
    if (pb128 > ((size_t)1 << 40)) return MIC_ERR_CAPACITY;                                  // (one source rectangle that no device holds)
    const size_t pb = (size_t)pb128;
    const size_t gmax = std::min<size_t>((size_t)n, std::max<size_t>(1, workspace_budget() / 4 / pb));
    const size_t stage_bytes = align_up(gmax * pb, 16), rec_bytes = align_up(gmax * sizeof(ScaledPatch), 16);
    int rc;
    if ((rc = s->ensure(1, 1))) return rc;                                                  // (the session's stream)
    if ((rc = s->wsi_stage.reserve(stage_bytes + rec_bytes + o.table_bytes() + 64))) return rc;
    char *base = (char *)s->wsi_stage.p;
    ScaledPatch *d_recs = (ScaledPatch *)(base + stage_bytes);
    void *d_table = base + stage_bytes + rec_bytes;
    if (o.typed()) HIP_TRY(hipMemcpyAsync(d_table, o.table.data(), o.table_bytes(), hipMemcpyHostToDevice, s->stream));
    std::vector<ScaledPatch> recs((size_t)n);                                               // (lives until the synchronise below)
    const ScaledGeom g{ pw, ph, sc.sw, sc.sh, sc.num, sc.den, o.pad_bits() };
    tot = ScaledTotals();
    size_t groups = 0;
    for (size_t i0 = 0; i0 < (size_t)n; i0 += gmax, groups++) {
        const size_t ng = std::min(gmax, (size_t)n - i0);
        ScaledTotals t;
        s->timer.reset(s->stream);                                                          // (a native call that launches nothing marks nothing)
        if ((rc = group((int)i0, (int)ng, base, ng * pb, status ? status + i0 : nullptr, t, recs.data() + i0))) return rc;
        tot.tiles += t.tiles; tot.pieces += t.pieces; tot.slabs += t.slabs; tot.slides = std::max(tot.slides, t.slides);
        HIP_TRY(hipMemcpyAsync(d_recs, recs.data() + i0, ng * sizeof(ScaledPatch), hipMemcpyHostToDevice, s->stream));
        s->timer.mark("k_wsi_resample");                                                    // behind the marks of the native call's last sub-batch
        launch_resample(s->stream, channels, bps, o, d_table, base, d_recs, ng, g, (char *)d_out + i0 * (size_t)ph * (size_t)pw * o.pixel());
        s->timer.mark("end");
        HIP_TRY(hipGetLastError());                                                         // (the next group's native call follows on the stream)
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (groups > 1) {
        ScaledTotals w;
        if ((rc = whole(w))) return rc;
        tot.pieces = w.pieces; tot.slides = w.slides;
        if (!cached) tot.tiles = w.tiles;
    }
    return MIC_OK;
}
// a patch's record: what of its source rectangle at (x, y) lies inside a level of lw x lh
ScaledPatch scaled_record(const Scale &sc, int64_t x, int64_t y, int64_t lw, int64_t lh, int32_t source) {
    const int64_t x0 = std::max<int64_t>(0, -x), x1 = std::min<int64_t>(sc.sw, lw - x), y0 = std::max<int64_t>(0, -y), y1 = std::min<int64_t>(sc.sh, lh - y);
    if (x0 >= x1 || y0 >= y1) return ScaledPatch{ 0, 0, 0, 0, source, 0 };
    return ScaledPatch{ (int32_t)x0, (int32_t)x1, (int32_t)y0, (int32_t)y1, source, 0 };
}

// The one-slide doors' scaled call on a parsed header: `native` is the door's own core call (wsi_patches on its source, or the
// session store's) for rectangles of sw x sh in the slide's format.
typedef std::function<int(const int32_t *xy, int n, void *d_out, size_t need, int32_t *status, mic_hip_patch_stats *stats)> NativePatches;
int scaled_level(mic_hip_session *s, const Mic3 &m, int level, const int32_t *xy, int n, int pw, int ph, const Scale &sc, const OutFormat &o, void *d_out,
                 int32_t *status, mic_hip_patch_stats *stats, bool cached, const NativePatches &native) {
    const Level &L = m.lv[(size_t)level];
    ScaledTotals tot;
    const int rc = scaled_patches(s, sc, m.channels, m.bps, n, pw, ph, o, d_out, status, cached,
        [&](int i0, int ng, void *d_stage, size_t bytes, int32_t *st, ScaledTotals &t, ScaledPatch *recs) -> int {
            mic_hip_patch_stats ps{ 0, 0, 0 };
            const int r = native(xy + 2 * (size_t)i0, ng, d_stage, bytes, st, &ps);
            if (r) return r;
            t.tiles = ps.tiles_decoded; t.pieces = ps.pieces; t.slabs = ps.slabs;
            for (int i = 0; i < ng; i++) recs[i] = scaled_record(sc, xy[2 * ((size_t)i0 + i)], xy[2 * ((size_t)i0 + i) + 1], L.w, L.h, 0);
            return MIC_OK;
        },
        [&](ScaledTotals &t) -> int {
            PatchPlan plan;
            const int r = plan_patches(L.w, L.h, m.tw, m.th, xy, n, sc.sw, sc.sh, plan);
            t.tiles = plan.units.size(); t.pieces = plan.pieces.size();
            return r;
        }, tot);
    if (rc) return rc;
    if (stats) *stats = mic_hip_patch_stats{ tot.tiles, tot.pieces, tot.slabs };
    return MIC_OK;
}

// The multi doors' scaled call, behind multi_args: what multi_call judges, in its order -- the slide indices, n == 0, the pointer --,
// then multi_call itself group by group on a fresh plan each (slides(plan) sets the plan's slides as the door does).
int multi_call_scaled(const std::function<void(MultiPlan &)> &slides, int nslides, const MultiFetch &fetch, const int32_t *xysl, int n, int pw, int ph,
                      int channels, int bps, const Scale &sc, const OutFormat &o, void *d_out, size_t need, int32_t *status, mic_hip_multi_patch_stats *stats,
                      const std::function<CacheOwner(uint32_t f)> &cache_of, bool cached) {
    for (int i = 0; i < n; i++) if (xysl[4 * (size_t)i + 2] < 0 || xysl[4 * (size_t)i + 2] >= nslides) return MIC_ERR_ARGS;
    if (stats) *stats = mic_hip_multi_patch_stats{ 0, 0, 0, 0 };
    if (n == 0) return MIC_OK;
    if (!d_out) return MIC_ERR_ARGS;
    DefaultLease lease;
    int rc;
    if ((rc = lease.acquire())) return rc;
    mic_hip_session *s = cur_default();
    if ((rc = patch_pointer(s, &d_out, need))) return rc;
    if (o.typed() ? !out_aligned(o, d_out) : (bps == 16 && ((size_t)d_out & 1))) return MIC_ERR_ARGS;
    OutFormat on;
    if ((rc = on.make(nullptr, channels, bps, 1))) return rc;
    auto heads = [](const MultiPlan &plan) { uint64_t k = 0; for (const MultiSlide &sl : plan.slides) k += sl.header_ok ? 1 : 0; return k; };
    ScaledTotals tot;
    rc = scaled_patches(s, sc, channels, bps, n, pw, ph, o, d_out, status, cached,
        [&](int i0, int ng, void *d_stage, size_t bytes, int32_t *st, ScaledTotals &t, ScaledPatch *recs) -> int {
            MultiPlan plan;
            slides(plan);
            mic_hip_multi_patch_stats ms{ 0, 0, 0, 0 };
            const int32_t *q = xysl + 4 * (size_t)i0;
            const int r = multi_call(plan, fetch, q, ng, sc.sw, sc.sh, channels, bps, on, d_stage, bytes, st, &ms, cache_of);
            if (r) return r;
            t.tiles = ms.tiles_decoded; t.pieces = ms.pieces; t.slabs = ms.slabs; t.slides = ms.slides_read;
            for (int i = 0; i < ng; i++) {                                                  // a refused slide, a level it does not have: all pad
                const int32_t f = q[4 * (size_t)i + 2], level = q[4 * (size_t)i + 3];
                const MultiSlide &sl = plan.slides[(size_t)f];
                if (sl.status != MIC_OK || level < 0 || level >= (int)sl.hdr().lv.size()) { recs[i] = ScaledPatch{ 0, 0, 0, 0, f, 0 }; continue; }
                const Level &L = sl.hdr().lv[(size_t)level];
                recs[i] = scaled_record(sc, q[4 * (size_t)i], q[4 * (size_t)i + 1], L.w, L.h, f);
            }
            return MIC_OK;
        },
        [&](ScaledTotals &t) -> int {
            MultiPlan plan;
            slides(plan);
            const int r = multi_plan(plan, xysl, n, sc.sw, sc.sh, channels, bps);
            t.tiles = plan.units.size(); t.pieces = plan.pieces.size(); t.slides = heads(plan);
            return r;
        }, tot);
    if (rc) return rc;
    if (stats) *stats = mic_hip_multi_patch_stats{ tot.tiles, tot.pieces, tot.slabs, tot.slides };
    return MIC_OK;
}
}  // namespace

extern "C" {

// parallel.wsi_band_plan behind the band path of mic_hip_wsi_compress_ex (band_plan); no device needed
int mic_hip_wsi_band_plan(int width, int height, int tile_w, int tile_h, int levels, int shards, int *k_out, int *row_first) try {
    if (!k_out || !row_first || width <= 0 || height <= 0 || tile_w < 0 || tile_h < 0 || levels > 32 || shards <= 0) return MIC_ERR_ARGS;
    if (tile_w == 0) tile_w = 256;
    if (tile_h == 0) tile_h = 256;
    *k_out = band_plan(height, tile_h, (int)plan_levels(width, height, tile_w, tile_h, levels).size(), shards, row_first);
    return MIC_OK;
} MIC_ABI_CATCH

// CompressWSI (wsicompress.go:27-171): 8-bit RGB (channels 3) or 8/16-bit greyscale (channels 1, little-endian samples).
// Bands of tile rows over the devices of mic_hip_set_devices when that gives two or more (and the call is not nested), else one band.
int mic_hip_wsi_compress_ex(const uint8_t *rgb, int width, int height, int channels, int bits_per_sample, int tile_w, int tile_h,
                            int levels, uint8_t *out, size_t out_cap, size_t *out_len) try {
    if (!rgb || !out || !out_len || width <= 0 || height <= 0 || tile_w < 0 || tile_h < 0) return MIC_ERR_ARGS;
    Mic3 fmt;
    int rc = wsi_options(width, height, channels, bits_per_sample, tile_w, tile_h, levels, fmt);
    if (rc) return rc;
    const std::vector<Level> lv = plan_levels(width, height, fmt.tw, fmt.th, levels);
    if (!cur_default()) {                                                                   // several devices: bands of tile rows
        const std::vector<int> devs = default_devices();
        if (devs.size() > 1) {
            std::vector<int> row_first(devs.size() + 1);
            const int K = band_plan(height, fmt.th, (int)lv.size(), (int)devs.size(), row_first.data());
            int bands = 0;
            for (size_t b = 0; b < devs.size(); b++) bands += row_first[b + 1] > row_first[b];
            if (bands >= 2) return wsi_compress_bands(rgb, fmt, lv, K, row_first, out, out_cap, out_len);
        }
    }
    std::vector<int> row_first(2);                                                          // the default device, or the session held
    const int K = band_plan(height, fmt.th, (int)lv.size(), 1, row_first.data());
    return wsi_compress_bands(rgb, fmt, lv, K, row_first, out, out_cap, out_len);
} MIC_ABI_CATCH

// CompressRGB (rgbcompress.go:25-27) = compressRGBTileBlob on the whole image: one "tile" of width x height
int mic_hip_rgb_compress(const uint8_t *rgb, int width, int height, uint8_t *out, size_t out_cap, size_t *out_len) try {
    if (!rgb || !out || !out_len || width <= 0 || height <= 0) return MIC_ERR_ARGS;
    if ((size_t)width * height > ((size_t)1 << 26)) return MIC_ERR_UNSUPPORTED;
    Mic3 fmt; fmt.channels = 3; fmt.bps = 8; fmt.flags = 0x03; fmt.tw = width; fmt.th = height;
    DefaultLease lease;
    int rc = lease.acquire();
    if (rc) return rc;
    mic_hip_session *s = cur_default();
    if ((rc = s->ensure(1, (size_t)width * height))) return rc;
    struct Bufs : SlabBufs { DevBuf img; ~Bufs() { img.release(); } } bufs;                // freed on every return path
    if ((rc = bufs.img.reserve((size_t)width * height * 3 + 64))) return rc;
    HIP_TRY(hipMemcpyAsync(bufs.img.p, rgb, (size_t)width * height * 3, hipMemcpyHostToDevice, s->stream));
    TileRun blob;
    if ((rc = code_level(s, fmt, bufs.img.p, Level{ width, height, 1, 1, 0 }, bufs, slab_tiles(fmt, (size_t)8 << 30), blob))) return rc;
    if (blob.bytes.size() > out_cap) return MIC_ERR_CAPACITY;
    memcpy(out, blob.bytes.data(), blob.bytes.size());
    *out_len = blob.bytes.size();
    return MIC_OK;
} MIC_ABI_CATCH

// DecompressRGB (rgbcompress.go:31-33)
int mic_hip_rgb_decompress(const uint8_t *c, size_t len, int width, int height, uint8_t *rgb_out, size_t out_cap) try {
    if (!c || !rgb_out || width <= 0 || height <= 0) return MIC_ERR_ARGS;
    if ((size_t)width * height > ((size_t)1 << 26)) return MIC_ERR_UNSUPPORTED;
    if ((size_t)width * height * 3 > out_cap) return MIC_ERR_CAPACITY;
    Mic3 m; m.w = width; m.h = height; m.tw = width; m.th = height; m.channels = 3; m.bps = 8; m.flags = 0x03; m.nlev = 1; m.total = 1; m.data_off = 0;
    DefaultLease lease;
    int rc = lease.acquire();
    if (rc) return rc;
    return decode_blobs(m, std::vector<TileBlob>(1, TileBlob{ c, len }), std::vector<int4>(1, make_int4(0, 0, width, height)), rgb_out, width, height);
} MIC_ABI_CATCH

// MICR file = "MICR", width, height (u32 LE), CompressRGB blob (writeMICRFile, cmd/mic-compress/main.go:62-91)
int mic_hip_micr_compress(const uint8_t *rgb, int width, int height, uint8_t *out, size_t out_cap, size_t *out_len) try {
    if (!out || !out_len) return MIC_ERR_ARGS;
    if (out_cap < 12) return MIC_ERR_CAPACITY;
    size_t n = 0;
    const int rc = mic_hip_rgb_compress(rgb, width, height, out + 12, out_cap - 12, &n);
    if (rc) return rc;
    memcpy(out, "MICR", 4); put_u32(out + 4, (uint32_t)width); put_u32(out + 8, (uint32_t)height);
    *out_len = 12 + n;
    return MIC_OK;
} MIC_ABI_CATCH
int mic_hip_micr_info(const uint8_t *c, size_t len, int *width, int *height) try {
    if (!c) return MIC_ERR_ARGS;
    if (len < 12 || memcmp(c, "MICR", 4) != 0) return MIC_ERR_CORRUPT;
    const uint32_t w = get_u32(c + 4), h = get_u32(c + 8);
    if (w == 0 || h == 0 || w > (1u << 26) || h > (1u << 26)) return MIC_ERR_CORRUPT;
    if (width) *width = (int)w; if (height) *height = (int)h;
    return MIC_OK;
} MIC_ABI_CATCH
int mic_hip_micr_decompress(const uint8_t *c, size_t len, uint8_t *rgb_out, size_t out_cap) try {
    int w = 0, h = 0;
    const int rc = mic_hip_micr_info(c, len, &w, &h);
    if (rc) return rc;
    return mic_hip_rgb_decompress(c + 12, len - 12, w, h, rgb_out, out_cap);
} MIC_ABI_CATCH

// MIC1 file = "MIC1", width, height, pipeline 1, payload length (u32 LE each), CompressSingleFrame stream
// (writeMicFile, cmd/mic-compress/main.go:26-59; the stream's own magic tells the state count)
int mic_hip_mic1_compress(const uint16_t *pixels, int width, int height, uint16_t max_value, int n_states,
                          uint8_t *out, size_t out_cap, size_t *out_len) try {
    if (!out || !out_len) return MIC_ERR_ARGS;
    if (out_cap < 20) return MIC_ERR_CAPACITY;
    size_t n = 0;
    const int rc = mic_hip_compress_frame(pixels, width, height, max_value, n_states, out + 20, out_cap - 20, &n);
    if (rc) return rc;
    if (n > 0xFFFFFFFFu) return MIC_ERR_UNSUPPORTED;
    memcpy(out, "MIC1", 4); put_u32(out + 4, (uint32_t)width); put_u32(out + 8, (uint32_t)height); put_u32(out + 12, 1); put_u32(out + 16, (uint32_t)n);
    *out_len = 20 + n;
    return MIC_OK;
} MIC_ABI_CATCH
int mic_hip_mic1_info(const uint8_t *c, size_t len, int *width, int *height) try {
    if (!c) return MIC_ERR_ARGS;
    if (len < 20 || memcmp(c, "MIC1", 4) != 0) return MIC_ERR_CORRUPT;
    const uint32_t w = get_u32(c + 4), h = get_u32(c + 8);
    if (w == 0 || h == 0 || w > (1u << 26) || h > (1u << 26) || get_u32(c + 12) != 1 || (size_t)get_u32(c + 16) > len - 20) return MIC_ERR_CORRUPT;
    if (width) *width = (int)w; if (height) *height = (int)h;
    return MIC_OK;
} MIC_ABI_CATCH
int mic_hip_mic1_decompress(const uint8_t *c, size_t len, uint16_t *pixels_out, size_t out_cap_px) try {
    int w = 0, h = 0;
    const int rc = mic_hip_mic1_info(c, len, &w, &h);
    if (rc) return rc;
    if ((size_t)w * h > out_cap_px) return MIC_ERR_CAPACITY;
    return mic_hip_decompress_frame(c + 20, get_u32(c + 16), pixels_out, w, h);
} MIC_ABI_CATCH

int mic_hip_wsi_compress(const uint8_t *rgb, int width, int height, int tile_w, int tile_h, int levels,
                         uint8_t *out, size_t out_cap, size_t *out_len) try {
    return mic_hip_wsi_compress_ex(rgb, width, height, 3, 8, tile_w, tile_h, levels, out, out_cap, out_len);
} MIC_ABI_CATCH

// WSIHeader.Channels / BitsPerSample / ColorTransform (wsiformat.go:169-227)
int mic_hip_wsi_format(const uint8_t *c, size_t len, int *channels, int *bits_per_sample, int *color_transform) try {
    if (!c) return MIC_ERR_ARGS;
    Mic3 m; int rc = parse_mic3(c, len, m);
    if (rc) return rc;
    if (channels) *channels = m.channels; if (bits_per_sample) *bits_per_sample = m.bps; if (color_transform) *color_transform = (m.flags & 0x02) ? 1 : 0;
    return MIC_OK;
} MIC_ABI_CATCH

// ReadWSIHeader (wsicompress.go:299-306)
int mic_hip_wsi_info(const uint8_t *c, size_t len, int *width, int *height, int *tile_w, int *tile_h, int *levels, uint64_t *total_tiles) try {
    if (!c) return MIC_ERR_ARGS;
    Mic3 m; int rc = parse_mic3(c, len, m);
    if (rc) return rc;
    if (width) *width = m.w; if (height) *height = m.h; if (tile_w) *tile_w = m.tw; if (tile_h) *tile_h = m.th;
    if (levels) *levels = m.nlev; if (total_tiles) *total_tiles = m.total;
    return MIC_OK;
} MIC_ABI_CATCH
int mic_hip_wsi_level_info(const uint8_t *c, size_t len, int level, int *width, int *height, int *tiles_x, int *tiles_y) try {
    if (!c) return MIC_ERR_ARGS;
    Mic3 m; int rc = parse_mic3(c, len, m);
    if (rc) return rc;
    if (level < 0 || level >= m.nlev) return MIC_ERR_ARGS;
    const Level &L = m.lv[(size_t)level];
    if (width) *width = L.w; if (height) *height = L.h; if (tiles_x) *tiles_x = L.tx; if (tiles_y) *tiles_y = L.ty;
    return MIC_OK;
} MIC_ABI_CATCH

// DecompressWSITile (wsicompress.go:175-217): one tile, cropped at the level's edge
int mic_hip_wsi_decompress_tile(const uint8_t *c, size_t len, int level, int tile_x, int tile_y,
                                uint8_t *rgb_out, size_t out_cap, int *out_w, int *out_h) try {
    if (!c || !rgb_out) return MIC_ERR_ARGS;
    Mic3 m; int rc = parse_mic3(c, len, m);
    if (rc) return rc;
    return wsi_tile(flat_source(c, len, m), m, level, tile_x, tile_y, rgb_out, out_cap, out_w, out_h);
} MIC_ABI_CATCH

// Whole pyramid level in one batch: every tile of the level, stitched (viewer / bench path)
int mic_hip_wsi_decompress_level(const uint8_t *c, size_t len, int level, uint8_t *rgb_out, size_t out_cap) try {
    if (!c || !rgb_out) return MIC_ERR_ARGS;
    Mic3 m; int rc = parse_mic3(c, len, m);
    if (rc) return rc;
    if (level < 0 || level >= m.nlev) return MIC_ERR_ARGS;
    const Level &L = m.lv[(size_t)level];
    if (!m.supported()) return MIC_ERR_UNSUPPORTED;
    if (L.w <= 0 || L.h <= 0 || (size_t)L.w * L.h * m.bpp() > out_cap) return (L.w <= 0 || L.h <= 0) ? MIC_ERR_CORRUPT : MIC_ERR_CAPACITY;
    if ((size_t)L.tx * m.tw < (size_t)L.w || (size_t)L.ty * m.th < (size_t)L.h) return MIC_ERR_CORRUPT;
    return decode_box(c, len, m, L, 0, L.tx - 1, 0, L.ty - 1, 0, L.w, L.h, rgb_out);
} MIC_ABI_CATCH

// DecompressWSIRegion (wsicompress.go:219-297): the tiles that overlap the rectangle are decoded in one batch into
// their tile-aligned bounding box, the rectangle is cut out of it.  w / h are clamped to the level like the reference does.
int mic_hip_wsi_decompress_region(const uint8_t *c, size_t len, int level, int x, int y, int w, int h,
                                  uint8_t *rgb_out, size_t out_cap, int *out_w, int *out_h) try {
    if (!c || !rgb_out) return MIC_ERR_ARGS;
    Mic3 m; int rc = parse_mic3(c, len, m);
    if (rc) return rc;
    return wsi_region(flat_source(c, len, m), m, level, x, y, w, h, rgb_out, out_cap, out_w, out_h);
} MIC_ABI_CATCH

// plan_patches behind the three read_patches calls: the tiles n patches touch (sorted, each once) and the number of pieces
int mic_hip_wsi_patch_plan(int level_w, int level_h, int tile_w, int tile_h, const int32_t *xy, int n, int pw, int ph,
                           uint64_t *tiles, size_t cap, uint64_t *ntiles, uint64_t *npieces) try {
    if (level_w <= 0 || level_h <= 0 || tile_w < 0 || tile_h < 0 || n < 0 || (n > 0 && !xy) || pw <= 0 || ph <= 0 || (cap > 0 && !tiles)) return MIC_ERR_ARGS;
    PatchPlan plan;
    const int rc = plan_patches(level_w, level_h, tile_w ? tile_w : 256, tile_h ? tile_h : 256, xy, n, pw, ph, plan);
    if (rc) return rc;
    if (ntiles) *ntiles = plan.units.size();
    if (npieces) *npieces = plan.pieces.size();
    if (plan.units.size() > cap) return MIC_ERR_CAPACITY;
    for (size_t u = 0; u < plan.units.size(); u++) tiles[u] = plan.units[u].tile;
    return MIC_OK;
} MIC_ABI_CATCH

// mic_hip_wsi_scaled_extent: Scale::judge; needs no device
int mic_hip_wsi_scaled_extent(int pw, int ph, int scale_num, int scale_den, int *sw, int *sh) try {
    Scale sc; sc.num = scale_num; sc.den = scale_den;
    const int rc = sc.judge(pw, ph);
    if (rc) return rc;
    if (sw) *sw = sc.sw;
    if (sh) *sh = sc.sh;
    return MIC_OK;
} MIC_ABI_CATCH

// The scaled call of the file and reader doors on the session the thread holds: d_out judged as wsi_patches judges it, then the
// door's own native call group by group (scaled_level).
static int wsi_patches_scaled(const BlobSource &src, const Mic3 &m, int level, const int32_t *xy, int n, int pw, int ph, const Scale &sc, const OutFormat &o,
                              void *d_out, size_t need, int32_t *status, mic_hip_patch_stats *stats, CacheOwner co = CacheOwner{ nullptr, 0, 0 }) {
    mic_hip_session *s = cur_default();
    int rc;
    if ((rc = patch_pointer(s, &d_out, need))) return rc;
    if (!out_aligned(o, d_out)) return MIC_ERR_ARGS;
    OutFormat on;
    if ((rc = on.make(nullptr, m.channels, m.bps, 1))) return rc;
    return scaled_level(s, m, level, xy, n, pw, ph, sc, o, d_out, status, stats, co.c != nullptr,
                        [&](const int32_t *q, int ng, void *d_stage, size_t bytes, int32_t *st, mic_hip_patch_stats *ps) {
                            return wsi_patches(src, m, level, q, ng, sc.sw, sc.sh, on, d_stage, bytes, st, ps, co);
                        });
}

// n patches of one level of a MIC3 file in host memory, into a tensor on the default session's device (sc: the _scaled door's scale)
static int wsi_read_patches_door(const uint8_t *c, size_t len, int level, const int32_t *xy, int n, int pw, int ph,
                                 void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec, Scale *sc) {
    if (!c) return MIC_ERR_ARGS;
    Mic3 m; int rc = parse_mic3(c, len, m);
    if (rc) return rc;
    size_t need = 0;
    OutFormat o;
    if ((rc = patch_args(m, level, xy, n, pw, ph, spec, o, out_cap, &need, sc))) return rc;
    if (stats) *stats = mic_hip_patch_stats{ 0, 0, 0 };
    if (n == 0) return MIC_OK;
    if (!d_out) return MIC_ERR_ARGS;
    DefaultLease lease;
    if ((rc = lease.acquire())) return rc;
    if (sc && !sc->unit()) return wsi_patches_scaled(flat_source(c, len, m), m, level, xy, n, pw, ph, *sc, o, d_out, need, status, stats);
    return wsi_patches(flat_source(c, len, m), m, level, xy, n, pw, ph, o, d_out, need, status, stats);
}
int mic_hip_wsi_read_patches_as(const uint8_t *c, size_t len, int level, const int32_t *xy, int n, int pw, int ph,
                                void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec) try {
    return wsi_read_patches_door(c, len, level, xy, n, pw, ph, d_out, out_cap, status, stats, spec, nullptr);
} MIC_ABI_CATCH
int mic_hip_wsi_read_patches_scaled(const uint8_t *c, size_t len, int level, const int32_t *xy, int n, int pw, int ph,
                                    void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec,
                                    int scale_num, int scale_den) try {
    Scale sc; sc.num = scale_num; sc.den = scale_den;
    return wsi_read_patches_door(c, len, level, xy, n, pw, ph, d_out, out_cap, status, stats, spec, &sc);
} MIC_ABI_CATCH
int mic_hip_wsi_read_patches(const uint8_t *c, size_t len, int level, const int32_t *xy, int n, int pw, int ph,
                             void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats) {
    return mic_hip_wsi_read_patches_as(c, len, level, xy, n, pw, ph, d_out, out_cap, status, stats, nullptr);
}

// multi_plan behind the two multi-slide calls: the (slide, tile) units n patches need decoded and the number of pieces
int mic_hip_wsi_multi_patch_plan(const uint8_t *const *files, const size_t *lens, int nfiles,
                                 const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                 uint32_t *slide_of, uint64_t *tile_of, size_t cap,
                                 uint64_t *ntiles_out, uint64_t *npieces, int32_t *file_status) try {
    if (nfiles < 0 || (nfiles > 0 && (!files || !lens)) || (cap > 0 && (!slide_of || !tile_of))) return MIC_ERR_ARGS;
    size_t need = 0;
    OutFormat o;
    int rc = multi_args(xysl, n, pw, ph, channels, bits_per_sample, nullptr, 1, o, SIZE_MAX, &need);
    if (rc) return rc;
    MultiPlan plan;
    plan.slides.resize((size_t)nfiles);
    for (int f = 0; f < nfiles; f++) { plan.slides[(size_t)f].head = files[f]; plan.slides[(size_t)f].file_len = lens[f]; }
    if ((rc = multi_plan(plan, xysl, n, pw, ph, channels, bits_per_sample))) return rc;
    if (file_status) for (int f = 0; f < nfiles; f++) file_status[f] = plan.slides[(size_t)f].status;
    if (ntiles_out) *ntiles_out = plan.units.size();
    if (npieces) *npieces = plan.pieces.size();
    if (plan.units.size() > cap) return MIC_ERR_CAPACITY;
    for (size_t u = 0; u < plan.units.size(); u++) { slide_of[u] = plan.units[u].slide; tile_of[u] = plan.units[u].tile; }
    return MIC_OK;
} MIC_ABI_CATCH

// n patches of many MIC3 files in host memory, any levels, into a tensor on the default session's device
static int wsi_multi_read_patches_door(const uint8_t *const *files, const size_t *lens, int nfiles,
                                       const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                       void *d_out, size_t out_cap, int32_t *status, mic_hip_multi_patch_stats *stats, const mic_hip_out_spec *spec, Scale *sc) {
    if (nfiles < 0 || (nfiles > 0 && (!files || !lens))) return MIC_ERR_ARGS;
    size_t need = 0;
    OutFormat o;
    const int rc = multi_args(xysl, n, pw, ph, channels, bits_per_sample, spec, nfiles, o, out_cap, &need, sc);
    if (rc) return rc;
    auto slides = [&](MultiPlan &plan) {
        plan.slides.resize((size_t)nfiles);
        for (int f = 0; f < nfiles; f++) { plan.slides[(size_t)f].head = files[f]; plan.slides[(size_t)f].file_len = lens[f]; }
    };
    if (sc && !sc->unit())
        return multi_call_scaled(slides, nfiles, nullptr, xysl, n, pw, ph, channels, bits_per_sample, *sc, o, d_out, need, status, stats, nullptr, false);
    MultiPlan plan;
    slides(plan);
    return multi_call(plan, nullptr, xysl, n, pw, ph, channels, bits_per_sample, o, d_out, need, status, stats);
}
int mic_hip_wsi_multi_read_patches_as(const uint8_t *const *files, const size_t *lens, int nfiles,
                                      const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                      void *d_out, size_t out_cap, int32_t *status, mic_hip_multi_patch_stats *stats, const mic_hip_out_spec *spec) try {
    return wsi_multi_read_patches_door(files, lens, nfiles, xysl, n, pw, ph, channels, bits_per_sample, d_out, out_cap, status, stats, spec, nullptr);
} MIC_ABI_CATCH
int mic_hip_wsi_multi_read_patches_scaled(const uint8_t *const *files, const size_t *lens, int nfiles,
                                          const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                          void *d_out, size_t out_cap, int32_t *status, mic_hip_multi_patch_stats *stats, const mic_hip_out_spec *spec,
                                          int scale_num, int scale_den) try {
    Scale sc; sc.num = scale_num; sc.den = scale_den;
    return wsi_multi_read_patches_door(files, lens, nfiles, xysl, n, pw, ph, channels, bits_per_sample, d_out, out_cap, status, stats, spec, &sc);
} MIC_ABI_CATCH
int mic_hip_wsi_multi_read_patches(const uint8_t *const *files, const size_t *lens, int nfiles,
                                   const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                   void *d_out, size_t out_cap, int32_t *status, mic_hip_multi_patch_stats *stats) {
    return mic_hip_wsi_multi_read_patches_as(files, lens, nfiles, xysl, n, pw, ph, channels, bits_per_sample, d_out, out_cap, status, stats, nullptr);
}

}  // extern "C"

// ==========================================================================================
// MIC3 on a device-resident slide (what bench.py times for BASELINE config 5).  mic_hip_session_wsi_encode runs the pyramid and the
// tile path of mic_hip_wsi_compress_ex (encode_level), but the coded planes never leave the device: they are appended to a store
// the session owns (device bytes + one host record per plane).  mic_hip_session_wsi_write turns the store into the MIC3 file
// (WriteMIC3, wsiformat.go:99-165: the only step that needs the bytes on the host); mic_hip_session_wsi_decode_level decodes every
// tile of a level from the store into a device image.
struct mic_hip_wsi_store {
    Mic3 fmt; std::vector<Level> lv; size_t total_tiles = 0;
    std::vector<WsiPlane> planes;                                                       // total_tiles * fmt.planes(), tile-major; off: into bytes
    DevBuf bytes; size_t used = 0;
    int append(hipStream_t st, const void *d_src, size_t n, uint64_t *off) {            // grows by copying (rare: starts at the raw size / 2)
        if (used + n > bytes.cap) {
            DevBuf nb;
            int rc = nb.reserve(std::max(bytes.cap * 2, used + n));
            if (rc) return rc;
            if (used && hipMemcpyAsync(nb.p, bytes.p, used, hipMemcpyDeviceToDevice, st) != hipSuccess) { nb.release(); return MIC_ERR_DEVICE; }
            if (hipStreamSynchronize(st) != hipSuccess) { nb.release(); return MIC_ERR_DEVICE; }
            bytes.release(); bytes = nb;
        }
        if (n && hipMemcpyAsync((char *)bytes.p + used, d_src, n, hipMemcpyDeviceToDevice, st) != hipSuccess) return MIC_ERR_DEVICE;
        *off = used; used += n;
        return MIC_OK;
    }
};

void mic_wsi_store_free(mic_hip_wsi_store *w) { if (w) { w->bytes.release(); delete w; } }

namespace {

// tiles per slab of the session's slide (encode and decode)
size_t session_slab_tiles(const Mic3 &fmt) { return slab_tiles(fmt, (size_t)16 << 30); }

// The store as the container's payload (compressTileBlob, wsicompress.go:334-364, for every tile in container order), built on the
// device in s->wsi_payload: WriteMIC3 then is one transfer of it behind the header and the tile index; a multi-GPU writer gathers
// it device to device.  tlen[t] = bytes of tile t (total_tiles entries), *total = their sum.
int wsi_assemble(mic_hip_session *s, uint64_t *tlen, uint64_t *total) {
    mic_hip_wsi_store &W = *s->wsi;
    return assemble_tiles(s, W.planes.data(), W.total_tiles, (size_t)W.fmt.planes(), (uint64_t)(uintptr_t)W.bytes.p, s->wsi_payload,
                          s->wsi_recs, tlen, total);
}

}  // namespace

extern "C" {

int mic_hip_session_wsi_encode(mic_hip_session *s, const uint8_t *d_pixels, int width, int height, int channels, int bits_per_sample,
                               int tile_w, int tile_h, int levels, uint64_t *total_tiles, uint64_t *compressed_bytes) try {
    if (!s || !d_pixels || width <= 0 || height <= 0 || tile_w < 0 || tile_h < 0) return MIC_ERR_ARGS;
    Mic3 fmt;
    int rc = wsi_options(width, height, channels, bits_per_sample, tile_w, tile_h, levels, fmt);
    if (rc) return rc;
    if ((rc = s->activate())) return rc;
    if ((rc = s->ensure(1, (size_t)fmt.tw * fmt.th))) return rc;
    if (!s->wsi) s->wsi = new mic_hip_wsi_store();
    if (s->tile_cache) {                                                                    // the store is replaced: its tiles in the cache are the old slide's
        mic_hip_tile_cache *c = s->tile_cache;
        if (c->tw != fmt.tw || c->th != fmt.th || c->channels != fmt.channels || c->bps != fmt.bps) { c->detach(s->tile_owner); s->tile_cache = nullptr; }
        else { std::lock_guard<std::mutex> lk(c->mu); c->index.drop_owner(s->tile_owner); s->tile_owner = tile_cache_new_owner(); }
    }
    mic_hip_wsi_store &W = *s->wsi;
    W.fmt = fmt; W.lv = plan_levels(width, height, fmt.tw, fmt.th, levels);
    W.fmt.nlev = (int)W.lv.size();
    W.total_tiles = 0;
    for (const Level &l : W.lv) W.total_tiles += (size_t)l.tx * l.ty;
    W.fmt.total = W.total_tiles;
    const size_t P = (size_t)fmt.planes();
    W.planes.assign(W.total_tiles * P, WsiPlane{ 0, 0, 0, 0 });
    W.used = 0;
    const size_t bpp = fmt.bpp();
    if ((rc = W.bytes.reserve((size_t)width * height * bpp / 2 + (1 << 20)))) return rc;
    // pyramid on the device (Downsample2xRGB / Downsample2xGrey, wsipyramid.go:10-55); level 0 is the caller's buffer
    std::vector<DevBuf> &img = s->wsi_pyr;
    if (img.size() < W.lv.size()) img.resize(W.lv.size());
    std::vector<const void *> lvl(W.lv.size(), d_pixels);
    for (size_t i = 1; i < W.lv.size(); i++) if ((rc = img[i].reserve((size_t)W.lv[i].w * W.lv[i].h * bpp + 64))) return rc;
    s->timer.reset(s->stream); s->timer.mark("k_wsi_downsample");
    for (size_t i = 1; i < W.lv.size(); i++) {
        launch_downsample(s->stream, fmt, lvl[i - 1], W.lv[i - 1].w, img[i].p, W.lv[i].w, W.lv[i].h);
        lvl[i] = img[i].p;
    }
    s->timer.mark("end");
    HIP_TRY(hipGetLastError());
    // each slab's streams go into the store in one copy, its raw planes one by one; the records then point into the store
    for (size_t i = 0; i < W.lv.size(); i++) {
        const Level &L = W.lv[i];
        rc = encode_level(s, fmt, lvl[i], L, s->wsi_planes, s->wsi_stats, session_slab_tiles(fmt), [&](const Slab &sl) -> int {
            uint64_t base = 0;
            int r;
            if (sl.stream_bytes && (r = W.append(s->stream, sl.streams, (size_t)sl.stream_bytes, &base))) return r;
            for (size_t p = 0; p < sl.planes.size(); p++) {
                WsiPlane wp = sl.planes[p];
                if (wp.mode == 2) wp.off = base + (wp.off - (uint64_t)(uintptr_t)sl.streams);
                else if (wp.mode == 3 && (r = W.append(s->stream, (const void *)(uintptr_t)wp.off, (size_t)wp.len, &wp.off))) return r;
                W.planes[((size_t)L.first + sl.t0) * P + p] = wp;
            }
            HIP_TRY(hipStreamSynchronize(s->stream));                                                    // the slab's planes are reused by the next one
            return MIC_OK;
        });
        if (rc) return rc;
    }
    if (total_tiles) *total_tiles = W.total_tiles;
    if (compressed_bytes) {                                                     // size of the file mic_hip_session_wsi_write would produce
        uint64_t n = 48 + 20 * (uint64_t)W.lv.size() + 16 * (uint64_t)W.total_tiles + (P == 3 ? 12 * (uint64_t)W.total_tiles : 0);
        for (const WsiPlane &wp : W.planes) n += plane_bytes(wp);
        *compressed_bytes = n;
    }
    return MIC_OK;
} MIC_ABI_CATCH

// The store as the container's payload, on the device: *d_payload (valid until the session's next wsi call), its size, and the
// byte length of every tile in container order (tile_lens[cap >= total tiles], host).  What a multi-GPU writer gathers.
int mic_hip_session_wsi_payload(mic_hip_session *s, const uint8_t **d_payload, uint64_t *payload_bytes, uint64_t *tile_lens, size_t cap) try {
    if (!s || !d_payload || !payload_bytes || !tile_lens || !s->wsi) return MIC_ERR_ARGS;
    int rc = s->activate();
    if (rc) return rc;
    if (cap < s->wsi->total_tiles) return MIC_ERR_CAPACITY;
    if ((size_t)kMaxGridX < s->wsi->total_tiles) return MIC_ERR_UNSUPPORTED;
    if ((rc = wsi_assemble(s, tile_lens, payload_bytes))) return rc;
    *d_payload = (const uint8_t *)s->wsi_payload.p;
    return MIC_OK;
} MIC_ABI_CATCH

// WriteMIC3 (wsiformat.go:99-165) around the store: one device-to-host copy of the assembled payload, then header, level table and
// tile index in front of it
int mic_hip_session_wsi_write(mic_hip_session *s, uint8_t *out, size_t out_cap, size_t *out_len) try {
    if (!s || !out || !out_len || !s->wsi) return MIC_ERR_ARGS;
    int rc = s->activate();
    if (rc) return rc;
    mic_hip_wsi_store &W = *s->wsi;
    if ((size_t)kMaxGridX < W.total_tiles) return MIC_ERR_UNSUPPORTED;
    const size_t hdr = 48 + 20 * W.lv.size() + 16 * W.total_tiles;
    std::vector<uint64_t> tlen(W.total_tiles); uint64_t total = 0;
    if ((rc = wsi_assemble(s, tlen.data(), &total))) return rc;
    if (out_cap < hdr + total) return MIC_ERR_CAPACITY;
    if ((rc = micapi::host_copy(s->device, s->wsi_payload.p, out + hdr, (size_t)total, false))) return rc;
    put_mic3_index(out, W.fmt, W.lv, tlen);
    *out_len = hdr + (size_t)total;
    return MIC_OK;
} MIC_ABI_CATCH

// every tile of one level, from the store, into a device image of the level's size (bytes per pixel as the slide's)
int mic_hip_session_wsi_decode_level(mic_hip_session *s, int level, uint8_t *d_pixels_out, size_t out_cap) try {
    if (!s || !d_pixels_out || !s->wsi) return MIC_ERR_ARGS;
    int rc = s->activate();
    if (rc) return rc;
    mic_hip_wsi_store &W = *s->wsi;
    if (level < 0 || level >= (int)W.lv.size()) return MIC_ERR_ARGS;
    const Mic3 &m = W.fmt;
    const Level &L = W.lv[(size_t)level];
    const size_t P = (size_t)m.planes();
    if ((size_t)L.w * L.h * m.bpp() > out_cap) return MIC_ERR_CAPACITY;
    const size_t ntl = (size_t)L.tx * L.ty, per = session_slab_tiles(m);
    for (size_t t0 = 0; t0 < ntl; t0 += per) {
        const size_t nt = std::min(per, ntl - t0);
        std::vector<int4> place(nt);
        for (size_t k = 0; k < nt; k++) {
            const int tx = (int)((t0 + k) % (size_t)L.tx), ty = (int)((t0 + k) / (size_t)L.tx);
            place[k] = make_int4(tx * m.tw, ty * m.th, std::min(m.tw, L.w - tx * m.tw), std::min(m.th, L.h - ty * m.th));
        }
        if ((rc = decode_planes(s, m, (const uint8_t *)W.bytes.p, W.planes.data() + ((size_t)L.first + t0) * P, nt, place.data(),
                                s->wsi_planes, s->wsi_stats, d_pixels_out, L.w))) return rc;
    }
    return MIC_OK;
} MIC_ABI_CATCH

// n patches of one level from the store: the plane records of the union's tiles as they stand (no blob is put together or parsed),
// their bytes where mic_hip_session_wsi_encode left them
static int session_wsi_read_patches_door(mic_hip_session *s, int level, const int32_t *xy, int n, int pw, int ph,
                                         void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec, Scale *sc) {
    if (!s || !s->wsi) return MIC_ERR_ARGS;
    mic_hip_wsi_store &W = *s->wsi;
    Mic3 m = W.fmt; m.lv = W.lv; m.nlev = (int)W.lv.size();
    size_t need = 0;
    OutFormat o;
    int rc = patch_args(m, level, xy, n, pw, ph, spec, o, out_cap, &need, sc);
    if (rc) return rc;
    if (stats) *stats = mic_hip_patch_stats{ 0, 0, 0 };
    if (n == 0) return MIC_OK;
    if (!d_out) return MIC_ERR_ARGS;
    if ((rc = s->activate()) || (rc = patch_pointer(s, &d_out, need))) return rc;
    if (!out_aligned(o, d_out)) return MIC_ERR_ARGS;
    const Level &L = m.lv[(size_t)level];
    const size_t P = (size_t)m.planes();
    // n patches of pw x ph at xy through the core into d_out as o says (the scaled call: its source rectangles into the staging tensor)
    auto native = [&](const int32_t *q, int k, int w, int h, const OutFormat &of, void *dst, size_t bytes, int32_t *st, mic_hip_patch_stats *ps) -> int {
        PatchPlan plan;
        int r;
        if ((r = plan_patches(L.w, L.h, m.tw, m.th, q, k, w, h, plan))) return r;
        // the records of units [u0, u0 + nt) of `dp`: the plan, or what a tile cache has left of it to decode
        auto records = [&](const PatchPlan &dp) {
            return [&, P](size_t u0, size_t nt, const uint8_t **base, std::vector<WsiPlane> &pl, int32_t *) -> int {
                for (size_t t = 0; t < nt; t++) {
                    const WsiPlane *rec = W.planes.data() + ((size_t)L.first + (size_t)dp.units[u0 + t].tile) * P;
                    pl.insert(pl.end(), rec, rec + P);
                }
                *base = (const uint8_t *)W.bytes.p;
                return MIC_OK;
            };
        };
        if (s->tile_cache) {
            CachePlan cp;
            const CacheOwner co{ s->tile_cache, s->tile_owner, (uint64_t)L.first };
            if ((r = cp.split(s, plan, std::vector<const Mic3 *>(plan.units.size(), &m), w, h, of, [&](size_t) { return co; }))) return r;
            const std::vector<const Mic3 *> um(cp.decode.units.size(), &m);
            return level_patches(s, cp.decode, um, k, w, h, of, [&](size_t) { return session_slab_tiles(m); }, records(cp.decode), dst, bytes, st, ps, &cp, &plan);
        }
        const std::vector<const Mic3 *> um(plan.units.size(), &m);
        return level_patches(s, plan, um, k, w, h, of, [&](size_t) { return session_slab_tiles(m); }, records(plan), dst, bytes, st, ps);
    };
    if (sc && !sc->unit()) {
        OutFormat on;
        if ((rc = on.make(nullptr, m.channels, m.bps, 1))) return rc;
        return scaled_level(s, m, level, xy, n, pw, ph, *sc, o, d_out, status, stats, s->tile_cache != nullptr,
                            [&](const int32_t *q, int ng, void *d_stage, size_t bytes, int32_t *st, mic_hip_patch_stats *ps) {
                                return native(q, ng, sc->sw, sc->sh, on, d_stage, bytes, st, ps);
                            });
    }
    return native(xy, n, pw, ph, o, d_out, need, status, stats);
}
int mic_hip_session_wsi_read_patches_as(mic_hip_session *s, int level, const int32_t *xy, int n, int pw, int ph,
                                        void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec) try {
    return session_wsi_read_patches_door(s, level, xy, n, pw, ph, d_out, out_cap, status, stats, spec, nullptr);
} MIC_ABI_CATCH
int mic_hip_session_wsi_read_patches_scaled(mic_hip_session *s, int level, const int32_t *xy, int n, int pw, int ph,
                                            void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec,
                                            int scale_num, int scale_den) try {
    Scale sc; sc.num = scale_num; sc.den = scale_den;
    return session_wsi_read_patches_door(s, level, xy, n, pw, ph, d_out, out_cap, status, stats, spec, &sc);
} MIC_ABI_CATCH

int mic_hip_session_set_tile_cache(mic_hip_session *s, mic_hip_tile_cache *c) try {
    if (!s) return MIC_ERR_ARGS;
    if (c == s->tile_cache) return MIC_OK;
    if (c && s->wsi) {
        const Mic3 &f = s->wsi->fmt;
        if (c->tw != f.tw || c->th != f.th || c->channels != f.channels || c->bps != f.bps) return MIC_ERR_ARGS;
    }
    if (s->tile_cache) s->tile_cache->detach(s->tile_owner);
    s->tile_cache = c;
    if (c) { std::lock_guard<std::mutex> lk(c->mu); c->attached++; s->tile_owner = tile_cache_new_owner(); }
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_session_tile_cache_probe(mic_hip_session *s, const uint64_t *tiles, size_t n, uint8_t *resident) try {
    if (!s || (n && (!tiles || !resident))) return MIC_ERR_ARGS;
    mic_hip_tile_cache *c = s->tile_cache;
    if (!c) { for (size_t i = 0; i < n; i++) resident[i] = 0; return MIC_OK; }
    std::lock_guard<std::mutex> lk(c->mu);
    for (size_t i = 0; i < n; i++) resident[i] = c->index.has(SlotIndex::Key{ s->tile_owner, tiles[i] }) ? 1 : 0;
    return MIC_OK;
} MIC_ABI_CATCH
int mic_hip_session_wsi_read_patches(mic_hip_session *s, int level, const int32_t *xy, int n, int pw, int ph,
                                     void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats) {
    return mic_hip_session_wsi_read_patches_as(s, level, xy, n, pw, ph, d_out, out_cap, status, stats, nullptr);
}

int mic_hip_session_wsi_levels(mic_hip_session *s, int *levels, int *widths, int *heights, int cap) try {
    if (!s || !s->wsi || !levels) return MIC_ERR_ARGS;
    *levels = (int)s->wsi->lv.size();
    for (int i = 0; i < *levels && i < cap; i++) { if (widths) widths[i] = s->wsi->lv[(size_t)i].w; if (heights) heights[i] = s->wsi->lv[(size_t)i].h; }
    return MIC_OK;
} MIC_ABI_CATCH

}  // extern "C"

// ==========================================================================================
// MIC3 streaming.  The writer takes a slide's rows in pushes of any size and codes it in bands of B tile rows (R = B * tile_h rows
// of level 0).  Every level k keeps, on the device, the rows it has made but not yet coded, behind one carried row: slot 0 of the
// level's buffer holds its row `base`, slot i row base + i.  Level k + 1 row y is the 2x2 box of level-k rows 2y and 2y + 1
// (Downsample2xRGB / Downsample2xGrey, wsipyramid.go:10-55, the odd last row and column dropped), so the row a level carries over
// a coded band edge is the one that still waits for its partner.  A level codes its rows once it holds B whole tile rows, or all of
// its rows: only its last tile row is ever padded, as in the one-shot file.
namespace {

// one level of a band: rows [lo, hi) are new in this band; buf = slot 0 (global row `base`); w = the level's width
struct BandLevel { uint8_t *buf; int w, base, lo, hi; };
struct BandPyr { BandLevel L[33]; int nlev, strip; };   // strip: level-0 columns per workgroup, a power of two >= 2^(nlev - 1)

typedef uint32_t bp_u32x4 __attribute__((ext_vector_type(4)));
typedef bp_u32x4 bp_u32x4_u __attribute__((aligned(1)));    // (rows are packed: a row starts at any byte)

// VP output pixels of one row from 2 * VP pixels of two source rows: 16-byte loads of each row, 16-byte stores.
// u8 (RGB or grey): VP = 16; u16 grey: VP = 8.  Each output sample is (a + b + c + d + 2) / 4 of its 2x2 source samples.
template <typename T, int C>
__device__ __forceinline__ void band_pyr_chunk(const uint8_t *ra, const uint8_t *rb, uint8_t *o) {
    constexpr int VP = sizeof(T) == 1 ? 16 : 8, NI = 2 * VP * C * (int)sizeof(T) / 16, NO = NI / 2;
    uint32_t a[4 * NI], b[4 * NI], r[4 * NO];
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const bp_u32x4 va = *(const bp_u32x4_u *)(ra + 16 * i), vb = *(const bp_u32x4_u *)(rb + 16 * i);
        a[4 * i] = va.x; a[4 * i + 1] = va.y; a[4 * i + 2] = va.z; a[4 * i + 3] = va.w;
        b[4 * i] = vb.x; b[4 * i + 1] = vb.y; b[4 * i + 2] = vb.z; b[4 * i + 3] = vb.w;
    }
#pragma unroll
    for (int i = 0; i < 4 * NO; i++) r[i] = 0;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int j = 0; j < VP; j++) {                         // word j of a row pair = source samples 2j, 2j + 1
            const uint32_t v = ((a[j] & 0xFFFFu) + (a[j] >> 16) + (b[j] & 0xFFFFu) + (b[j] >> 16) + 2) >> 2;
            r[j >> 1] |= v << (16 * (j & 1));
        }
    } else {
#pragma unroll
        for (int j = 0; j < VP * C; j++) {                     // output byte j = channel j % C of pixel j / C
            const int i1 = 2 * (j / C) * C + j % C, i2 = i1 + C;
            const uint32_t v = (((a[i1 >> 2] >> (8 * (i1 & 3))) & 0xFFu) + ((a[i2 >> 2] >> (8 * (i2 & 3))) & 0xFFu) +
                                ((b[i1 >> 2] >> (8 * (i1 & 3))) & 0xFFu) + ((b[i2 >> 2] >> (8 * (i2 & 3))) & 0xFFu) + 2) >> 2;
            r[j >> 2] |= v << (8 * (j & 3));
        }
    }
#pragma unroll
    for (int i = 0; i < NO; i++) *(bp_u32x4_u *)(o + 16 * i) = bp_u32x4{ r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3] };
}

// Every level's new rows of one band in one launch.  Workgroup g owns level-0 columns [g * strip, (g + 1) * strip) and so columns
// [g * strip >> k, (g + 1) * strip >> k) of level k: what it reads of level k - 1 it wrote itself (or an earlier launch did), so the
// levels follow each other behind a workgroup barrier and no workgroup waits for another.  A lane makes VP pixels of a row from
// 16-byte loads of the row pair; a chunk cut by the strip's or the row's end goes sample by sample.  32-bit index arithmetic only.
template <typename T, int C>
__global__ void __launch_bounds__(256) k_wsi_band_pyramid(BandPyr P) {
    constexpr int VP = sizeof(T) == 1 ? 16 : 8, BPP = C * (int)sizeof(T);
    const int g = blockIdx.x;
    for (int k = 1; k < P.nlev; k++) {
        const BandLevel D = P.L[k], S = P.L[k - 1];
        const int sk = P.strip >> k, x0 = g * sk, x1 = min(D.w, x0 + sk);
        if (D.lo < D.hi && x0 < x1) {
            const int nch = (x1 - x0 + VP - 1) / VP, items = nch * (D.hi - D.lo);
            const size_t srow = (size_t)S.w * BPP, drow = (size_t)D.w * BPP;
            for (int i = threadIdx.x; i < items; i += blockDim.x) {
                const int yr = i / nch, ch = i - yr * nch;
                const int y = D.lo + yr, px0 = x0 + ch * VP, n = min(VP, x1 - px0);
                const uint8_t *ra = S.buf + (size_t)(2 * y - S.base) * srow + (size_t)px0 * 2 * BPP, *rb = ra + srow;
                uint8_t *o = D.buf + (size_t)(y - D.base) * drow + (size_t)px0 * BPP;
                if (n == VP) { band_pyr_chunk<T, C>(ra, rb, o); continue; }
                const T *ta = (const T *)ra, *tb = (const T *)rb;
                T *to = (T *)o;
                for (int p = 0; p < n; p++)
#pragma unroll
                    for (int c = 0; c < C; c++)
                        to[p * C + c] = (T)(((uint32_t)ta[2 * p * C + c] + ta[2 * p * C + C + c] + tb[2 * p * C + c] + tb[2 * p * C + C + c] + 2) / 4);
            }
        }
        __syncthreads();                                        // level k is complete in this strip before level k + 1 reads it
    }
}
void launch_band_pyramid(hipStream_t st, const Mic3 &fmt, unsigned grid, const BandPyr &P) {
    if (fmt.planes() == 3) hipLaunchKernelGGL((k_wsi_band_pyramid<uint8_t, 3>), dim3(grid), dim3(256), 0, st, P);
    else if (fmt.bps == 16) hipLaunchKernelGGL((k_wsi_band_pyramid<uint16_t, 1>), dim3(grid), dim3(256), 0, st, P);
    else hipLaunchKernelGGL((k_wsi_band_pyramid<uint8_t, 1>), dim3(grid), dim3(256), 0, st, P);
}

}  // namespace

struct mic_hip_wsi_writer {
    std::mutex mu;
    mic_hip_write_fn write = nullptr; void *user = nullptr;
    Mic3 fmt; int width = 0, height = 0, tw = 0, th = 0;
    std::vector<Level> lv; size_t total_tiles = 0, hdr = 0;
    int B = 0, R = 0, strip = 0, nbuf = 0;        // band tile rows, band rows, columns per workgroup, levels the buffers hold
    mic_hip_session *s = nullptr;
    DevBuf pyr;
    SlabBufs bufs; size_t per = 1;                     // the tile path's buffers, tiles per slab
    std::vector<size_t> lvoff; std::vector<int> cap;   // per level: byte offset of its buffer in pyr, its slots
    std::vector<int> base, made, coded;                // per level: row in slot 0, rows made, rows coded
    std::vector<uint64_t> lens;                        // every tile's blob length (level 0's as they are coded)
    uint64_t l0_bytes = 0;                             // level-0 blob bytes written so far
    TileRun l0;                                        // the band's level-0 blobs on their way to the sink
    std::vector<TileRun> upper;                        // blobs of levels >= 1, held until finish
    size_t upper_bytes = 0, host_peak = 0;
    uint64_t device_bytes = 0, bands = 0;
    double pyr_ms = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int err = MIC_OK; bool done = false;
    ~mic_hip_wsi_writer() {
        if (s) {
            (void)s->activate();
            pyr.release(); bufs.release();
            if (ev0) (void)hipEventDestroy(ev0);
            if (ev1) (void)hipEventDestroy(ev1);
            mic_hip_session_destroy(s);
        }
    }
    size_t row_bytes(int k) const { return (size_t)(width >> k) * fmt.bpp(); }
    uint8_t *slot(int k, int row) { return (uint8_t *)pyr.p + lvoff[(size_t)k] + (size_t)(row - base[(size_t)k]) * row_bytes(k); }
    int sink(uint64_t off, const uint8_t *p, size_t n) { return n == 0 || write(user, off, p, n) == 0 ? MIC_OK : MIC_ERR_IO; }
    void note_host() { host_peak = std::max(host_peak, upper_bytes + lens.size() * 16 + l0.bytes.capacity()); }

    // level k codes `rows` rows from `coded` on (whole tile rows, or the rest of the level); level 0's blobs go to the sink
    int code_rows(int k, int rows) {
        const Level &G = lv[(size_t)k];
        const Level band{ G.w, rows, G.tx, (rows + th - 1) / th, 0 };
        TileRun up, &run = k == 0 ? l0 : up;
        run.first = (size_t)G.first + (size_t)(coded[(size_t)k] / th) * G.tx; run.bytes.clear(); run.lens.clear();
        int rc = code_level(s, fmt, slot(k, coded[(size_t)k]), band, bufs, per, run);
        if (rc) return rc;
        std::copy(run.lens.begin(), run.lens.end(), lens.begin() + (long)run.first);
        if (k == 0) {
            note_host();
            if ((rc = sink(hdr + l0_bytes, l0.bytes.data(), l0.bytes.size()))) return rc;
            l0_bytes += l0.bytes.size();
        } else {
            upper_bytes += up.bytes.size();
            upper.push_back(std::move(up));
            note_host();
        }
        coded[(size_t)k] += rows;
        // keep the rows not coded yet and the one before them at the front of the buffer (they never overlap what they replace:
        // at least one tile row was coded, at most tile_h - 1 rows are left behind)
        const int keep_from = coded[(size_t)k] - 1, n = made[(size_t)k] - keep_from;
        if (n > 0 && keep_from > base[(size_t)k])
            HIP_TRY(hipMemcpyAsync(slot(k, base[(size_t)k]), slot(k, keep_from), (size_t)n * row_bytes(k), hipMemcpyDeviceToDevice, s->stream));
        base[(size_t)k] = keep_from;
        return MIC_OK;
    }

    // level 0 holds a full band, or the slide's last rows: the other levels' new rows, then every level that has enough to code
    int band() {
        const int nlev = (int)lv.size();
        BandPyr P{};
        P.nlev = nlev; P.strip = strip;
        bool any = false;
        for (int k = 0; k < nlev; k++) {
            BandLevel &L = P.L[k];
            L.buf = (uint8_t *)pyr.p + lvoff[(size_t)k]; L.w = lv[(size_t)k].w; L.base = base[(size_t)k];
            L.lo = L.hi = made[(size_t)k];
            if (k > 0) {
                L.hi = std::min(lv[(size_t)k].h, made[(size_t)k - 1] / 2);
                if (L.hi - L.base > cap[(size_t)k] || 2 * L.lo < P.L[k - 1].base) return MIC_ERR_INTERNAL;   // (the slot bound of open)
                made[(size_t)k] = L.hi;
                any |= L.hi > L.lo;
            }
        }
        if (any) {
            const unsigned grid = (unsigned)((width + strip - 1) / strip);
            HIP_TRY(hipEventRecord(ev0, s->stream));
            launch_band_pyramid(s->stream, fmt, grid, P);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(ev1, s->stream));
        }
        for (int k = 0; k < nlev; k++) {
            const int pending = made[(size_t)k] - coded[(size_t)k];
            if (pending <= 0) continue;
            int rc = MIC_OK;
            if (made[(size_t)k] == lv[(size_t)k].h) rc = code_rows(k, pending);
            else if (pending / th >= B) rc = code_rows(k, pending / th * th);
            if (rc) return rc;
        }
        if (any) {
            float ms = 0;
            HIP_TRY(hipEventSynchronize(ev1));
            if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) pyr_ms += ms;
        }
        bands++;
        return MIC_OK;
    }
};

struct mic_hip_wsi_reader {
    std::mutex mu, io;                      // mu: one call at a time; io: one callback at a time (decode_box asks from several threads)
    mic_hip_read_fn read = nullptr; void *user = nullptr;
    uint64_t file_len = 0;
    Mic3 m;
    std::vector<uint8_t> head;              // header, level table, tile index
    mic_hip_tile_cache *cache = nullptr; uint64_t owner = 0;   // mic_hip_wsi_reader_set_cache (guarded by mu): the patch calls' tile cache and this reader's owner number in it
    // the blobs of `tiles` through the callback: every entry checked against file_len first, then one read per run of contiguous blobs
    int fetch(const std::vector<size_t> &tiles, std::vector<TileBlob> &blobs, std::vector<uint8_t> &keep) {
        std::vector<uint64_t> off(tiles.size()), len(tiles.size());
        size_t total = 0;
        for (size_t i = 0; i < tiles.size(); i++) {
            if (tiles[i] >= m.total) return MIC_ERR_CORRUPT;
            const uint8_t *e = head.data() + 48 + 20 * (size_t)m.nlev + 16 * tiles[i];
            const uint64_t bo = get_u64(e), bl = get_u64(e + 8);
            if (bo > file_len || bl > file_len || m.data_off + bo + bl > file_len) return MIC_ERR_CORRUPT;
            off[i] = m.data_off + bo; len[i] = bl; total += (size_t)bl;
        }
        keep.resize(total + 1);
        std::lock_guard<std::mutex> lk(io);
        size_t pos = 0;
        for (size_t i = 0; i < tiles.size();) {
            size_t j = i + 1, n = (size_t)len[i];
            while (j < tiles.size() && off[j] == off[j - 1] + len[j - 1]) n += (size_t)len[j++];
            if (n && read(user, off[i], keep.data() + pos, n) != 0) return MIC_ERR_IO;
            for (; i < j; i++) { blobs.push_back(TileBlob{ keep.data() + pos, (size_t)len[i] }); pos += (size_t)len[i]; }
        }
        return MIC_OK;
    }
    BlobSource source() {
        return [this](const std::vector<size_t> &t, std::vector<TileBlob> &b, std::vector<uint8_t> &k) { return fetch(t, b, k); };
    }
};

extern "C" {

int mic_hip_wsi_writer_open(int width, int height, int channels, int bits_per_sample, int tile_w, int tile_h, int levels,
                            int band_tile_rows, mic_hip_write_fn write, void *user, mic_hip_wsi_writer **out) try {
    if (!write || !out || width <= 0 || height <= 0 || tile_w < 0 || tile_h < 0 || band_tile_rows < 0) return MIC_ERR_ARGS;
    *out = nullptr;
    Mic3 fmt;
    int rc = wsi_options(width, height, channels, bits_per_sample, tile_w, tile_h, levels, fmt);
    if (rc) return rc;
    tile_w = fmt.tw; tile_h = fmt.th;
    const size_t bpp = fmt.bpp(), P = (size_t)fmt.planes(), npx = (size_t)tile_w * tile_h;
    const size_t tiles_x = ((size_t)width + tile_w - 1) / tile_w;
    if ((size_t)width * bpp * tile_h > ((size_t)1 << 31)) return MIC_ERR_UNSUPPORTED;    // one tile row of level 0 under 2 GiB
    std::unique_ptr<mic_hip_wsi_writer> w(new mic_hip_wsi_writer());
    w->write = write; w->user = user; w->fmt = fmt;
    w->width = width; w->height = height; w->tw = tile_w; w->th = tile_h;
    w->lv = plan_levels(width, height, tile_w, tile_h, levels);
    for (const Level &l : w->lv) w->total_tiles += (size_t)l.tx * l.ty;
    w->hdr = 48 + 20 * w->lv.size() + 16 * w->total_tiles;
    int dev = default_devices()[0];
    rc = check_device(dev);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(dev));
    // B: one band fills a sub-batch of the unit codec, at most 256 MiB of level-0 pixels
    size_t B = (size_t)band_tile_rows;
    if (B == 0) {
        const size_t fill = std::max<size_t>(1, std::min<size_t>(kMaxGridY / P, batch_units_for(npx, P)) / tiles_x);
        B = std::max<size_t>(1, std::min(fill, ((size_t)256 << 20) / ((size_t)width * bpp * tile_h)));
    }
    if (B * tile_h > (size_t)1 << 28) return MIC_ERR_UNSUPPORTED;
    w->B = (int)B; w->R = (int)B * tile_h;
    // the buffers hold every level the width allows (the level count follows the height): level 0 a band and the carried row,
    // level k >= 1 up to B tile rows not yet coded + a band's new rows (R / 2 + 1) + the carried row
    int nbuf = 0;
    while (nbuf < 33 && (width >> nbuf) >= 1) nbuf++;
    w->nbuf = nbuf;
    size_t bytes = 0;
    for (int k = 0; k < nbuf; k++) {
        const int c = k == 0 ? w->R + 1 : w->R + w->R / 2 + 2;
        w->lvoff.push_back(bytes); w->cap.push_back(c);
        bytes += ((size_t)c * w->row_bytes(k) + 255) & ~(size_t)255;
    }
    w->strip = 64;                                                  // (the kernel's workgroups: no memory hangs on it)
    while (w->strip < (1 << std::min((int)w->lv.size() - 1, 30)) || (width + w->strip - 1) / w->strip > 1024) w->strip *= 2;
    const size_t per = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(kMaxGridY / P, B * tiles_x), ((size_t)8 << 30) / (P * npx * 2)));
    if ((rc = mic_hip_session_create_on(dev, &w->s, (int)(per * P), npx))) return rc;
    mic_hip_session *s = w->s;
    if ((rc = w->pyr.reserve(bytes + 64))) return rc;
    if ((rc = w->bufs.planes.reserve(per * P * npx * 2 + 64))) return rc;
    if ((rc = w->bufs.stats.reserve(per * P * 8 + 64))) return rc;
    w->per = per;
    HIP_TRY(hipEventCreate(&w->ev0));
    HIP_TRY(hipEventCreate(&w->ev1));
    const size_t nl = w->lv.size();
    w->base.assign(nl, -1); w->made.assign(nl, 0); w->coded.assign(nl, 0);
    w->lens.assign(w->total_tiles, 0);
    w->device_bytes = w->pyr.cap + w->bufs.planes.cap + w->bufs.stats.cap + s->reserved_bytes();
    w->note_host();
    *out = w.release();
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_wsi_writer_push_rows(mic_hip_wsi_writer *w, const uint8_t *rows, int nrows) try {
    if (!w) return MIC_ERR_ARGS;
    std::lock_guard<std::mutex> lk(w->mu);
    if (w->err) return w->err;
    if (!rows || nrows <= 0 || w->done || (int64_t)w->made[0] + nrows > w->height) return MIC_ERR_ARGS;
    int rc = w->s->activate();
    const size_t rb = w->row_bytes(0);
    while (rc == MIC_OK && nrows > 0) {
        const int n = std::min(nrows, w->R - (w->made[0] - w->coded[0]));
        if (hipMemcpyAsync(w->slot(0, w->made[0]), rows, (size_t)n * rb, hipMemcpyHostToDevice, w->s->stream) != hipSuccess) { rc = MIC_ERR_DEVICE; break; }
        w->made[0] += n; rows += (size_t)n * rb; nrows -= n;
        if (w->made[0] - w->coded[0] == w->R || w->made[0] == w->height) rc = w->band();
    }
    if (rc == MIC_OK && hipStreamSynchronize(w->s->stream) != hipSuccess) rc = MIC_ERR_DEVICE;   // the caller's rows are consumed
    if (rc) w->err = rc;
    return rc;
} catch (...) { return w->err = exception_code(); }

int mic_hip_wsi_writer_finish(mic_hip_wsi_writer *w, uint64_t *file_len) try {
    if (!w) return MIC_ERR_ARGS;
    std::lock_guard<std::mutex> lk(w->mu);
    if (w->err) return w->err;
    if (w->done || w->made[0] != w->height) return MIC_ERR_ARGS;
    for (size_t k = 0; k < w->lv.size(); k++) if (w->coded[k] != w->lv[k].h) { w->err = MIC_ERR_INTERNAL; return w->err; }
    // the upper levels' blobs behind level 0's in file order, then header, level table and tile index (WriteMIC3,
    // wsiformat.go:99-165) at 0
    std::sort(w->upper.begin(), w->upper.end(), [](const TileRun &a, const TileRun &b) { return a.first < b.first; });
    uint64_t off = w->hdr + w->l0_bytes;
    int rc = MIC_OK;
    for (size_t r = 0; r < w->upper.size() && rc == MIC_OK; r++) { rc = w->sink(off, w->upper[r].bytes.data(), w->upper[r].bytes.size()); off += w->upper[r].bytes.size(); }
    if (rc == MIC_OK) {
        std::vector<uint8_t> head(w->hdr);
        put_mic3_index(head.data(), w->fmt, w->lv, w->lens);
        rc = w->sink(0, head.data(), head.size());
    }
    if (rc) { w->err = rc; return rc; }
    w->done = true;
    if (file_len) *file_len = off;
    return MIC_OK;
} catch (...) { return w->err = exception_code(); }

int mic_hip_wsi_writer_device_bytes(const mic_hip_wsi_writer *w, uint64_t *bytes) {
    if (!w || !bytes) return MIC_ERR_ARGS;
    *bytes = w->device_bytes;
    return MIC_OK;
}

int mic_hip_wsi_writer_stats(const mic_hip_wsi_writer *w, uint64_t *bands, int *band_rows, double *pyramid_ms, uint64_t *host_bytes_peak) {
    if (!w) return MIC_ERR_ARGS;
    if (bands) *bands = w->bands;
    if (band_rows) *band_rows = w->R;
    if (pyramid_ms) *pyramid_ms = w->pyr_ms;
    if (host_bytes_peak) *host_bytes_peak = w->host_peak;
    return MIC_OK;
}

void mic_hip_wsi_writer_close(mic_hip_wsi_writer *w) { delete w; }

int mic_hip_wsi_reader_open(mic_hip_read_fn read, void *user, uint64_t file_len, mic_hip_wsi_reader **out) try {
    if (!read || !out) return MIC_ERR_ARGS;
    *out = nullptr;
    std::unique_ptr<mic_hip_wsi_reader> r(new mic_hip_wsi_reader());
    r->read = read; r->user = user; r->file_len = file_len;
    if (file_len < 48) return MIC_ERR_CORRUPT;
    r->head.resize(48);
    if (read(user, 0, r->head.data(), 48) != 0) return MIC_ERR_IO;
    int rc = parse_mic3_fixed(r->head.data(), (size_t)file_len, r->m);
    if (rc) return rc;
    r->head.resize(r->m.data_off);
    if (r->m.data_off > 48 && read(user, 48, r->head.data() + 48, r->m.data_off - 48) != 0) return MIC_ERR_IO;
    if ((rc = parse_mic3_levels(r->head.data(), r->m))) return rc;
    *out = r.release();
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_wsi_reader_info(const mic_hip_wsi_reader *r, int *width, int *height, int *tile_w, int *tile_h, int *levels,
                            int *channels, int *bits_per_sample) {
    if (!r) return MIC_ERR_ARGS;
    if (width) *width = r->m.w; if (height) *height = r->m.h; if (tile_w) *tile_w = r->m.tw; if (tile_h) *tile_h = r->m.th;
    if (levels) *levels = r->m.nlev; if (channels) *channels = r->m.channels; if (bits_per_sample) *bits_per_sample = r->m.bps;
    return MIC_OK;
}

int mic_hip_wsi_reader_decompress_tile(mic_hip_wsi_reader *r, int level, int tile_x, int tile_y,
                                       uint8_t *out, size_t out_cap, int *out_w, int *out_h) try {
    if (!r || !out) return MIC_ERR_ARGS;
    std::lock_guard<std::mutex> lk(r->mu);
    return wsi_tile(r->source(), r->m, level, tile_x, tile_y, out, out_cap, out_w, out_h);
} MIC_ABI_CATCH

int mic_hip_wsi_reader_decompress_region(mic_hip_wsi_reader *r, int level, int x, int y, int w, int h,
                                         uint8_t *out, size_t out_cap, int *out_w, int *out_h) try {
    if (!r || !out) return MIC_ERR_ARGS;
    std::lock_guard<std::mutex> lk(r->mu);
    return wsi_region(r->source(), r->m, level, x, y, w, h, out, out_cap, out_w, out_h);
} MIC_ABI_CATCH

static int wsi_reader_read_patches_door(mic_hip_wsi_reader *r, int level, const int32_t *xy, int n, int pw, int ph,
                                        void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec, Scale *sc) {
    if (!r) return MIC_ERR_ARGS;
    std::lock_guard<std::mutex> lk(r->mu);
    size_t need = 0;
    OutFormat o;
    int rc = patch_args(r->m, level, xy, n, pw, ph, spec, o, out_cap, &need, sc);
    if (rc) return rc;
    if (stats) *stats = mic_hip_patch_stats{ 0, 0, 0 };
    if (n == 0) return MIC_OK;
    if (!d_out) return MIC_ERR_ARGS;
    DefaultLease lease;
    if ((rc = lease.acquire())) return rc;
    const CacheOwner co{ r->cache, r->owner, 0 };
    if (sc && !sc->unit()) return wsi_patches_scaled(r->source(), r->m, level, xy, n, pw, ph, *sc, o, d_out, need, status, stats, co);
    return wsi_patches(r->source(), r->m, level, xy, n, pw, ph, o, d_out, need, status, stats, co);
}
int mic_hip_wsi_reader_read_patches_as(mic_hip_wsi_reader *r, int level, const int32_t *xy, int n, int pw, int ph,
                                       void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec) try {
    return wsi_reader_read_patches_door(r, level, xy, n, pw, ph, d_out, out_cap, status, stats, spec, nullptr);
} MIC_ABI_CATCH
int mic_hip_wsi_reader_read_patches_scaled(mic_hip_wsi_reader *r, int level, const int32_t *xy, int n, int pw, int ph,
                                           void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats, const mic_hip_out_spec *spec,
                                           int scale_num, int scale_den) try {
    Scale sc; sc.num = scale_num; sc.den = scale_den;
    return wsi_reader_read_patches_door(r, level, xy, n, pw, ph, d_out, out_cap, status, stats, spec, &sc);
} MIC_ABI_CATCH

int mic_hip_wsi_reader_set_cache(mic_hip_wsi_reader *r, mic_hip_tile_cache *c) try {
    if (!r) return MIC_ERR_ARGS;
    std::lock_guard<std::mutex> lk(r->mu);
    if (c == r->cache) return MIC_OK;
    if (c && (!r->m.supported() || c->tw != r->m.tw || c->th != r->m.th || c->channels != r->m.channels || c->bps != r->m.bps)) return MIC_ERR_ARGS;
    if (r->cache) r->cache->detach(r->owner);
    r->cache = c;
    if (c) { std::lock_guard<std::mutex> lc(c->mu); c->attached++; r->owner = tile_cache_new_owner(); }
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_wsi_reader_cache_probe(mic_hip_wsi_reader *r, const uint64_t *tiles, size_t n, uint8_t *resident) try {
    if (!r || (n && (!tiles || !resident))) return MIC_ERR_ARGS;
    std::lock_guard<std::mutex> lk(r->mu);
    mic_hip_tile_cache *c = r->cache;
    if (!c) { for (size_t i = 0; i < n; i++) resident[i] = 0; return MIC_OK; }
    std::lock_guard<std::mutex> lc(c->mu);
    for (size_t i = 0; i < n; i++) resident[i] = c->index.has(SlotIndex::Key{ r->owner, tiles[i] }) ? 1 : 0;
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_wsi_reader_read_patches(mic_hip_wsi_reader *r, int level, const int32_t *xy, int n, int pw, int ph,
                                    void *d_out, size_t out_cap, int32_t *status, mic_hip_patch_stats *stats) {
    return mic_hip_wsi_reader_read_patches_as(r, level, xy, n, pw, ph, d_out, out_cap, status, stats, nullptr);
}

// mic_hip_wsi_multi_read_patches through readers.  Only the readers some patch names are touched: each distinct one is locked once,
// in address order (one order for every caller), and asked for its blobs in one fetch.
static int wsi_readers_read_patches_door(mic_hip_wsi_reader *const *readers, int nreaders,
                                         const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                         void *d_out, size_t out_cap, int32_t *status, mic_hip_multi_patch_stats *stats, const mic_hip_out_spec *spec, Scale *sc) {
    if (nreaders < 0 || (nreaders > 0 && !readers)) return MIC_ERR_ARGS;
    size_t need = 0;
    OutFormat o;
    const int rc = multi_args(xysl, n, pw, ph, channels, bits_per_sample, spec, nreaders, o, out_cap, &need, sc);
    if (rc) return rc;
    std::vector<mic_hip_wsi_reader *> named;
    for (int i = 0; i < n; i++) {
        const int32_t f = xysl[4 * (size_t)i + 2];
        if (f < 0 || f >= nreaders) return MIC_ERR_ARGS;
        if (readers[f]) named.push_back(readers[f]);
    }
    std::sort(named.begin(), named.end(), std::less<mic_hip_wsi_reader *>());
    named.erase(std::unique(named.begin(), named.end()), named.end());
    std::vector<std::unique_lock<std::mutex>> locks;
    locks.reserve(named.size());
    for (mic_hip_wsi_reader *r : named) locks.emplace_back(r->mu);
    auto slides = [&](MultiPlan &plan) {
        plan.slides.resize((size_t)nreaders);
        for (int i = 0; i < n; i++) {
            const size_t f = (size_t)xysl[4 * (size_t)i + 2];
            mic_hip_wsi_reader *r = readers[f];
            if (r) { plan.slides[f].head = r->head.data(); plan.slides[f].file_len = r->file_len; plan.slides[f].m = &r->m; }
        }
    };
    const MultiFetch fetch = [&](uint32_t f, const std::vector<size_t> &tiles, std::vector<TileBlob> &blobs, std::vector<uint8_t> &keep) {
        return readers[f]->fetch(tiles, blobs, keep);
    };
    // (each reader its own cache, shared, or none; a unit's reader is one of `named`)
    const std::function<CacheOwner(uint32_t)> cache_of = [&](uint32_t f) { return CacheOwner{ readers[f]->cache, readers[f]->owner, 0 }; };
    if (sc && !sc->unit()) {
        bool cached = false;
        for (mic_hip_wsi_reader *r : named) cached = cached || r->cache != nullptr;
        return multi_call_scaled(slides, nreaders, fetch, xysl, n, pw, ph, channels, bits_per_sample, *sc, o, d_out, need, status, stats, cache_of, cached);
    }
    MultiPlan plan;
    slides(plan);
    return multi_call(plan, fetch, xysl, n, pw, ph, channels, bits_per_sample, o, d_out, need, status, stats, cache_of);
}
int mic_hip_wsi_readers_read_patches_as(mic_hip_wsi_reader *const *readers, int nreaders,
                                        const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                        void *d_out, size_t out_cap, int32_t *status, mic_hip_multi_patch_stats *stats, const mic_hip_out_spec *spec) try {
    return wsi_readers_read_patches_door(readers, nreaders, xysl, n, pw, ph, channels, bits_per_sample, d_out, out_cap, status, stats, spec, nullptr);
} MIC_ABI_CATCH
int mic_hip_wsi_readers_read_patches_scaled(mic_hip_wsi_reader *const *readers, int nreaders,
                                            const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                            void *d_out, size_t out_cap, int32_t *status, mic_hip_multi_patch_stats *stats, const mic_hip_out_spec *spec,
                                            int scale_num, int scale_den) try {
    Scale sc; sc.num = scale_num; sc.den = scale_den;
    return wsi_readers_read_patches_door(readers, nreaders, xysl, n, pw, ph, channels, bits_per_sample, d_out, out_cap, status, stats, spec, &sc);
} MIC_ABI_CATCH
int mic_hip_wsi_readers_read_patches(mic_hip_wsi_reader *const *readers, int nreaders,
                                     const int32_t *xysl, int n, int pw, int ph, int channels, int bits_per_sample,
                                     void *d_out, size_t out_cap, int32_t *status, mic_hip_multi_patch_stats *stats) {
    return mic_hip_wsi_readers_read_patches_as(readers, nreaders, xysl, n, pw, ph, channels, bits_per_sample, d_out, out_cap, status, stats, nullptr);
}

void mic_hip_wsi_reader_close(mic_hip_wsi_reader *r) {
    if (r && r->cache) r->cache->detach(r->owner);                                          // (its entries go with it)
    delete r;
}

}  // extern "C"
