// mic_rgb_batch.hip -- CompressRGB / DecompressRGB (rgbcompress.go:25-33) of many images of different sizes per call.
//
// CompressRGB = compressRGBTileBlob on the whole image (wsicompress.go:319-363): YCoCg-R, Co and Cg zigzagged, three u16 planes, per
// plane constant-zero / constant / CompressSingleFrame / raw (compressWSIPlane, :373-421), [Y_len][Co_len][Cg_len] + the planes.
// The single-image path (mic_api_ext.hip) runs that as one "tile" of a slide; its kernels take one tile size per launch and planes
// at tile * 3 * npx.  Here every launch is driven by a descriptor table: an image is its own tile, there is no padding, and work is
// cut into chunks of kRgbChunk pixels by a prefix sum over the table, so a 1 x 1 image beside a 1920 x 1080 one costs one block.
// This file holds the kernels, the core on device buffers (rgb_encode_run / rgb_decode_run) and the session entry points; the host
// pipeline -- sub-batches, staging, devices -- is with the other containers' in mic_host_io.hip.
#include "mic_session.h"
#include "mic_staged.h"
#include "mic_wave.h"

namespace {

constexpr uint32_t kRgbChunk = 4096;                 // pixels a block of 256 threads works on
constexpr size_t kRgbMaxPx = (size_t)1 << 26;        // as mic_hip_rgb_compress
constexpr int kRgbMaxImages = 65535 / 3;             // an image's three units: a launch's grid y in the unit codec

// An image of a sub-batch: RGB at rgb + rgb_off (any byte alignment), its Y plane at planes + plane_off, Co and Cg rgb_stride(w * h)
// u16 behind it each (mic_session.h); chunk0 = the chunks of the images before it; slot: where its statistics go.
struct RgbDesc { uint64_t rgb_off, plane_off; int32_t w, h; uint32_t chunk0, slot; };
static_assert(sizeof(RgbDesc) == 32, "the table travels as four u64 per image");

typedef uint16_t rgb_u16x4 __attribute__((ext_vector_type(4)));
typedef rgb_u16x4 RgbQ __attribute__((aligned(2)));                    // (a group of four pixels starts at any even address: gfx950 stores it unaligned)

// the image chunk `chunk` belongs to: the last one whose chunk0 <= chunk
__device__ __forceinline__ RgbDesc rgb_find(const RgbDesc *tab, int nimg, uint32_t chunk) {
    int lo = 0, hi = nimg - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tab[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1; }
    return tab[lo];
}

// YCoCgRForward (asm_amd64.go:88-104) + ZigZag of Co and Cg (deltazigzagcompressu16.go:108-111): k_wsi_tile_planes' arithmetic
__device__ __forceinline__ void rgb_forward(int r, int g, int b, uint32_t &v0, uint32_t &v1, uint32_t &v2) {
    const int co = r - b;
    const int t = b + (co >> 1);
    const int cg = g - t;
    const int yv = t + (cg >> 1);
    v0 = (uint16_t)yv;
    v1 = (uint16_t)(((int16_t)co << 1) ^ ((int16_t)co >> 15));
    v2 = (uint16_t)(((int16_t)cg << 1) ^ ((int16_t)cg >> 15));
}
// UnZigZag (:113-116) + YCoCgRInverse (asm_amd64.go:106-121): k_wsi_planes_to_rgb's arithmetic; returns r | g << 8 | b << 16
__device__ __forceinline__ uint32_t rgb_inverse(uint32_t yv, uint32_t uco, uint32_t ucg) {
    const int co = (int)(int16_t)((uco >> 1) ^ (uint16_t)(-(int)(uco & 1)));
    const int cg = (int)(int16_t)((ucg >> 1) ^ (uint16_t)(-(int)(ucg & 1)));
    const int t = (int)yv - (cg >> 1);
    const int g = cg + t;
    const int b = t - (co >> 1);
    const int r = co + b;
    return (uint32_t)(uint8_t)r | ((uint32_t)(uint8_t)g << 8) | ((uint32_t)(uint8_t)b << 16);
}

// The forward transform and the constant / max scan of compressWSIPlane (wsicompress.go:375-385) for every image of the table.
// grid = the table's chunks in all, block = 256.  stats: [slot][3] {min, ~max} as u32 pairs, pre-set to 0xFFFFFFFF (both fall by
// atomicMin, so one memset prepares them).
// GROUPED: a lane takes four pixels whose twelve bytes are three aligned dwords.  The image's bytes lie back to back, so only its
// first byte's alignment matters: the first (address & 3) pixels -- 3 k = -address (mod 4) iff k = address (mod 4) -- are the head,
// taken byte-wise by chunk 0, the up to three pixels behind the last whole group the tail, taken by the last chunk.  Chunk c takes
// groups [1024 c, 1024 c + 1024): four per lane, a wave's lanes on neighbouring groups.  !GROUPED: three byte loads per pixel.
// BOUNDS: blockIdx.x < sum of the images' chunks, so c < ceil(npx / 4096); a pixel index is used only below npx = w h; a group g <
// (npx - head) / 4 reads bytes [3 (head + 4 g), 3 (head + 4 g) + 12) of the image's 3 npx and writes pixels head + 4 g .. + 3.
template <bool GROUPED>
__global__ void __launch_bounds__(256) k_rgb_batch_planes(const uint8_t *rgb, const RgbDesc *tab, int nimg, uint16_t *planes, uint32_t *stats) {
    const RgbDesc im = rgb_find(tab, nimg, blockIdx.x);
    const uint32_t c = blockIdx.x - im.chunk0, npx = (uint32_t)im.w * (uint32_t)im.h, tid = threadIdx.x;
    const uint32_t nchunks = (npx + kRgbChunk - 1) / kRgbChunk;
    if (c >= nchunks) return;
    const mic_gp<const uint8_t> src = mic_g(rgb) + im.rgb_off;
    const size_t ps = rgb_stride(npx);
    const mic_gp<uint16_t> py = mic_g(planes) + im.plane_off, pco = py + ps, pcg = pco + ps;
    uint32_t mn[3] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu }, mx[3] = { 0, 0, 0 };
    auto note = [&](uint32_t v0, uint32_t v1, uint32_t v2) {
        mn[0] = min(mn[0], v0); mx[0] = max(mx[0], v0);
        mn[1] = min(mn[1], v1); mx[1] = max(mx[1], v1);
        mn[2] = min(mn[2], v2); mx[2] = max(mx[2], v2);
    };
    auto one = [&](uint32_t i) {                                        // pixel i, byte-wise
        const mic_gp<const uint8_t> p = src + (size_t)i * 3;
        uint32_t v0, v1, v2;
        rgb_forward(p[0], p[1], p[2], v0, v1, v2);
        py[i] = (uint16_t)v0; pco[i] = (uint16_t)v1; pcg[i] = (uint16_t)v2;
        note(v0, v1, v2);
    };
    if (!GROUPED) {
#pragma unroll 4
        for (uint32_t k = 0; k < kRgbChunk / 256; k++) { const uint32_t i = c * kRgbChunk + k * 256 + tid; if (i < npx) one(i); }
    } else {
        const uint32_t head = min(npx, (uint32_t)((uintptr_t)(rgb + im.rgb_off) & 3u)), ngroups = (npx - head) / 4, tail0 = head + 4 * ngroups;
        if (c == 0 && tid < head) one(tid);
        if (c == nchunks - 1 && tail0 + tid < npx) one(tail0 + tid);
#pragma unroll
        for (uint32_t k = 0; k < kRgbChunk / 1024; k++) {
            const uint32_t g = c * (kRgbChunk / 4) + k * 256 + tid;
            if (g >= ngroups) continue;
            const uint32_t i = head + 4 * g;
            const mic_gp<const uint32_t> q = (mic_gp<const uint32_t>)(src + (size_t)i * 3);
            const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];             // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
            rgb_u16x4 a, o, e;
            uint32_t v0, v1, v2;
            rgb_forward(d0 & 255, (d0 >> 8) & 255, (d0 >> 16) & 255, v0, v1, v2); a.x = (uint16_t)v0; o.x = (uint16_t)v1; e.x = (uint16_t)v2; note(v0, v1, v2);
            rgb_forward(d0 >> 24, d1 & 255, (d1 >> 8) & 255, v0, v1, v2);         a.y = (uint16_t)v0; o.y = (uint16_t)v1; e.y = (uint16_t)v2; note(v0, v1, v2);
            rgb_forward((d1 >> 16) & 255, d1 >> 24, d2 & 255, v0, v1, v2);        a.z = (uint16_t)v0; o.z = (uint16_t)v1; e.z = (uint16_t)v2; note(v0, v1, v2);
            rgb_forward((d2 >> 8) & 255, (d2 >> 16) & 255, d2 >> 24, v0, v1, v2); a.w = (uint16_t)v0; o.w = (uint16_t)v1; e.w = (uint16_t)v2; note(v0, v1, v2);
            *(mic_gp<RgbQ>)(py + i) = a; *(mic_gp<RgbQ>)(pco + i) = o; *(mic_gp<RgbQ>)(pcg + i) = e;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        mn[k] = mic_wave_reduce_min(mn[k]); mx[k] = mic_wave_reduce_max(mx[k]);
        if ((tid & 63) == 0 && mn[k] <= mx[k]) { atomicMin(&stats[((size_t)im.slot * 3 + k) * 2], mn[k]); atomicMin(&stats[((size_t)im.slot * 3 + k) * 2 + 1], ~mx[k]); }
    }
}

// The inverse: the three planes of every image of the table -> interleaved u8 at out + rgb_off.  grid = the table's chunks, block
// = 256; four pixels a lane as three aligned dword stores, head and tail byte-wise, cut as in k_rgb_batch_planes by the alignment of
// the image's first OUTPUT byte.  BOUNDS: as there, with reads and writes exchanged.
__global__ void __launch_bounds__(256) k_rgb_batch_from_planes(const uint16_t *planes, const RgbDesc *tab, int nimg, uint8_t *out) {
    const RgbDesc im = rgb_find(tab, nimg, blockIdx.x);
    const uint32_t c = blockIdx.x - im.chunk0, npx = (uint32_t)im.w * (uint32_t)im.h, tid = threadIdx.x;
    const uint32_t nchunks = (npx + kRgbChunk - 1) / kRgbChunk;
    if (c >= nchunks) return;
    const mic_gp<uint8_t> dst = mic_g(out) + im.rgb_off;
    const size_t ps = rgb_stride(npx);
    const mic_gp<const uint16_t> py = mic_g(planes) + im.plane_off, pco = py + ps, pcg = pco + ps;
    auto one = [&](uint32_t i) {
        const uint32_t v = rgb_inverse(py[i], pco[i], pcg[i]);
        const mic_gp<uint8_t> o = dst + (size_t)i * 3;
        o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16);
    };
    const uint32_t head = min(npx, (uint32_t)((uintptr_t)(out + im.rgb_off) & 3u)), ngroups = (npx - head) / 4, tail0 = head + 4 * ngroups;
    if (c == 0 && tid < head) one(tid);
    if (c == nchunks - 1 && tail0 + tid < npx) one(tail0 + tid);
#pragma unroll
    for (uint32_t k = 0; k < kRgbChunk / 1024; k++) {
        const uint32_t g = c * (kRgbChunk / 4) + k * 256 + tid;
        if (g >= ngroups) continue;
        const uint32_t i = head + 4 * g;
        const rgb_u16x4 a = *(mic_gp<const RgbQ>)(py + i), o = *(mic_gp<const RgbQ>)(pco + i), e = *(mic_gp<const RgbQ>)(pcg + i);
        const uint32_t p0 = rgb_inverse(a.x, o.x, e.x), p1 = rgb_inverse(a.y, o.y, e.y), p2 = rgb_inverse(a.z, o.z, e.z), p3 = rgb_inverse(a.w, o.w, e.w);
        const mic_gp<uint32_t> q = (mic_gp<uint32_t>)(dst + (size_t)i * 3);
        q[0] = p0 | (p1 << 24); q[1] = (p1 >> 8) | (p2 << 16); q[2] = (p2 >> 16) | (p3 << 8);
    }
}

// Planes the unit codec does not write, on decode (decompressWSIPlane, wsicompress.go:494-519): mode 0 / 1 a constant -- the plane's
// padded extent in 16-byte stores, a plane starts 16-byte aligned --, mode 3 the raw little-endian pixels at blobs + src_off, which
// may be an odd address: two byte loads a pixel.  grid = (chunks, records): as k_fill_spans, a record per plane.
// BOUNDS: a record's plane holds rgb_stride(npx) u16 at plane_off; the host has checked that the blob holds 2 npx bytes at src_off.
struct RgbFill { uint64_t plane_off, src_off; uint32_t npx, mode_value; };   // mode_value = mode | value << 8
__global__ void __launch_bounds__(256) k_rgb_batch_fill(uint16_t *planes, const uint8_t *blobs, const RgbFill *fill) {
    const RgbFill f = fill[blockIdx.y];
    const mic_gp<uint16_t> p = mic_g(planes) + f.plane_off;
    const size_t step = (size_t)gridDim.x * 256, i0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if ((f.mode_value & 0xFFu) == 3u) {
        const mic_gp<const uint8_t> s = mic_g(blobs) + f.src_off;
        for (size_t i = i0; i < f.npx; i += step) p[i] = (uint16_t)(s[2 * i] | (s[2 * i + 1] << 8));
    } else {
        typedef uint32_t fv4 __attribute__((ext_vector_type(4)));
        const uint32_t v = (f.mode_value >> 8) & 0xFFFFu, vv = v | (v << 16);
        const fv4 q = { vv, vv, vv, vv };
        const size_t n8 = rgb_stride(f.npx) / 8;
        for (size_t i = i0; i < n8; i += step) *(mic_gp<fv4>)(p + i * 8) = q;
    }
}

// compressRGBTileBlob's output (wsicompress.go:349-363) for every image that coded, at payload + dst: for a MICR file "MICR", w, h
// (writeMICRFile, cmd/mic-compress/main.go:62-91), then [Y_len][Co_len][Cg_len] u32 LE, then each plane as mode byte + constant /
// stream / raw pixels.  k_wsi_assemble's records carry no per-image header and live in another translation unit: this is its
// sibling with one record per image.  grid = (images, 3 planes, slices of a plane's copy), block = 256.
// BOUNDS: the host lays the blobs out from the same lengths, so image t writes [dst, dst + header + 12 + the planes' bytes) only.
struct RgbAsm { uint64_t src[3]; uint64_t dst; uint32_t len[3]; uint32_t mode_value[3]; int32_t w, h; uint32_t container, pad; };
__device__ __forceinline__ uint32_t rgb_plane_bytes(uint32_t mode_value, uint32_t len) { const uint32_t m = mode_value & 0xFFu; return m == 0 ? 1u : m == 1 ? 3u : 1u + len; }
__device__ __forceinline__ void rgb_put_u32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
__global__ void __launch_bounds__(256) k_rgb_batch_assemble(const RgbAsm *recs, uint8_t *payload) {
    const RgbAsm &r = recs[blockIdx.x];
    const uint32_t p = blockIdx.y, hdr = r.container ? 12u : 0u;
    uint64_t off = hdr + 12;
    for (uint32_t q = 0; q < p; q++) off += rgb_plane_bytes(r.mode_value[q], r.len[q]);
    uint8_t *base = payload + r.dst, *d = base + off;
    const uint32_t mode = r.mode_value[p] & 0xFFu, value = r.mode_value[p] >> 8, len = r.len[p];
    if (blockIdx.z == 0 && threadIdx.x == 0) {
        if (p == 0 && hdr) { base[0] = 'M'; base[1] = 'I'; base[2] = 'C'; base[3] = 'R'; rgb_put_u32(base + 4, (uint32_t)r.w); rgb_put_u32(base + 8, (uint32_t)r.h); }
        rgb_put_u32(base + hdr + 4 * p, rgb_plane_bytes(r.mode_value[p], len));
        d[0] = (uint8_t)mode;
        if (mode == 1) { d[1] = (uint8_t)value; d[2] = (uint8_t)(value >> 8); }
    }
    if (mode >= 2) {
        typedef uint32_t wv4 __attribute__((ext_vector_type(4)));
        typedef wv4 WQ __attribute__((aligned(1)));
        const uint8_t *sp = (const uint8_t *)(uintptr_t)r.src[p]; uint8_t *dp = d + 1;
        const uint32_t nv = len / 16;
        for (uint32_t i = blockIdx.z * 256 + threadIdx.x; i < nv; i += 256 * gridDim.z) *(WQ *)(dp + (size_t)i * 16) = *(const WQ *)(sp + (size_t)i * 16);
        if (blockIdx.z == 0 && threadIdx.x < (len & 15u)) dp[(size_t)nv * 16 + threadIdx.x] = sp[(size_t)nv * 16 + threadIdx.x];
    }
}

// RgbHead of every blob of a device buffer (micapi::rgb_head_of, on the device): one thread per blob, begins[i] .. ends[i] its bytes
// (blobs that lie back to back: ends = begins + 1).
// BOUNDS: a byte is read only at an index below the blob's length.
__global__ void __launch_bounds__(256) k_rgb_batch_heads(const uint8_t *blobs, const uint64_t *begins, const uint64_t *ends, int n, RgbHead *heads) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    RgbHead h;
    memset(&h, 0, sizeof h);
    const uint64_t b0 = begins[i], bl = ends[i] >= b0 ? ends[i] - b0 : 0;
    const uint8_t *c = blobs + b0;
    if (bl >= 12) {
        uint64_t off = 12;
        for (int p = 0; p < 3; p++) h.len[p] = (uint32_t)c[4 * p] | ((uint32_t)c[4 * p + 1] << 8) | ((uint32_t)c[4 * p + 2] << 16) | ((uint32_t)c[4 * p + 3] << 24);
        for (int p = 0; p < 3; p++) {
            for (uint32_t k = 0; k < 3; k++) if (k < h.len[p] && off + k < bl) h.b[p][k] = c[off + k];
            off += h.len[p];
        }
    }
    heads[i] = h;
}

std::atomic<int> g_rgb_bytewise{0};                  // mic_hip_debug_rgb_planes_bytewise: the plane kernel's byte-wise form (A / B runs)

}  // namespace

namespace micapi {

void rgb_head_of(const uint8_t *c, uint64_t bl, RgbHead &h) {
    memset(&h, 0, sizeof h);
    if (bl < 12) return;
    uint64_t off = 12;
    for (int p = 0; p < 3; p++) h.len[p] = get_u32(c + 4 * p);
    for (int p = 0; p < 3; p++) {
        for (uint32_t k = 0; k < 3; k++) if (k < h.len[p] && off + k < bl) h.b[p][k] = c[off + k];
        off += h.len[p];
    }
}

int rgb_heads_enqueue(hipStream_t stream, const uint8_t *d_blobs, const uint64_t *d_begins, const uint64_t *d_ends, int n, RgbHead *d_heads) {
    if (n <= 0) return MIC_OK;
    hipLaunchKernelGGL(k_rgb_batch_heads, dim3((unsigned)(n + 255) / 256), dim3(256), 0, stream, d_blobs, d_begins, d_ends, n, d_heads);
    HIP_TRY(hipGetLastError());
    return MIC_OK;
}

int rgb_parse_head(const RgbHead &h, uint64_t bl, size_t npx, RgbPlaneRec pl[3], int32_t *failed_plane) {
    *failed_plane = -1;
    if (bl < 12) return MIC_ERR_CORRUPT;                                                    // "RGB tile blob too small", wsicompress.go:432-434
    if (12 + (uint64_t)h.len[0] + h.len[1] + h.len[2] > bl) return MIC_ERR_CORRUPT;       // "truncated", :441-443
    uint64_t off = 12;
    for (int p = 0; p < 3; p++) {                                                           // decompressWSIPlane, :487-524
        const uint64_t dl = h.len[p];
        const uint8_t mode = h.b[p][0];
        pl[p] = RgbPlaneRec{ mode, 0, off + 1, 0 };
        bool ok = dl != 0;                                                                  // "empty plane data"
        if (ok && mode == 1) { ok = dl >= 3; pl[p].value = (uint16_t)(h.b[p][1] | (h.b[p][2] << 8)); }
        else if (ok && mode == 2) { pl[p].len = dl - 1; ok = dl > 1; }                      // (an empty stream: DecompressSingleFrame rejects it)
        else if (ok && mode == 3) { pl[p].len = 2 * (uint64_t)npx; ok = dl >= 1 + 2 * (uint64_t)npx; }
        else if (ok && mode > 3) ok = false;                                                // "unknown plane mode"
        if (!ok) { *failed_plane = p; return MIC_ERR_CORRUPT; }
        off += dl;
    }
    return MIC_OK;
}

int rgb_next_cut(const std::function<size_t(int)> &npx, int i0, int n, size_t target_px) {
    // (beside a unit's slabs: its share of the staged RGB, the planes, the packed streams and the assembled blobs, two halves of each that has two)
    return (int)next_sub_batch((size_t)i0, (size_t)n, [&](size_t i) { return npx((int)i); },
        cap_by_largest([](size_t mp) { return batch_units_for(std::max<size_t>(mp, 1), 1, 10 * mp) / 3; }),
        CutRule{ (size_t)kRgbMaxImages, ~(size_t)0, target_px });
}

// the table of the images that take part (status MIC_OK), their planes laid out back to back; of[k]: the image behind table row k
static int rgb_table(const std::function<bool(int, uint64_t &, int32_t &, int32_t &)> &image, int n, std::vector<RgbDesc> &tab, std::vector<int> &of, size_t *plane_px) {
    size_t poff = 0; uint64_t chunks = 0;
    for (int i = 0; i < n; i++) {
        uint64_t rgb_off; int32_t w, h;
        if (!image(i, rgb_off, w, h)) continue;
        const size_t npx = (size_t)w * (size_t)h;
        tab.push_back(RgbDesc{ rgb_off, (uint64_t)poff, w, h, (uint32_t)chunks, (uint32_t)tab.size() });
        of.push_back(i);
        poff += 3 * rgb_stride(npx); chunks += (npx + kRgbChunk - 1) / kRgbChunk;
        if (chunks > 0x7FFFFFFFull) return MIC_ERR_UNSUPPORTED;                             // (a launch's grid x; callers cut sub-batches far below it)
    }
    *plane_px = poff;
    return MIC_OK;
}
static uint32_t rgb_chunks(const std::vector<RgbDesc> &tab) {
    const RgbDesc &l = tab.back();
    return l.chunk0 + (uint32_t)(((size_t)l.w * (size_t)l.h + kRgbChunk - 1) / kRgbChunk);
}

int rgb_encode_run(mic_hip_session *s, const uint8_t *d_rgb, RgbImage *img, int n, DevBuf &payload, uint64_t pay0, uint64_t *pay_end) {
    *pay_end = pay0;
    if (n > kRgbMaxImages) return MIC_ERR_UNSUPPORTED;
    std::vector<RgbDesc> tab; std::vector<int> of; size_t plane_px = 0;
    int rc = rgb_table([&](int i, uint64_t &off, int32_t &w, int32_t &h) { off = img[i].rgb_off; w = img[i].w; h = img[i].h; return img[i].status == MIC_OK; }, n, tab, of, &plane_px);
    if (rc) return rc;
    const size_t m = tab.size();
    if (m == 0) return MIC_OK;
    if (!s->stream) HIP_TRY(mic_stream_create(&s->stream));
    // aux: the table, the statistics, the assembly records
    const size_t tab_b = m * sizeof(RgbDesc), st_b = m * 3 * 8, rec_b = m * sizeof(RgbAsm);
    if ((rc = s->rgb_planes.reserve(plane_px * 2 + 64)) || (rc = s->rgb_aux.reserve(tab_b + st_b + rec_b + 64)) || (rc = s->rgb_pin.reserve(m * 3))) return rc;
    uint16_t *d_planes = (uint16_t *)s->rgb_planes.p;
    RgbDesc *d_tab = (RgbDesc *)s->rgb_aux.p;
    uint32_t *d_stats = (uint32_t *)((char *)s->rgb_aux.p + tab_b);
    RgbAsm *d_recs = (RgbAsm *)((char *)s->rgb_aux.p + tab_b + st_b);
    HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab_b, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemsetAsync(d_stats, 0xFF, st_b, s->stream));
    s->timer.reset(s->stream); s->timer.mark("k_rgb_batch_planes");
    if (g_rgb_bytewise.load()) hipLaunchKernelGGL(k_rgb_batch_planes<false>, dim3(rgb_chunks(tab)), dim3(256), 0, s->stream, d_rgb, (const RgbDesc *)d_tab, (int)m, d_planes, d_stats);
    else hipLaunchKernelGGL(k_rgb_batch_planes<true>, dim3(rgb_chunks(tab)), dim3(256), 0, s->stream, d_rgb, (const RgbDesc *)d_tab, (int)m, d_planes, d_stats);
    s->timer.mark("end");
    HIP_TRY(hipGetLastError());
    const uint32_t *st = (const uint32_t *)s->rgb_pin.p;
    HIP_TRY(hipMemcpyAsync(s->rgb_pin.p, d_stats, st_b, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));                                               // the 3 m statistics, read back once
    // the plane modes (compressWSIPlane, wsicompress.go:373-421, as encode_level picks them): a unit per non-constant plane
    std::vector<mic_hip_unit> units;
    for (size_t q = 0; q < 3 * m; q++) {
        const RgbDesc &d = tab[q / 3];
        const uint32_t mn = st[2 * q], mx = ~st[2 * q + 1];
        if (mn != mx) units.push_back(mic_hip_unit{ d.plane_off + (q % 3) * rgb_stride((size_t)d.w * (size_t)d.h), d.w, d.h, (uint16_t)std::max<uint32_t>(mx, 255u), 2 });   // :398-402
    }
    std::vector<uint64_t> offs(units.size() + 1, 0); std::vector<int32_t> ust(units.size()), uns(units.size());
    const uint8_t *d_streams = nullptr;
    if (!units.empty()) {
        if ((rc = session_encode_enqueue(s, d_planes, units.data(), (int)units.size()))) return rc;
        if ((rc = session_encode_finish(s, &d_streams, offs.data(), ust.data(), uns.data()))) return rc;
    }
    std::vector<RgbAsm> recs;
    uint64_t off = pay0;
    for (size_t k = 0, u = 0; k < m; k++) {
        RgbImage &im = img[of[k]];
        const size_t npx = (size_t)im.w * (size_t)im.h;
        RgbAsm r{};
        r.dst = off; r.w = im.w; r.h = im.h; r.container = im.container ? 1u : 0u;
        uint64_t bytes = (im.container ? 12 : 0) + 12;
        for (size_t p = 0; p < 3; p++) {
            const size_t q = 3 * k + p;
            const uint32_t mn = st[2 * q], mx = ~st[2 * q + 1];
            if (mn == mx) { r.mode_value[p] = (mn == 0 ? 0u : 1u) | (mn << 8); bytes += mn == 0 ? 1 : 3; continue; }
            const int32_t us = ust[u];
            if (us == MIC_OK) { r.mode_value[p] = 2; r.src[p] = (uint64_t)(uintptr_t)d_streams + offs[u]; r.len[p] = (uint32_t)(offs[u + 1] - offs[u]); }
            else if (us == MIC_ERR_USE_RLE || us == MIC_ERR_INCOMPRESSIBLE) {                // raw fallback, :403-414
                r.mode_value[p] = 3; r.src[p] = (uint64_t)(uintptr_t)(d_planes + tab[k].plane_off + p * rgb_stride(npx)); r.len[p] = (uint32_t)(npx * 2);
            } else if (im.status == MIC_OK) { im.status = us; im.failed_plane = (int32_t)p; } // "Y plane: %w", :337-348: the first plane that fails
            bytes += 1 + (uint64_t)r.len[p];
            u++;
        }
        if (im.status != MIC_OK) continue;
        im.blob_off = off; im.blob_len = bytes;
        off += bytes;
        recs.push_back(r);
    }
    *pay_end = off;
    if (recs.empty()) return MIC_OK;
    if (pay0 == 0 && (rc = payload.reserve((size_t)off + 64))) return rc;
    if ((size_t)off > payload.cap) return MIC_ERR_INTERNAL;
    HIP_TRY(hipMemcpyAsync(d_recs, recs.data(), recs.size() * sizeof(RgbAsm), hipMemcpyHostToDevice, s->stream));
    s->timer.stream = s->stream; s->timer.mark("k_rgb_batch_assemble");
    hipLaunchKernelGGL(k_rgb_batch_assemble, dim3((unsigned)recs.size(), 3, 4), dim3(256), 0, s->stream, (const RgbAsm *)d_recs, (uint8_t *)payload.p);
    s->timer.mark("end");
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MIC_OK;
}

int rgb_decode_run(mic_hip_session *s, const uint8_t *d_blobs, RgbBlob *bl, int n, uint8_t *d_rgb_out) {
    if (n > kRgbMaxImages) return MIC_ERR_UNSUPPORTED;
    std::vector<RgbDesc> tab; std::vector<int> of; size_t plane_px = 0;
    int rc = rgb_table([&](int i, uint64_t &off, int32_t &w, int32_t &h) { off = bl[i].rgb_off; w = bl[i].w; h = bl[i].h; return bl[i].status == MIC_OK; }, n, tab, of, &plane_px);
    if (rc) return rc;
    const size_t m = tab.size();
    if (m == 0) return MIC_OK;
    if (!s->stream) HIP_TRY(mic_stream_create(&s->stream));
    std::vector<RgbFill> fills; std::vector<mic_hip_unit> units; std::vector<uint64_t> begins, ends; std::vector<size_t> unit_plane;
    for (size_t q = 0; q < 3 * m; q++) {
        const RgbDesc &d = tab[q / 3];
        const RgbBlob &b = bl[of[q / 3]];
        const RgbPlaneRec &pr = b.pl[q % 3];
        const size_t npx = (size_t)d.w * (size_t)d.h;
        const uint64_t poff = d.plane_off + (q % 3) * rgb_stride(npx);
        if (pr.mode == 2) { units.push_back(mic_hip_unit{ poff, d.w, d.h, 0, 0 }); begins.push_back(b.blob_off + pr.off); ends.push_back(b.blob_off + pr.off + pr.len); unit_plane.push_back(q); }
        else fills.push_back(RgbFill{ poff, b.blob_off + pr.off, (uint32_t)npx, (uint32_t)pr.mode | ((uint32_t)(pr.mode == 1 ? pr.value : 0) << 8) });
    }
    const size_t fill_b = align_up(fills.size() * sizeof(RgbFill), 64);
    if ((rc = s->rgb_planes.reserve(plane_px * 2 + 64)) || (rc = s->rgb_aux.reserve(fill_b + m * sizeof(RgbDesc) + 64))) return rc;
    uint16_t *d_planes = (uint16_t *)s->rgb_planes.p;
    RgbFill *d_fill = (RgbFill *)s->rgb_aux.p;
    RgbDesc *d_tab = (RgbDesc *)((char *)s->rgb_aux.p + fill_b);
    if (!fills.empty()) {
        HIP_TRY(hipMemcpyAsync(d_fill, fills.data(), fills.size() * sizeof(RgbFill), hipMemcpyHostToDevice, s->stream));
        s->timer.reset(s->stream); s->timer.mark("k_rgb_batch_fill");
        for (size_t f0 = 0; f0 < fills.size(); f0 += 65535)
            hipLaunchKernelGGL(k_rgb_batch_fill, dim3(8, (unsigned)std::min<size_t>(65535, fills.size() - f0)), dim3(256), 0, s->stream, d_planes, d_blobs, (const RgbFill *)d_fill + f0);
        s->timer.mark("end");
        HIP_TRY(hipGetLastError());
    }
    if (!units.empty()) {                                                                   // ONE unit decode over every mode-2 plane
        if ((rc = session_decode_enqueue_spans(s, d_blobs, begins.data(), ends.data(), units.data(), (int)units.size(), d_planes))) return rc;
        std::vector<int32_t> ust(units.size());
        if ((rc = session_decode_finish(s, ust.data()))) return rc;
        for (size_t u = 0; u < ust.size(); u++) {
            RgbBlob &b = bl[of[unit_plane[u] / 3]];
            if (ust[u] != MIC_OK && b.status == MIC_OK) { b.status = ust[u]; b.failed_plane = (int32_t)(unit_plane[u] % 3); }   // "Y plane: %w", :446-461
        }
    }
    // the images whose planes all stand: the table again without those a stream failed (the planes keep their places)
    std::vector<RgbDesc> good;
    uint64_t chunks = 0;
    for (size_t k = 0; k < m; k++) {
        if (bl[of[k]].status != MIC_OK) continue;
        RgbDesc d = tab[k];
        d.chunk0 = (uint32_t)chunks; chunks += ((size_t)d.w * (size_t)d.h + kRgbChunk - 1) / kRgbChunk;
        good.push_back(d);
    }
    if (!good.empty()) {
        HIP_TRY(hipMemcpyAsync(d_tab, good.data(), good.size() * sizeof(RgbDesc), hipMemcpyHostToDevice, s->stream));
        s->timer.stream = s->stream; s->timer.mark("k_rgb_batch_from_planes");
        hipLaunchKernelGGL(k_rgb_batch_from_planes, dim3((unsigned)chunks), dim3(256), 0, s->stream, (const uint16_t *)d_planes, (const RgbDesc *)d_tab, (int)good.size(), d_rgb_out);
        s->timer.mark("end");
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MIC_OK;
}

}  // namespace micapi

// ================================================================================ C ABI
extern "C" {

// debug probe (not part of the public header): 1 = k_rgb_batch_planes loads bytes one at a time, 0 = a group of four pixels as three
// dwords (what ships); tools/bench_rgb_batch.py measures both
int mic_hip_debug_rgb_planes_bytewise(int on) { g_rgb_bytewise.store(on ? 1 : 0); return MIC_OK; }

static int32_t rgb_image_args(const mic_hip_rgb_image &im) {
    if (im.width <= 0 || im.height <= 0) return MIC_ERR_ARGS;
    if ((size_t)im.width * (size_t)im.height > kRgbMaxPx) return MIC_ERR_UNSUPPORTED;
    return MIC_OK;
}

int mic_hip_session_rgb_encode(mic_hip_session *s, const uint8_t *d_rgb, const mic_hip_rgb_image *imgs, int n,
                               const uint8_t **d_blobs, uint64_t *h_offsets, int32_t *status, int32_t *failed_plane) try {
    if (!s || !d_rgb || !imgs || !d_blobs || !h_offsets || !status || n < 0) return MIC_ERR_ARGS;
    { const int arc = s->activate(); if (arc) return arc; }
    std::vector<RgbImage> img((size_t)n);
    uint64_t bound = 0;
    for (int i = 0; i < n; i++) {
        img[(size_t)i] = RgbImage{ imgs[i].rgb_off, imgs[i].width, imgs[i].height, 0, rgb_image_args(imgs[i]), -1, 0, 0 };
        if (img[(size_t)i].status == MIC_OK) bound += MIC_HIP_RGB_BOUND((size_t)imgs[i].width * (size_t)imgs[i].height);
    }
    auto npx = [&](int i) { return img[(size_t)i].status == MIC_OK ? (size_t)img[(size_t)i].w * (size_t)img[(size_t)i].h : (size_t)0; };
    int rc;
    uint64_t end = 0;
    for (int i0 = 0; i0 < n;) {
        const int i1 = rgb_next_cut(npx, i0, n, ~(size_t)0);
        if (i0 > 0 || i1 < n) { if ((rc = s->rgb_payload.reserve((size_t)bound + 64))) return rc; }   // several sub-batches write one buffer: reserved once, at its bound
        if ((rc = rgb_encode_run(s, d_rgb, img.data() + i0, i1 - i0, s->rgb_payload, (i0 > 0 || i1 < n) ? end : 0, &end))) return rc;
        i0 = i1;
    }
    uint64_t off = 0;
    for (int i = 0; i < n; i++) {
        const RgbImage &im = img[(size_t)i];
        h_offsets[i] = im.status == MIC_OK ? im.blob_off : off;
        off = h_offsets[i] + (im.status == MIC_OK ? im.blob_len : 0);
        status[i] = im.status;
        if (failed_plane) failed_plane[i] = im.failed_plane;
    }
    h_offsets[n] = off;
    *d_blobs = (const uint8_t *)s->rgb_payload.p;
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_session_rgb_decode(mic_hip_session *s, const uint8_t *d_blobs, const uint64_t *h_offsets,
                               const mic_hip_rgb_image *imgs, int n, uint8_t *d_rgb_out, int32_t *status, int32_t *failed_plane) try {
    if (!s || !d_blobs || !h_offsets || !imgs || !d_rgb_out || !status || n < 0) return MIC_ERR_ARGS;
    if (n == 0) return MIC_OK;
    { const int arc = s->activate(); if (arc) return arc; }
    for (int i = 0; i < n; i++) if (h_offsets[i + 1] < h_offsets[i]) return MIC_ERR_ARGS;
    if (!s->stream) HIP_TRY(mic_stream_create(&s->stream));
    // the blobs go device to device into the session's compressed-input buffer, which keeps the slack the decode kernels may read
    // past a stream's end (the caller's allocation owes them nothing); their heads come to the host in one copy
    const uint64_t b0 = h_offsets[0], total = h_offsets[n] - b0;
    const size_t offs_b = ((size_t)n + 1) * 8, head_b = (size_t)n * sizeof(RgbHead);
    int rc;
    if ((rc = s->io_comp.reserve((size_t)total + 64)) || (rc = s->rgb_aux.reserve(offs_b + head_b + 64)) || (rc = s->rgb_pin.reserve((offs_b + head_b) / 8 + 1))) return rc;
    uint64_t *h_rel = s->rgb_pin.p;
    for (int i = 0; i <= n; i++) h_rel[i] = h_offsets[i] - b0;
    RgbHead *h_heads = (RgbHead *)(s->rgb_pin.p + n + 1);
    uint64_t *d_offs = (uint64_t *)s->rgb_aux.p;
    RgbHead *d_heads = (RgbHead *)((char *)s->rgb_aux.p + offs_b);
    if (total) HIP_TRY(hipMemcpyAsync(s->io_comp.p, d_blobs + b0, (size_t)total, hipMemcpyDeviceToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(d_offs, h_rel, offs_b, hipMemcpyHostToDevice, s->stream));
    if ((rc = rgb_heads_enqueue(s->stream, (const uint8_t *)s->io_comp.p, d_offs, d_offs + 1, n, d_heads))) return rc;
    HIP_TRY(hipMemcpyAsync(h_heads, d_heads, head_b, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    std::vector<RgbBlob> bl((size_t)n);
    for (int i = 0; i < n; i++) {
        RgbBlob &b = bl[(size_t)i];
        b = RgbBlob{ h_rel[i], h_rel[i + 1] - h_rel[i], imgs[i].rgb_off, imgs[i].width, imgs[i].height, rgb_image_args(imgs[i]), -1, {} };
        if (b.status == MIC_OK) b.status = rgb_parse_head(h_heads[i], b.blob_len, (size_t)b.w * (size_t)b.h, b.pl, &b.failed_plane);
    }
    auto npx = [&](int i) { return bl[(size_t)i].status == MIC_OK ? (size_t)bl[(size_t)i].w * (size_t)bl[(size_t)i].h : (size_t)0; };
    for (int i0 = 0; i0 < n;) {
        const int i1 = rgb_next_cut(npx, i0, n, ~(size_t)0);
        if ((rc = rgb_decode_run(s, (const uint8_t *)s->io_comp.p, bl.data() + i0, i1 - i0, d_rgb_out))) return rc;
        i0 = i1;
    }
    for (int i = 0; i < n; i++) { status[i] = bl[(size_t)i].status; if (failed_plane) failed_plane[i] = bl[(size_t)i].failed_plane; }
    return MIC_OK;
} MIC_ABI_CATCH

}  // extern "C"
