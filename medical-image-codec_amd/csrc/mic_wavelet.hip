// mic_wavelet.hip -- WaveletV2 on the GPU (waveletu16.go, waveletfsecompressu16.go:303-534).
//
// WaveletV2{,SIMD}RLEFSECompressU16 = up to 8 levels of the Le Gall 5/3 integer lifting in Mallat
// layout -> subband scan -> zigzag (+ 3-word escape) -> RLE with length prefix -> 4-state FSE (no
// fallback) behind an 11-byte header.  The reference lifts in place, predict pass then update pass,
// rows then columns, AVX2 over 8-column blocks (wavelet_simd_amd64.s).  Here every output sample is
// written straight from the <= 5 input samples it depends on,
//     d[i] = x[2i+1] - ((x[2i] + x[2i+2]) >> 1)        s[i] = x[2i] + ((d[i-1] + d[i] + 2) >> 2)
// with the reference's boundary rules, so there is no serial dependence at all; a LEVEL is one kernel (k_wv_fwd2d / k_wv_inv2d:
// rows and columns over a tile in LDS, de-interleaving on the fly, the smooth plane handed from level to level in a scratch plane).
// The subband scan is a closed-form index map, so collect + zigzag + escape + max is one pass with a
// prefix sum for the rare escapes.  RLE / FSE reuse the unit-codec kernels (mode 2 / mode 1 units).
// Every launch is driven by tables (WvFrame, WvWork below): a launch chain takes frames of any shapes and level counts -- the
// one-shape entry points are callers with a table of equal rows (mic_hip_wavelet_v2_compress_jobs / _decompress_jobs: mic_host_io.hip).
// A chain still lays every unit out by its largest frame, in the tier-2 slabs; the cut rule of the
// host doors (wv_next_cut) bounds what that costs.
#include "mic_session.h"
#include "mic_staged.h"
#include "mic_wave.h"
#include "mic_rlewalk.h"

namespace {

#define WV_THREADS 1024
#define WV_WAVES 16

struct WvDims { int rows, cols, levels; int nr[9], nc[9]; };

__host__ __device__ inline WvDims wv_dims(int rows, int cols, int levels) {
    WvDims d; d.rows = rows; d.cols = cols; d.levels = levels;
    d.nr[0] = rows; d.nc[0] = cols;
    for (int l = 1; l <= 8; l++) { d.nr[l] = (d.nr[l - 1] + 1) / 2; d.nc[l] = (d.nc[l - 1] + 1) / 2; }
    return d;
}

// ---- table-driven geometry: frames of any shapes and level counts in one launch chain -------------------------------------------------
// A sub-batch's frames are described by one WvFrame each, uploaded with the unit descriptors (frame f <-> unit f).  Their planes lie
// back to back, with no padding to the largest frame: the u16 pixels px_off elements behind the launch's pixel pointer (a decode at
// `level`: the nr[level] x nc[level] band), the int32 coefficient plane (row stride = the frame's own cols) a_off elements into the
// session's wv_a, the two smooth planes of ll_half elements each b_off elements into wv_b -- the int32 offsets multiples of 4, so
// that the 16-byte accesses of the scan kernels keep the alignment a frame on its own has.
// A block finds its frame and tile with ONE load of a WvWork record the host builds per launch ("WaveletV2,
// mixed frames"): the grid of a launch is the sum of its frames' own tiles, and a frame takes part in a level launch only if it has
// that level.  The one-group kernels run group f on frame f and need no work records.
struct WvFrame {
    WvDims d;                       // rows, cols, the level count applied (the header's)
    int32_t level;                  // decode: the resolution wanted (0: the full image)
    uint32_t lim;                   // the scan positions wanted: nr[level] * nc[level] (rows * cols at level 0)
    uint32_t ll_half, pad[2];       // elements of one smooth plane: nr[1] * nc[1] rounded up to 4 (pad: no hole, the host compares records bytewise)
    uint64_t px_off, a_off, b_off;
};
struct WvWork { uint32_t frame, bx, by, pad; };
__device__ __forceinline__ WvWork wv_work(const WvWork *__restrict__ wk) {
    const uint4 v = *(const uint4 *)(wk + blockIdx.x);
    return WvWork{ v.x, v.y, v.z, v.w };
}

// ---- lifting, one output sample at a time (waveletu16.go:26-122) ---------------------------------
template <typename Get>
__device__ __forceinline__ int32_t wv_d(Get x, int n, int i) {           // detail i (0 <= i < n/2)
    const int32_t l = x(2 * i), r = (2 * i + 2 < n) ? x(2 * i + 2) : l;  // symmetric extension on the right
    return x(2 * i + 1) - ((l + r) >> 1);
}
template <typename Get>
__device__ __forceinline__ int32_t wv_s(Get x, int n, int i) {           // smooth i (0 <= i < (n+1)/2)
    int32_t d_right, d_left;
    if (2 * i + 1 < n) d_right = wv_d(x, n, i);
    else d_right = (i > 0) ? wv_d(x, n, i - 1) : 0;
    d_left = (i > 0) ? wv_d(x, n, i - 1) : d_right;
    return x(2 * i) + ((d_left + d_right + 2) >> 2);
}
// inverse: c(k) reads the Mallat-ordered line (low half first); returns sample k of the restored line
template <typename Get>
__device__ __forceinline__ int32_t wv_even(Get c, int n, int i) {        // x[2i]
    const int n_low = (n + 1) / 2;
    auto d = [&](int k) { return c(n_low + k); };
    int32_t d_right, d_left;
    if (2 * i + 1 < n) d_right = d(i);
    else d_right = (i > 0) ? d(i - 1) : 0;
    d_left = (i > 0) ? d(i - 1) : d_right;
    return c(i) - ((d_left + d_right + 2) >> 2);
}
template <typename Get>
__device__ __forceinline__ int32_t wv_sample(Get c, int n, int k) {
    if (n < 2) return c(k);
    const int n_low = (n + 1) / 2;
    if ((k & 1) == 0) return wv_even(c, n, k >> 1);
    const int i = k >> 1;
    const int32_t l = wv_even(c, n, i), r = (2 * i + 2 < n) ? wv_even(c, n, i + 1) : l;
    return c(n_low + i) + ((l + r) >> 1);
}

// inverse: columns first, then rows   (waveletu16.go:213-257); a thread restores samples 2i and 2i+1 of its line
template <typename Get>
__device__ __forceinline__ void wv_pair(Get cf, int n, int i, int32_t &ev, int32_t &od) {
    if (n < 2) { ev = cf(0); od = 0; return; }
    const int n_low = (n + 1) / 2;
    ev = wv_even(cf, n, i);
    od = 0;
    if (2 * i + 1 < n) { const int32_t rr = (2 * i + 2 < n) ? wv_even(cf, n, i + 1) : ev; od = cf(n_low + i) + ((ev + rr) >> 1); }
}
// ---- one level of the transform in ONE pass, no LDS ------------------------------------------------------------------------------
// A lane owns one column PAIR (samples 2 gi, 2 gi + 1 of every row) and walks down a strip of rows.  The rows pass of a row needs
// the neighbour lanes' samples only -- x[2 gi + 2] from the lane to the right, d[gi - 1] from the lane to the left: two DPP wave
// shifts -- and the columns pass is a window of three rows of the rows pass's output that slides down the lane's registers.  A wave
// covers 64 pairs and writes 62 (one pair of context on either side), a strip is WS_ROWS output rows (+ one pair of rows of
// context at its top); every access is a run of 256 bytes (128 for 16-bit pixels) per wave, the addresses advance by a stride a row.
// (Rounds 2-3: rows and columns over a 64 x 16 tile in LDS -- one pass over memory as well, 9 N bytes a transform, but ~100
// instructions of tile index arithmetic per sample: 4.9 + 6.4 ms for 256 CR frames both ways where the memory traffic is ~4.)
// The detail subbands go to their Mallat places in `a` (row stride `stride`); the smooth subband -- the next level's input -- goes to
// a compact scratch plane (`ll`, row stride = its width), except the last level's, which goes to the top-left corner of `a`:
// nothing is read and written in the same buffer by one launch.
#define WS_ROWS 64
#define WS_LANES 62                 // pairs a wave writes
template <int CTRL> __device__ __forceinline__ int32_t wv_shift(int32_t v) {    // 0x130: from the lane to the right, 0x138: from the lane to the left
    return (int32_t)mic_dpp<CTRL>(0u, (uint32_t)v);
}
typedef uint32_t wv_u32u __attribute__((aligned(2)));
typedef unsigned long long wv_u64u __attribute__((aligned(4)));

// Level l of the frames a launch's work records name: src16 = the launch's pixels (level 0), A / B = the session's planes.
template <bool FROM_U16>
__global__ void __launch_bounds__(256) k_wv_fwd2d(const WvFrame *__restrict__ ft, const WvWork *__restrict__ wk, const uint16_t *__restrict__ src16,
                                                  int32_t *__restrict__ A, int32_t *__restrict__ B, int l) {
    const WvWork wr = wv_work(wk);
    const WvFrame &fr = ft[wr.frame];
    const int r = fr.d.nr[l], c = fr.d.nc[l];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int nlc = (c + 1) / 2, nlr = (r + 1) / 2;
    const int gi = ((int)wr.bx * 4 + wave) * WS_LANES - 1 + lane;               // this lane's pair (lanes 0 and 63: context only)
    const int gp0 = (int)wr.by * WS_ROWS, gp1 = min(gp0 + WS_ROWS, nlr);
    if (((int)wr.bx * 4 + wave) * WS_LANES >= nlc) return;
    // level l reads the pixels (l = 0) or the smooth plane of parity l - 1; its own smooth plane has parity l, the last level's goes to `a`
    const bool last = l == fr.d.levels - 1;
    int32_t *const a = A + fr.a_off, *const bf = B + fr.b_off;
    const int stride = fr.d.cols, sstride = c;
    const void *const src_ = FROM_U16 ? (const void *)(src16 + fr.px_off) : (const void *)(bf + (((l - 1) & 1) ? fr.ll_half : 0u));
    int32_t *const ll = last ? a : bf + ((l & 1) ? fr.ll_half : 0u);
    const int llstride = last ? stride : nlc;
    const bool has0 = gi >= 0 && 2 * gi < c, has1 = gi >= 0 && 2 * gi + 1 < c, hasr = 2 * gi + 2 < c, left = gi > 0;
    const bool out_lo = lane >= 1 && lane <= WS_LANES && has0, out_hi = lane >= 1 && lane <= WS_LANES && has1;
    // input row y: this lane's two samples ...
    auto fetch = [&](int y, int32_t &x0, int32_t &x1) {
        x0 = 0; x1 = 0;
        const size_t o = (size_t)y * sstride + (size_t)(2 * gi);
        if (FROM_U16) {
            const uint16_t *p = (const uint16_t *)src_ + o;
            if (has1) { const uint32_t w = *(const wv_u32u *)p; x0 = (int32_t)(w & 0xFFFFu); x1 = (int32_t)(w >> 16); }
            else if (has0) x0 = (int32_t)p[0];
        } else {
            const int32_t *p = (const int32_t *)src_ + o;
            if (has1) { const unsigned long long w = *(const wv_u64u *)p; x0 = (int32_t)(uint32_t)w; x1 = (int32_t)(uint32_t)(w >> 32); }
            else if (has0) x0 = p[0];
        }
    };
    // ... and its rows pass (waveletu16.go:26-74, :170-182): smooth and detail of the pair
    auto lift = [&](int32_t x0, int32_t x1, int32_t &lo, int32_t &hi) {
        const int32_t xn = wv_shift<0x130>(x0), xr = hasr ? xn : x0;       // symmetric extension on the right
        const int32_t d = x1 - ((x0 + xr) >> 1);
        const int32_t dp = wv_shift<0x138>(d);
        const int32_t dr = has1 ? d : (left ? dp : 0), dl = left ? dp : dr;
        lo = x0 + ((dl + dr + 2) >> 2); hi = d;
    };
    auto row = [&](int y, int32_t &lo, int32_t &hi) { int32_t x0, x1; fetch(y, x0, x1); lift(x0, x1, lo, hi); };
    // the columns pass (:183-208) down the strip: rows 2 gp, 2 gp + 1 in (l0, h0), (l1, h1); row 2 gp + 2 in (ln, hn)
    int32_t l0, h0, l1 = 0, h1 = 0, ln = 0, hn = 0, dlo = 0, dhi = 0;       // dlo, dhi: the details of pair-row gp - 1
    if (gp0 > 0) {
        int32_t pl0, ph0, pl1, ph1;
        row(2 * gp0 - 2, pl0, ph0); row(2 * gp0 - 1, pl1, ph1); row(2 * gp0, l0, h0);
        dlo = pl1 - ((pl0 + l0) >> 1); dhi = ph1 - ((ph0 + h0) >> 1);
    } else row(0, l0, h0);
    if (2 * gp0 + 1 < r) row(2 * gp0 + 1, l1, h1);
    for (int gp = gp0; gp < gp1; gp++) {
        const bool odd = 2 * gp + 1 < r, more = 2 * gp + 2 < r, more1 = 2 * gp + 3 < r;
        int32_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;                              // (both rows of the next pair are fetched before either is used)
        if (more) fetch(2 * gp + 2, a0, a1);
        if (more1) fetch(2 * gp + 3, b0, b1);
        if (more) lift(a0, a1, ln, hn);
        const int32_t rl = more ? ln : l0, rh = more ? hn : h0;
        const int32_t d_l = l1 - ((l0 + rl) >> 1), d_h = h1 - ((h0 + rh) >> 1);
        const int32_t drl = odd ? d_l : (gp > 0 ? dlo : 0), drh = odd ? d_h : (gp > 0 ? dhi : 0);
        const int32_t dll = gp > 0 ? dlo : drl, dlh = gp > 0 ? dhi : drh;
        const int32_t s_l = l0 + ((dll + drl + 2) >> 2), s_h = h0 + ((dlh + drh + 2) >> 2);
        if (out_lo) ll[(size_t)gp * llstride + gi] = s_l;
        if (out_hi) a[(size_t)gp * stride + nlc + gi] = s_h;
        if (odd) {
            if (out_lo) a[(size_t)(nlr + gp) * stride + gi] = d_l;
            if (out_hi) a[(size_t)(nlr + gp) * stride + nlc + gi] = d_h;
        }
        dlo = d_l; dhi = d_h; l0 = ln; h0 = hn;
        if (more1) lift(b0, b1, l1, h1);
    }
}
// The inverse of one level (columns, then rows: waveletu16.go:213-257): the smooth subband from `ll` (the level below wrote it; the
// coarsest level's lies in `a`), the detail subbands from `a`, the restored region to `dst` (a compact plane, or the 16-bit pixels).
// A lane owns smooth column gi and detail column gi of the Mallat layout -- after the rows pass, samples 2 gi and 2 gi + 1.
// SAT (with TO_U16): the samples are saturated to [0, 65535] -- the last level of a reduced-resolution decode, whose LL band may
// over- or undershoot the pixel range at edges; the full decode's store keeps the reference's plain truncation.
template <bool TO_U16, bool SAT = false>
__global__ void __launch_bounds__(256) k_wv_inv2d(const WvFrame *__restrict__ ft, const WvWork *__restrict__ wk, const int32_t *__restrict__ A, int32_t *__restrict__ B,
                                                  uint16_t *__restrict__ dst16, int l) {
    const WvWork wr = wv_work(wk);
    const WvFrame &fr = ft[wr.frame];
    const int r = fr.d.nr[l], c = fr.d.nc[l];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int nlc = (c + 1) / 2, nlr = (r + 1) / 2;
    const int gi = ((int)wr.bx * 4 + wave) * WS_LANES - 1 + lane;
    const int gp0 = (int)wr.by * WS_ROWS, gp1 = min(gp0 + WS_ROWS, nlr);
    if (((int)wr.bx * 4 + wave) * WS_LANES >= nlc) return;
    // level l reads the smooth plane of parity l + 1 (the coarsest level's lies in `a`) and restores into the plane of parity l --
    // or into the pixels: level 0, or level `level` of a reduced decode (SAT); either way a compact plane of this level's width
    const bool coarsest = l == fr.d.levels - 1;
    const int stride = fr.d.cols;
    const int32_t *const af = A + fr.a_off;
    const int32_t *const lf = coarsest ? af : B + fr.b_off + (((l + 1) & 1) ? fr.ll_half : 0u);
    const int llstride = coarsest ? stride : nlc;
    void *const dst_ = TO_U16 ? (void *)(dst16 + fr.px_off) : (void *)(B + fr.b_off + ((l & 1) ? fr.ll_half : 0u));
    const int dstride = c;
    const bool has0 = gi >= 0 && 2 * gi < c, has1 = gi >= 0 && 2 * gi + 1 < c, hasr = 2 * gi + 2 < c, left = gi > 0;
    const bool out0 = lane >= 1 && lane <= WS_LANES && has0;
    // Mallat row j of this lane's two columns: smooth rows j < nlr, detail rows nlr + j
    auto smooth = [&](int j, int32_t &vs, int32_t &vd) {
        vs = has0 ? lf[(size_t)j * llstride + gi] : 0;
        vd = has1 ? af[(size_t)j * stride + nlc + gi] : 0;
    };
    auto detail = [&](int j, int32_t &vs, int32_t &vd) {
        vs = has0 ? af[(size_t)(nlr + j) * stride + gi] : 0;
        vd = has1 ? af[(size_t)(nlr + j) * stride + nlc + gi] : 0;
    };
    // even sample j of a column from its smooth value and the details on either side (wv_even's rules)
    auto even = [&](int j, int32_t cs, int32_t dm, int32_t d0) -> int32_t {
        const int32_t dr = (2 * j + 1 < r) ? d0 : (j > 0 ? dm : 0), dl = j > 0 ? dm : dr;
        return cs - ((dl + dr + 2) >> 2);
    };
    // one restored row of the columns pass through the rows pass, to `dst`
    auto put = [&](int y, int32_t vs, int32_t vd) {
        const int32_t dp = wv_shift<0x138>(vd);
        const int32_t dr = has1 ? vd : (left ? dp : 0), dl = left ? dp : dr;
        const int32_t ev = vs - ((dl + dr + 2) >> 2);
        const int32_t en = wv_shift<0x130>(ev);
        const int32_t od = vd + ((ev + (hasr ? en : ev)) >> 1);
        if (!out0) return;
        const size_t o = (size_t)y * dstride + (size_t)(2 * gi);
        if (TO_U16) {
            uint16_t *d = (uint16_t *)dst_ + o;
            const int32_t e16 = SAT ? min(max(ev, 0), 65535) : ev, o16 = SAT ? min(max(od, 0), 65535) : od;
            if (SAT) { if (has1) *(wv_u32u *)d = (uint32_t)e16 | ((uint32_t)o16 << 16); else d[0] = (uint16_t)e16; }
            else if (has1) *(wv_u32u *)d = ((uint32_t)ev & 0xFFFFu) | ((uint32_t)od << 16); else d[0] = (uint16_t)ev;
        } else {
            int32_t *d = (int32_t *)dst_ + o;
            if (has1) *(wv_u64u *)d = (uint32_t)ev | ((unsigned long long)(uint32_t)od << 32); else d[0] = ev;
        }
    };
    // the columns pass down the strip: (es, ed) = even sample gp of the two columns, (ds, dd) = their details gp
    int32_t ss, sd, ds = 0, dd = 0, pms = 0, pmd = 0;
    if (gp0 > 0) detail(gp0 - 1, pms, pmd);
    smooth(gp0, ss, sd);
    if (2 * gp0 + 1 < r) detail(gp0, ds, dd);
    int32_t es = even(gp0, ss, pms, ds), ed = even(gp0, sd, pmd, dd);
    for (int gp = gp0; gp < gp1; gp++) {
        const bool odd = 2 * gp + 1 < r, more = 2 * gp + 2 < r;
        int32_t ns = 0, nd = 0, nds = 0, ndd = 0, es1 = es, ed1 = ed;
        if (more) {
            smooth(gp + 1, ns, nd);
            if (2 * gp + 3 < r) detail(gp + 1, nds, ndd);
            es1 = even(gp + 1, ns, ds, nds); ed1 = even(gp + 1, nd, dd, ndd);
        }
        put(2 * gp, es, ed);
        if (odd) put(2 * gp + 1, ds + ((es + es1) >> 1), dd + ((ed + ed1) >> 1));
        es = es1; ed = ed1; ds = nds; dd = ndd;
    }
}
// The frames without a level (a side below 2: applied == 0) and the coarsest LL band of a reduced decode at level == levels, which
// runs no inverse level at all: a work record is WV_CHUNK consecutive elements of its frame (bx: which).
#define WV_CHUNK 4096u
__global__ void __launch_bounds__(256) k_wv_load(const WvFrame *__restrict__ ft, const WvWork *__restrict__ wk, const uint16_t *__restrict__ px, int32_t *__restrict__ A) {
    const WvWork wr = wv_work(wk);
    const WvFrame &fr = ft[wr.frame];
    const uint32_t n = (uint32_t)fr.d.rows * (uint32_t)fr.d.cols, i1 = min(n, (wr.bx + 1) * WV_CHUNK);
    for (uint32_t i = wr.bx * WV_CHUNK + threadIdx.x; i < i1; i += 256) A[fr.a_off + i] = (int32_t)px[fr.px_off + i];
}
__global__ void __launch_bounds__(256) k_wv_store(const WvFrame *__restrict__ ft, const WvWork *__restrict__ wk, const int32_t *__restrict__ A, uint16_t *__restrict__ px) {
    const WvWork wr = wv_work(wk);
    const WvFrame &fr = ft[wr.frame];
    const uint32_t n = (uint32_t)fr.d.rows * (uint32_t)fr.d.cols, i1 = min(n, (wr.bx + 1) * WV_CHUNK);
    for (uint32_t i = wr.bx * WV_CHUNK + threadIdx.x; i < i1; i += 256) px[fr.px_off + i] = (uint16_t)A[fr.a_off + i];
}
// the band (nr x nc at the top left of the frame's coefficient plane, row stride cols) saturated to u16, row stride nc
__global__ void __launch_bounds__(256) k_wv_band(const WvFrame *__restrict__ ft, const WvWork *__restrict__ wk, const int32_t *__restrict__ A, uint16_t *__restrict__ px) {
    const WvWork wr = wv_work(wk);
    const WvFrame &fr = ft[wr.frame];
    const uint32_t nc = (uint32_t)fr.d.nc[fr.level], cols = (uint32_t)fr.d.cols, i1 = min(fr.lim, (wr.bx + 1) * WV_CHUNK);
    for (uint32_t i = wr.bx * WV_CHUNK + threadIdx.x; i < i1; i += 256) {
        const uint32_t y = i / nc, x = i - y * nc;
        px[fr.px_off + i] = (uint16_t)min(max(A[fr.a_off + (size_t)y * cols + x], 0), 65535);
    }
}

// collectSubbandOrder / scatterSubbandOrder as an index map (waveletfsecompressu16.go:202-282):
// linear position p -> element offset y*cols + x.  LL of the coarsest level, then HL, LH, HH from the
// coarsest level to the finest.
__device__ __forceinline__ size_t wv_pos_to_index(const WvDims &d, size_t p) {
    const int L = d.levels;
    size_t sz = (size_t)d.nr[L] * d.nc[L];
    if (p < sz) return (p / d.nc[L]) * d.cols + (p % d.nc[L]);
    p -= sz;
    for (int l = L; l >= 1; l--) {
        const int hw = d.nc[l - 1] - d.nc[l], lh = d.nr[l - 1] - d.nr[l];
        sz = (size_t)d.nr[l] * hw;                                                        // HL: rows [0,nr[l]), cols [nc[l],nc[l-1])
        if (p < sz) return (p / hw) * d.cols + d.nc[l] + (p % hw);
        p -= sz;
        sz = (size_t)lh * d.nc[l];                                                        // LH: rows [nr[l],nr[l-1]), cols [0,nc[l])
        if (p < sz) return (d.nr[l] + p / d.nc[l]) * d.cols + (p % d.nc[l]);
        p -= sz;
        sz = (size_t)lh * hw;                                                             // HH
        if (p < sz) return (d.nr[l] + p / hw) * d.cols + d.nc[l] + (p % hw);
        p -= sz;
    }
    return 0;
}

// subband scan + waveletCoeffsToU16 (:28-40) + zzMax (:335-349).  One work-group per image; writes the
// symbol stream into u.sym, its length into u.nsym and the RLE maxValue into u.max_value.
__global__ void __launch_bounds__(WV_THREADS) k_wv_symbols(MicUnit *units, const WvFrame *__restrict__ ft, const int32_t *a) {
    MicUnit &u = units[blockIdx.x];
    if (!u.wv_slow) return;                                               // k_wv_symbols_par did this frame
    const WvDims &d = ft[blockIdx.x].d;
    a += ft[blockIdx.x].a_off;                                            // one group per frame of the batch
    __shared__ uint32_t s_scan[WV_WAVES], s_max[WV_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n = (size_t)d.rows * d.cols;
    uint16_t *sym = u.sym; const uint32_t cap = u.sym_cap;
    uint32_t carry = 0, zmax = 0; bool ovf = false;
    for (size_t base = 0; base < n; base += WV_THREADS) {
        const size_t p = base + tid;
        int32_t v = 0; uint32_t cnt = 0;
        if (p < n) { v = a[wv_pos_to_index(d, p)]; cnt = (v >= -32767 && v <= 32767) ? 1u : 3u; }
        __syncthreads();
        uint32_t tot;
        const uint32_t o = carry + mic_group_excl_add<WV_WAVES>(cnt, s_scan, &tot);
        if (cnt == 1) {
            const uint32_t z = (uint32_t)((v >> 31) ^ (int32_t)((uint32_t)v << 1)) & 0xFFFF;   // zigzagEncode16, :538-541
            if (o < cap) sym[o] = (uint16_t)z; else ovf = true;
            zmax = max(zmax, z);
        } else if (cnt == 3) {
            if (o + 2 < cap) { sym[o] = 65535; sym[o + 1] = (uint16_t)((uint32_t)v >> 16); sym[o + 2] = (uint16_t)(uint32_t)v; } else ovf = true;
            zmax = 65535;
        }
        carry += tot;
    }
    zmax = mic_wave_reduce_max(zmax);
    __syncthreads();
    if (lane == 0) s_max[wave] = zmax;
    const int any_ovf = __syncthreads_or(ovf ? 1 : 0);
    if (tid == 0) {
        uint32_t m = 0;
        for (int w = 0; w < WV_WAVES; w++) m = max(m, s_max[w]);
        int depth = m ? 32 - __clz(m) : 0;
        if (depth < 1) depth = 1;                                                         // :345-348
        u.max_value = (uint16_t)((1u << depth) - 1);
        u.nsym = carry;
        u.status = any_ovf ? MICD_ERR_CAPACITY : MICD_OK;
    }
}

// tokens -> symbols: RleDecompressU16.Init + Decompress (rledecompressu16.go:21-30, :87-97); header walk by
// wave 0, expansion by all waves (as in mic_decode_px.hip), length taken from the two prefix words.
// One work-group per unit; mode_filter >= 0 restricts the launch to units of that mode (MIC2 temporal residuals).
__global__ void __launch_bounds__(WV_THREADS) k_wv_expand(MicUnit *units, int mode_filter, int only_slow) {
    MicUnit &u = units[blockIdx.x];
    if (mode_filter >= 0 && u.mode != (uint32_t)mode_filter) return;
    if (only_slow && !u.wv_slow) return;                                  // k_wv_scatter did this frame
    if (u.status != MICD_OK) return;
    __shared__ uint32_t s_misc[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t ntok = u.ntok; const uint16_t *tok = u.tok;
    if (ntok < 3) { if (tid == 0) u.status = MICD_ERR_CORRUPT; return; }
    const bool pre = mic_is_prefix(u);                                   // the tokens end at the chain's ceiling, not at the stream's end
    uint32_t mid;
    if (!mic_rle_mid(tok[0], mid)) { if (tid == 0) u.status = MICD_ERR_CORRUPT; return; }
    uint32_t outlen = ((uint32_t)tok[1] << 16) + tok[2];
    if (outlen > u.sym_cap) { if (tid == 0) u.status = MICD_ERR_CORRUPT; return; }
    uint2 *seg = u.seg; uint16_t *sym = u.sym;
    if (wave == 0) {
        uint32_t pos = 3, outp = 0, nseg = 0, err = 0, fin = 0;
        const uint32_t segcap = u.seg_cap;
        while (pos < ntok && outp < outlen && !err && !fin) {
            const uint32_t w = (pos + lane < ntok) ? tok[pos + lane] : 0u;
            uint32_t j = 0;
            while (j < 64 && pos + j < ntok && outp < outlen) {
                uint32_t h = __builtin_amdgcn_readlane(w, (int)j);
                if (nseg >= segcap) { err = 1; break; }
                if (h == 0) h = 65536u;                                  // the reference's reading of a zero count: a literal chunk of 65536 - midCount (mic_decode_px.hip)
                const MicRleHdr hd = mic_rle_hdr(h, mid);
                if (hd.run) {
                    if (pos + j + 1 >= ntok) { if (pre) fin = 1; else err = 1; break; }   // (a prefix: the run's value lies behind it)
                    if (j == 63) break;
                }
                if (lane == 0) seg[nseg] = make_uint2(pos + j, outp);     // (this kernel's own records: the HEADER's token)
                nseg++; outp += hd.len; j += hd.adv;
            }
            pos += j;
        }
        if (outp < outlen && !pre) err = 1;                            // tokens ran out (Go: index panic)
        // the words the tokens cover: a prefix's last literal chunk may reach past its last token (pos: the header behind that chunk)
        const uint32_t cover = pre ? min(outlen, outp - (pos > ntok ? pos - ntok : 0u)) : outlen;
        if (lane == 0) { s_misc[0] = nseg; s_misc[1] = err; s_misc[2] = cover; }
    }
    __syncthreads();
    if (s_misc[1]) { if (tid == 0) u.status = MICD_ERR_CORRUPT; return; }
    const uint32_t nseg = s_misc[0];
    outlen = s_misc[2];                                                  // (a prefix: the words it covers)
    uint32_t bad = 0;
    for (uint32_t si = wave; si < nseg; si += WV_WAVES) {
        const uint2 r = seg[si];
        uint32_t h = tok[r.x];
        if (h == 0) h = 65536u;                                          // (a zero count: see the walker above)
        const MicRleHdr hd = mic_rle_hdr(h, mid);
        if (hd.run) {
            const uint16_t v = tok[r.x + 1];
            for (uint32_t k = lane; k < hd.len && r.y + k < outlen; k += 64) sym[r.y + k] = v;
        } else {
            const uint32_t cnt = hd.len;
            for (uint32_t k = lane; k < cnt && r.y + k < outlen; k += 64) { if (r.x + 1 + k < ntok) sym[r.y + k] = tok[r.x + 1 + k]; else bad = 1; }
        }
    }
    if (__syncthreads_or((int)bad)) { if (tid == 0) u.status = MICD_ERR_CORRUPT; return; }
    if (tid == 0) u.nsym = outlen;
}

// u16ToWaveletCoeffs (:43-58) + scatterSubbandOrder (:244-282): symbol stream -> Mallat image.
// A symbol is an escape marker iff it is 65535 and not one of the two payload words of a previous
// marker; with three-word escapes that is a 3-state recurrence, scanned as function composition.
__device__ __forceinline__ uint32_t wv_fn_compose(uint32_t g, uint32_t f) {      // functions on {0,1,2}, 2 bits per value
    const uint32_t f0 = f & 3, f1 = (f >> 2) & 3, f2 = (f >> 4) & 3;
    return ((g >> (2 * f0)) & 3) | (((g >> (2 * f1)) & 3) << 2) | (((g >> (2 * f2)) & 3) << 4);
}
// lim (the frame's): the coefficients wanted -- n, or P(r) of a decode at reduced resolution (the first P(r) of the subband scan); fewer is an error
__global__ void __launch_bounds__(WV_THREADS) k_wv_coeffs(MicUnit *units, const WvFrame *__restrict__ ft, int32_t *a) {
    MicUnit &u = units[blockIdx.x];
    const WvDims &d = ft[blockIdx.x].d;
    const uint32_t lim = ft[blockIdx.x].lim;
    a += ft[blockIdx.x].a_off;
    if (u.status != MICD_OK || !u.wv_slow) return;
    __shared__ uint32_t s_scan[WV_WAVES], s_fn[WV_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t m = u.nsym; const uint16_t *sym = u.sym;
    // state = payload words still to skip (0: a symbol starts here).  marker: 0 -> 2; payload: k -> k-1.
    // non-escape symbol: f = (0, 0, 1) i.e. state 0 -> 0, 1 -> 0, 2 -> 1 ; escape value 65535: f = (2, 0, 1)
    uint32_t carry_state = 0, carry_n = 0; bool bad = false;
    for (uint32_t base = 0; base < m && carry_n < lim; base += WV_THREADS) {
        const uint32_t i = base + tid;
        const bool in = i < m;
        const uint32_t x = in ? sym[i] : 0u;
        const uint32_t f = mic_wave_incl_scan((x == 65535u && in) ? (2u | (0u << 2) | (1u << 4)) : (0u | (0u << 2) | (1u << 4)), lane,
                                              [](uint32_t earlier, uint32_t later) { return wv_fn_compose(later, earlier); });
        __syncthreads();
        if (lane == 63) s_fn[wave] = f;
        __syncthreads();
        uint32_t st_in = carry_state;
        for (uint32_t w = 0; w < wave; w++) st_in = (s_fn[w] >> (2 * st_in)) & 3;
        const uint32_t st_after = (f >> (2 * st_in)) & 3;                          // state after symbol i
        uint32_t st_before = __shfl_up(st_after, 1); if (lane == 0) st_before = st_in;
        const bool starts = in && st_before == 0;                                  // a coefficient begins at i
        uint32_t tot, st_end = carry_state;
        const uint32_t before = mic_group_excl_add<WV_WAVES>(starts ? 1u : 0u, s_scan, &tot);
#pragma unroll
        for (int w = 0; w < WV_WAVES; w++) st_end = (s_fn[w] >> (2 * st_end)) & 3;
        if (starts) {
            const size_t k = (size_t)carry_n + before;
            if (k < lim) {
                int32_t v;
                if (x != 65535u) v = (int32_t)((x >> 1) ^ (uint32_t)(-(int32_t)(x & 1)));        // zigzagDecode16, :543-546
                else if (i + 2 < m) v = (int32_t)(((uint32_t)sym[i + 1] << 16) | (uint32_t)sym[i + 2]);
                else { v = 0; bad = true; }
                a[wv_pos_to_index(d, k)] = v;
            }
        }
        carry_n += tot; carry_state = st_end;
    }
    const int anybad = __syncthreads_or(bad ? 1 : 0);
    if (tid == 0 && (anybad || carry_n < lim)) u.status = MICD_ERR_CORRUPT;        // fewer coefficients than pixels (Go: panic)
}

// ---- the usual case in parallel: frames whose coefficients all fit 16 bits (no 3-word escapes), many groups per frame -------------
// Scan position p -> element offset, with the count of positions from p to the end of its subband row (they are consecutive
// in memory): 32-bit arithmetic (a frame has at most 2^27 samples).
__device__ __forceinline__ void wv_pos_row(const WvDims &d, uint32_t p, uint32_t &idx, uint32_t &left) {
    const int L = d.levels;
    const uint32_t cols = (uint32_t)d.cols;
    {
        const uint32_t w = (uint32_t)d.nc[L], sz = (uint32_t)d.nr[L] * w;
        if (p < sz) { const uint32_t y = p / w, x = p - y * w; idx = y * cols + x; left = w - x; return; }
        p -= sz;
    }
    for (int l = L; l >= 1; l--) {
        const uint32_t nc = (uint32_t)d.nc[l], nr = (uint32_t)d.nr[l], hw = (uint32_t)d.nc[l - 1] - nc, lh = (uint32_t)d.nr[l - 1] - nr;
        uint32_t sz = nr * hw;
        if (p < sz) { const uint32_t y = p / hw, x = p - y * hw; idx = y * cols + nc + x; left = hw - x; return; }
        p -= sz;
        sz = lh * nc;
        if (p < sz) { const uint32_t y = p / nc, x = p - y * nc; idx = (nr + y) * cols + x; left = nc - x; return; }
        p -= sz;
        sz = lh * hw;
        if (p < sz) { const uint32_t y = p / hw, x = p - y * hw; idx = (nr + y) * cols + nc + x; left = hw - x; return; }
        p -= sz;
    }
    idx = 0; left = 1;
}
#define WS_T 8192                                  // scan positions per group (a power of two: >> 13 below)
typedef uint32_t wv_v4 __attribute__((ext_vector_type(4)));
typedef wv_v4 WvQ2 __attribute__((aligned(2)));
typedef wv_v4 WvQ4 __attribute__((aligned(4)));
// subband scan + zigzag, WS_T positions per group (a work record: frame, bx = position tile).  A coefficient outside 16 bits sends the
// frame to k_wv_symbols (wv_slow); the frame's largest symbol is gathered with an atomic max.
__global__ void __launch_bounds__(1024) k_wv_symbols_par(MicUnit *units, const WvFrame *__restrict__ ft, const WvWork *__restrict__ wk, const int32_t *a) {
    const WvWork wr = wv_work(wk);
    const WvDims &d = ft[wr.frame].d;
    const uint32_t n = (uint32_t)d.rows * (uint32_t)d.cols, tid = threadIdx.x, lane = tid & 63;
    const uint32_t i0 = wr.bx * WS_T + tid * 8;
    MicUnit &u = units[wr.frame];
    const int32_t *af = a + ft[wr.frame].a_off;
    uint32_t w8[4] = { 0u, 0u, 0u, 0u }, zmax = 0, idx = 0, left = 0; bool wide = false;
    int32_t v8[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (i0 < n) wv_pos_row(d, i0, idx, left);
    if (i0 + 8 <= n && left >= 8) {                                    // the usual case: eight positions inside one subband row
        const wv_v4 lo = *(const WvQ4 *)(af + idx), hi = *(const WvQ4 *)(af + idx + 4);
        v8[0] = (int32_t)lo.x; v8[1] = (int32_t)lo.y; v8[2] = (int32_t)lo.z; v8[3] = (int32_t)lo.w;
        v8[4] = (int32_t)hi.x; v8[5] = (int32_t)hi.y; v8[6] = (int32_t)hi.z; v8[7] = (int32_t)hi.w;
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t p = i0 + (uint32_t)k;
            if (p < n) {
                if (left == 0) wv_pos_row(d, p, idx, left);
                v8[k] = af[idx]; idx++; left--;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int32_t v = v8[k];
        if (v < -32767 || v > 32767) wide = true;
        const uint32_t z = (uint32_t)((v >> 31) ^ (int32_t)((uint32_t)v << 1)) & 0xFFFF;   // zigzagEncode16, :538-541
        zmax = max(zmax, z);
        w8[k >> 1] |= z << (16 * (k & 1));
    }
    uint16_t *sym = u.sym;
    if (i0 + 8 <= n) { wv_v4 v; v.x = w8[0]; v.y = w8[1]; v.z = w8[2]; v.w = w8[3]; *(wv_v4 *)(sym + i0) = v; }   // (256-byte aligned slab, i0 a multiple of 8)
    else for (int k = 0; k < 8; k++) if (i0 + (uint32_t)k < n) sym[i0 + k] = (uint16_t)(w8[k >> 1] >> (16 * (k & 1)));
    zmax = mic_wave_reduce_max(zmax);
    // (one address per frame: an atomic per wave was 59 k atomics in a row on it.  The maximum only grows, so a wave whose own is
    // not above what the frame has already -- nearly every wave after the first few -- has nothing to say; a stale read only costs
    // an atomic that changes nothing)
    if (lane == 0 && zmax > __hip_atomic_load(&u.wv_zmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&u.wv_zmax, zmax);
    if (wide) u.wv_slow = 1;
}
// zzMax (:335-349) of the frames k_wv_symbols_par finished
__global__ void __launch_bounds__(256) k_wv_symbols_fin(MicUnit *units, const WvFrame *__restrict__ ft, int nf) {
    const int f = (int)(blockIdx.x * 256 + threadIdx.x);
    if (f >= nf) return;
    MicUnit &u = units[f];
    if (u.wv_slow) return;
    const uint32_t m = u.wv_zmax;
    int depth = m ? 32 - __clz(m) : 0;
    if (depth < 1) depth = 1;
    u.max_value = (uint16_t)((1u << depth) - 1);
    u.nsym = (uint32_t)ft[f].d.rows * (uint32_t)ft[f].d.cols;
    u.status = (u.nsym <= u.sym_cap) ? MICD_OK : MICD_ERR_CAPACITY;
}

// ---- the RLE header walk of a whole frame, in parts -----------------------------------------------------------------------------
// A WaveletV2 frame is ONE token stream of millions of tokens whose headers form a linked list (rledecompressu16.go:59-85: the
// next header's position is this one's value), and a walk costs a wave some hundreds of cycles per header whatever else the GPU
// does.  But the list is self-synchronising: a walk started at a token that is no header lands on a true one within a few steps
// and is the true walk from there.  So the stream is cut into WP_PARTS parts, a wave per part walks from the part's first token
// (part 0: from the first header; a walk that takes a zero token for a header has proved itself wrong -- no encoder writes a zero
// count, and zero symbols are common in literal chunks -- and starts over behind it) and leaves its records {payload token | run
// flag, first symbol RELATIVE to the part} in a region of its own; k_rle_walk_fix then hops from part to part -- the true walk
// enters a part at the exit of the part before; the true headers the part's own walk has not got are taken from a 64-token window
// (up to WP_EXTRA of them, else the frame goes to k_wv_expand) until it stands on a position the part has a record of -- and
// k_rle_walk_compact moves the true records to the front of `seg` with their absolute symbol positions, filling `flags` with
// the segment that holds every WS_T-th symbol.  A zero count that IS on the true walk is the reference's literal chunk of
// 65536 - midCount (k_wv_expand reads it so): the fix kernel hands such frames over.  Stop and error rules are k_wv_expand's.
#define WP_PARTS 64
#define WP_MINLEN 4096u
#define WP_EXTRA 1024u                             // true headers a part may hold in front of the point where its own walk joins the true one
// per part, in the unit's cumul[] slab (free after the tables)
struct WpPart { uint32_t start, exit, nrec, out_total, err, first, base_seg, out_delta, nextra, extra_base, pad0, pad1; };
__device__ __forceinline__ uint32_t wp_part_len(uint32_t ntok) { return max(WP_MINLEN, (((ntok + WP_PARTS - 1) / WP_PARTS) + 63u) & ~63u); }
__device__ __forceinline__ uint32_t wp_stride(uint32_t L) { return L / 2 + 1 + WP_EXTRA + 1; }     // records of a part: its own walk's, then the extras (+ an end mark)
__device__ __forceinline__ bool wp_fits(const MicUnit &u, uint32_t L) {        // temporary records in the upper half of seg, final ones in the lower
    const uint32_t nparts = (u.ntok + L - 1) / L;
    return u.seg != nullptr && (uint64_t)nparts * wp_stride(L) <= u.seg_cap / 2 && u.ntok / 2 + 2 <= u.seg_cap / 2;
}
__global__ void __launch_bounds__(64) k_rle_walk_parts(MicUnit *units) {
    MicUnit &u = units[blockIdx.y];
    if (u.status != MICD_OK || u.walk_mode != 1 || u.dec_stage != MIC_STAGE_PARTS) return;
    const uint32_t ntok = u.ntok, p = blockIdx.x, lane = threadIdx.x;
    if (ntok < 3) return;
    const uint16_t *tok = u.tok;
    const uint32_t L = wp_part_len(ntok), lo = p * L;
    if (lo >= ntok || !wp_fits(u, L)) return;
    const uint32_t hi = min(lo + L, ntok);
    uint32_t mid;
    if (!mic_rle_mid(tok[0], mid)) return;
    uint2 *rec = u.seg + u.seg_cap / 2 + (size_t)p * wp_stride(L);
    const bool pre = mic_is_prefix(u);                                      // the tokens end at the chain's ceiling
    uint32_t pos = p ? lo : 3u, out = 0, nrec = 0, err = 0, fin = 0;
    const uint32_t start = pos;
    while (pos < hi && !err && !fin) {
        const uint32_t w = (pos + lane < ntok) ? tok[pos + lane] : 0u;
        uint32_t j = 0;
        while (j < 64 && pos + j < hi) {
            const uint32_t h = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)j);
            if (h == 0) {
                // an encoder never writes a zero count.  The first part's walk is the true one: an error; any other part's walk started at
                // some token and has just proved itself wrong (zero symbols are common in literal chunks): it starts over behind the zero
                if (p == 0) { err = 1; break; }
                nrec = 0; out = 0; j += 1;
                continue;
            }
            const MicRleHdr hd = mic_rle_hdr(h, mid);
            if (hd.run && pos + j + 1 >= ntok) {
                if (pre) { fin = 1; break; }                                // a prefix ends in front of a run whose value it lacks: exit = that header
                if (p == 0) err = 1; else { nrec = 0; out = 0; j = 64; pos = hi; }
                break;
            }
            if (lane == 0) rec[nrec] = make_uint2(hd.rec(pos + j), out);
            nrec++; out += hd.len; j += hd.adv;
        }
        pos += j;
    }
    if (lane == 0) {
        WpPart &s = ((WpPart *)u.cumul)[p];
        s.start = start; s.exit = err ? 0xFFFFFFFFu : pos; s.nrec = nrec; s.out_total = out; s.err = err; s.first = 0xFFFFFFFFu; s.nextra = 0;
    }
}
// One wave per unit: the true walk from part to part.  In a part it first takes the true headers the part's own walk has not got
// (that walk started at a token that need not be a header; it joins the true one after a few of them) -- read from a 64-token
// window, noted as "extras" with their absolute symbol positions -- until it stands on a position the part has a record of.
__global__ void __launch_bounds__(64) k_rle_walk_fix(MicUnit *units) {
    MicUnit &u = units[blockIdx.x];
    if (u.status != MICD_OK || u.walk_mode != 1 || u.dec_stage != MIC_STAGE_PARTS) return;
    const uint32_t ntok = u.ntok, lane = threadIdx.x;
    const uint32_t L = wp_part_len(max(ntok, 1u));
    const uint16_t *tok = u.tok;
    uint32_t mid = 0;
    bool ok = ntok >= 3 && wp_fits(u, L) && mic_rle_mid(tok[0], mid), fin = false;
    const bool pre = mic_is_prefix(u);                                      // a prefix: the walk ends cleanly where its tokens do
    const uint32_t cap = ok ? ((uint32_t)tok[1] << 16) + tok[2] : 0u;
    if (cap > u.sym_cap) ok = false;
    WpPart *S = (WpPart *)u.cumul;
    uint32_t e = 3, N = 0, O = 0;                                           // the next true header, records and symbols in front of it
    uint32_t wbase = 0xFFFFFFFFu, wtok = 0;                                 // token window [wbase, wbase + 64)
    while (ok && e < ntok && O < cap) {
        const uint32_t q = e / L, hi = min((q + 1) * L, ntok);
        const WpPart s = S[q];
        uint2 *rec = u.seg + u.seg_cap / 2 + (size_t)q * wp_stride(L);
        uint2 *extra = rec + (L / 2 + 1);
        uint32_t blk = 0, nx = 0, first = s.nrec;
        const uint32_t N0 = N;
        uint2 r = (lane < s.nrec) ? rec[lane] : make_uint2(0xFFFFFFFFu, 0u);
        bool synced = false;
        uint32_t r0 = 0;
        while (e < hi && O < cap) {
            // first record of the part at or behind e
            uint64_t m;
            while (!(m = __ballot((r.x & 0x7FFFFFFFu) >= e + 1)) && (blk + 1) * 64 < s.nrec) {
                blk++;
                r = (blk * 64 + lane < s.nrec) ? rec[blk * 64 + lane] : make_uint2(0xFFFFFFFFu, 0u);
            }
            if (m) {
                const int i = (int)__builtin_ctzll(m);
                const uint32_t px = (uint32_t)__builtin_amdgcn_readlane((int)r.x, i) & 0x7FFFFFFFu;
                if (px == e + 1 && blk * 64 + (uint32_t)i < s.nrec) {       // the part's own walk stands here too: the rest of it is true
                    first = blk * 64 + (uint32_t)i;
                    r0 = (uint32_t)__builtin_amdgcn_readlane((int)r.y, i);
                    synced = true;
                    break;
                }
            }
            // a true header the part has no record of
            if (e - wbase >= 64u) { wbase = e; wtok = (e + lane < ntok) ? tok[e + lane] : 0u; }
            const uint32_t h = (uint32_t)__builtin_amdgcn_readlane((int)wtok, (int)(e - wbase));
            if (h == 0 || nx >= WP_EXTRA) { ok = false; break; }                // (a zero count: corrupt; too many: the one-group kernels take the frame)
            const MicRleHdr hd = mic_rle_hdr(h, mid);
            if (hd.run && e + 1 >= ntok) { if (pre) fin = true; else ok = false; break; }
            if (lane == 0) extra[nx] = make_uint2(hd.rec(e), O);
            nx++; O += hd.len; e += hd.adv;
        }
        if (!ok) break;
        if (lane == 0) {
            extra[nx] = make_uint2(0u, O);                                  // end mark: the symbol position behind the last extra
            S[q].first = first; S[q].nextra = nx; S[q].extra_base = N0; S[q].base_seg = N0 + nx; S[q].out_delta = O - r0;
        }
        N = N0 + nx;
        if (fin) break;
        if (!synced) continue;                                              // the true walk left the part on its own (or the stream has its symbols)
        N += s.nrec - first; O += s.out_total - r0;
        if (s.err) { if (O < cap) ok = false; break; }                      // the zero header is reached before the stream has its symbols
        e = s.exit;
        if (pre && e < hi) break;                                           // the part's walk stopped where the prefix does (a run without its value)
    }
    if (ok && O < cap && !pre) ok = false;                                  // tokens ran out (Go: index panic)
    // the words the tokens cover: all `cap`, or -- a prefix -- those in front of its end (e: the header behind the last one walked;
    // past ntok when that was a literal chunk the prefix holds only the front of)
    const uint32_t cover = pre ? min(cap, O - (e > ntok ? e - ntok : 0u)) : cap;
    if (lane == 0) {
        if (ok) { u.nseg = N; u.nsym = cover; u.dec_stage = MIC_STAGE_SEGS; }
        else u.dec_stage = MIC_STAGE_NONE;
    }
}
__global__ void __launch_bounds__(256) k_rle_walk_compact(MicUnit *units) {
    MicUnit &u = units[blockIdx.y];
    if (u.status != MICD_OK || u.walk_mode != 1 || u.dec_stage != MIC_STAGE_SEGS) return;
    const uint32_t L = wp_part_len(u.ntok), q = blockIdx.x;
    if (q * L >= u.ntok) return;
    const WpPart s = ((const WpPart *)u.cumul)[q];
    if (s.first == 0xFFFFFFFFu) return;                                     // the true walk jumps over this part (or ends before it)
    const uint2 *rec = u.seg + u.seg_cap / 2 + (size_t)q * wp_stride(L);
    const uint2 *extra = rec + (L / 2 + 1);
    uint32_t *tidx = u.flags;
    const uint32_t nsym = u.nsym;
    auto put = [&](uint32_t idx, uint32_t x, uint32_t o, uint32_t len) {
        u.seg[idx] = make_uint2(x, o);
        // the literal chunk that holds the stream's last symbol must lie inside the tokens: k_wv_scatter reads only the first n
        // symbols, Go reads all of them (rledecompressu16.go:87-97: index panic).  Such a frame is k_wv_expand's, which reports it.
        if (!(x >> 31) && o < nsym && nsym - o <= len && x + (nsym - 1 - o) >= u.ntok) u.wv_slow = 1;
        if (((o + len - 1) >> 13) != ((o - 1) >> 13))
            for (uint32_t kk = (o + (WS_T - 1)) >> 13; (kk << 13) < o + len && (kk << 13) < nsym; kk++) tidx[kk] = idx;
    };
    for (uint32_t r = threadIdx.x; r < s.nextra; r += 256) {                // (absolute symbol positions; the end mark carries the position behind the last)
        const uint2 v = extra[r];
        put(s.extra_base + r, v.x, v.y, extra[r + 1].y - v.y);
    }
    for (uint32_t r = s.first + threadIdx.x; r < s.nrec; r += 256) {
        const uint2 v = rec[r];
        const uint32_t nxt = (r + 1 < s.nrec) ? rec[r + 1].y : s.out_total;
        put(s.base_seg + (r - s.first), v.x, v.y + s.out_delta, nxt - v.y);
    }
}

// RLE expansion + zigzag decode + subband scatter in one pass, output-driven: a group owns WS_T consecutive scan positions, a
// thread eight; the RLE segments k_dec_translate's walker left ({payload token | run flag, first symbol}, and in `flags` the
// segment that holds every WS_T-th symbol) say where a position's symbol lies in the token stream (the fetch is
// k_dec_pixels_wg's: segment table in LDS, gallop + bisection, one 16-byte load inside a literal chunk).  A frame with an escape
// word (65535) in its symbols, fewer symbols than samples, or a stream the walker refused goes to k_wv_expand + k_wv_coeffs.
// lim (the frame's): the scan positions wanted -- n, or P(r) of a decode at reduced resolution (a prefix unit covering fewer goes the slow way)
__global__ void __launch_bounds__(1024) k_wv_scatter(MicUnit *units, const WvFrame *__restrict__ ft, const WvWork *__restrict__ wk, int32_t *a) {
    const WvWork wr = wv_work(wk);
    MicUnit &u = units[wr.frame];
    if (u.status != MICD_OK) return;
    const WvDims &d = ft[wr.frame].d;
    const uint32_t lim = ft[wr.frame].lim, tid = threadIdx.x;
    if (u.dec_stage != MIC_STAGE_SEGS || u.nsym < lim) { if (tid == 0) u.wv_slow = 1; return; }
    __shared__ uint32_t s_segx[1024], s_segy[1024 + 1];
    a += ft[wr.frame].a_off;
    const uint32_t nseg = u.nseg, ntok = u.ntok;
    const uint16_t *tok = u.tok;
    const uint2 *seg = u.seg;
    const uint32_t o0 = wr.bx * WS_T, tile_end = min(o0 + WS_T, lim);
    const uint32_t i0 = o0 + tid * 8, wend = min(i0 + 8, tile_end);
    uint32_t w8[4] = { 0u, 0u, 0u, 0u }, bad = 0;
    bool got = i0 >= tile_end;
    for (uint32_t r0 = u.flags[wr.bx];; r0 += 1024 - 8) {            // table rounds overlap by 8 segments (8 symbols span at most 8)
        __syncthreads();
        const uint32_t si = r0 + tid;
        uint2 sg = make_uint2(0u, 0xFFFFFFFFu);
        if (si < nseg) sg = seg[si];
        s_segx[tid] = sg.x; s_segy[tid] = sg.y;
        if (tid == 0) { const uint32_t sj = r0 + 1024; s_segy[1024] = (sj < nseg) ? seg[sj].y : 0xFFFFFFFFu; }
        __syncthreads();
        const uint32_t cover_end = s_segy[1024];
        if (!got && s_segy[0] <= i0 && wend <= cover_end) {
            uint32_t j = 0, stp = 16;
            while (j + stp <= 1024 && s_segy[j + stp] <= i0) { j += stp; stp <<= 1; }
            for (stp >>= 1; stp; stp >>= 1) if (j + stp <= 1024 && s_segy[j + stp] <= i0) j += stp;
            uint32_t start = s_segy[j], endj = s_segy[j + 1], sx = s_segx[j];
            if (wend - i0 == 8 && i0 + 8 <= endj) {
                const uint32_t xs = sx & 0x7FFFFFFFu;
                if (sx >> 31) { const uint32_t v = (xs < ntok) ? tok[xs] : 0u; w8[0] = w8[1] = w8[2] = w8[3] = v | (v << 16); }
                else {
                    const uint32_t src = xs + (i0 - start);
                    if (src + 8 <= ntok) { const wv_v4 v = *(const WvQ2 *)(tok + src); w8[0] = v.x; w8[1] = v.y; w8[2] = v.z; w8[3] = v.w; }
                    else bad = 1;                                           // literal chunk past the end (Go: index panic)
                }
            } else {
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const uint32_t i = i0 + (uint32_t)k;
                    if (i < wend) {
                        while (i >= endj) { j++; start = s_segy[j]; endj = s_segy[j + 1]; sx = s_segx[j]; }
                        const uint32_t xs = sx & 0x7FFFFFFFu;
                        const uint32_t src = (sx >> 31) ? xs : xs + (i - start);
                        if (src < ntok) w8[k >> 1] |= (uint32_t)tok[src] << (16 * (k & 1)); else bad = 1;
                    }
                }
            }
            got = true;
        }
        if (!(cover_end < tile_end)) break;
    }
    if (!got) bad = 1;
    uint32_t idx = 0, left = 0;
    int32_t v8[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t x = (w8[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
        if (x == 65535u && i0 + (uint32_t)k < wend) bad = 1;               // an escape marker: positions and symbols part ways
        v8[k] = (int32_t)((x >> 1) ^ (uint32_t)(-(int32_t)(x & 1)));       // zigzagDecode16, :543-546
    }
    if (bad) { u.wv_slow = 1; return; }
    if (i0 >= wend) return;
    wv_pos_row(d, i0, idx, left);
    if (wend - i0 == 8 && left >= 8) {
        wv_v4 lo, hi; lo.x = (uint32_t)v8[0]; lo.y = (uint32_t)v8[1]; lo.z = (uint32_t)v8[2]; lo.w = (uint32_t)v8[3];
        hi.x = (uint32_t)v8[4]; hi.y = (uint32_t)v8[5]; hi.z = (uint32_t)v8[6]; hi.w = (uint32_t)v8[7];
        *(WvQ4 *)(a + idx) = lo; *(WvQ4 *)(a + idx + 4) = hi;
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (i0 + (uint32_t)k < wend) {
                if (left == 0) wv_pos_row(d, i0 + (uint32_t)k, idx, left);
                a[idx] = v8[k]; idx++; left--;
            }
        }
    }
}

// The most symbols a WaveletV2 stream of n pixels may announce: every coefficient escaped (3 words), + 8.  Go has no ceiling
// (rledecompressu16.go:87-97 allocates what the stream announces); a stream above this one is MIC_ERR_CORRUPT here and in the oracle.
inline size_t wv_sym_ceiling(size_t n) { return 3 * n + 8; }

}  // namespace

void mic_launch_rle_expand(MicUnit *d_units, int n, hipStream_t stream, int mode_filter) {
    hipLaunchKernelGGL(k_wv_expand, dim3((unsigned)n), dim3(WV_THREADS), 0, stream, d_units, mode_filter, 0);
}

namespace {

// ---- the tables of a launch chain, on the host -------------------------------------------------------------------------------------
// The work lists of a chain, one per launch (a span of the chain's work records), in this order.
enum { WV_ENC_LOAD = 0, WV_ENC_FWD = 1 /* + l, 0 .. 7 */, WV_ENC_POS = 9, WV_ENC_LISTS = 10 };
enum { WV_DEC_POS = 0, WV_DEC_STORE = 1, WV_DEC_BAND = 2, WV_DEC_INV = 3 /* + l: level l restored as it is */,
       WV_DEC_SAT = 11 /* + l, 1 .. 7: level l as the saturated band of a reduced decode */, WV_DEC_LISTS = 19 };
struct WvTables {
    std::vector<WvFrame> fr; std::vector<WvWork> wk; std::vector<uint32_t> spans;       // spans: first, count per list
    size_t a_elems = 0, b_elems = 0, n_max = 0;
    // frame i: rows x cols with `levels` applied, wanted at `level`, its pixels px_off elements into the launch's pixel buffer
    void add(int rows, int cols, int levels, int level, uint64_t px_off) {
        WvFrame f{};
        f.d = wv_dims(rows, cols, levels); f.level = level;
        f.lim = (uint32_t)f.d.nr[level] * (uint32_t)f.d.nc[level];
        f.ll_half = (uint32_t)align_up((size_t)f.d.nr[1] * (size_t)f.d.nc[1], 4);
        f.px_off = px_off; f.a_off = a_elems; f.b_off = b_elems;
        const size_t n = (size_t)rows * (size_t)cols;
        a_elems += align_up(n, 4); b_elems += 2 * (size_t)f.ll_half;
        n_max = std::max(n_max, n);
        fr.push_back(f);
    }
    // the next list: nbx x nby records (tiles(f, nbx, nby)) of every frame that takes part
    template <class Take, class Tiles> void list(Take &&take, Tiles &&tiles) {
        const size_t first = wk.size();
        for (size_t f = 0; f < fr.size(); f++) {
            if (!take(fr[f])) continue;
            uint32_t nbx = 0, nby = 1;
            tiles(fr[f], nbx, nby);
            for (uint32_t by = 0; by < nby; by++) for (uint32_t bx = 0; bx < nbx; bx++) wk.push_back(WvWork{ (uint32_t)f, bx, by, 0u });
        }
        spans.push_back((uint32_t)first); spans.push_back((uint32_t)(wk.size() - first));
    }
    static void level_tiles(const WvFrame &f, int l, uint32_t &nbx, uint32_t &nby) {     // the blocks of level l: pairs of columns x pairs of rows
        nbx = (uint32_t)(((f.d.nc[l] + 1) / 2 + 4 * WS_LANES - 1) / (4 * WS_LANES));
        nby = (uint32_t)(((f.d.nr[l] + 1) / 2 + WS_ROWS - 1) / WS_ROWS);
    }
    void encode_lists() {
        list([](const WvFrame &f) { return f.d.levels == 0; }, [](const WvFrame &f, uint32_t &nbx, uint32_t &) { nbx = (f.lim + WV_CHUNK - 1) / WV_CHUNK; });
        for (int l = 0; l < 8; l++)
            list([l](const WvFrame &f) { return l < f.d.levels; }, [l](const WvFrame &f, uint32_t &nbx, uint32_t &nby) { level_tiles(f, l, nbx, nby); });
        list([](const WvFrame &) { return true; }, [](const WvFrame &f, uint32_t &nbx, uint32_t &) { nbx = (f.lim + WS_T - 1) / WS_T; });
    }
    void decode_lists() {
        list([](const WvFrame &) { return true; }, [](const WvFrame &f, uint32_t &nbx, uint32_t &) { nbx = (f.lim + WS_T - 1) / WS_T; });
        list([](const WvFrame &f) { return f.d.levels == 0; }, [](const WvFrame &f, uint32_t &nbx, uint32_t &) { nbx = (f.lim + WV_CHUNK - 1) / WV_CHUNK; });
        list([](const WvFrame &f) { return f.d.levels > 0 && f.level == f.d.levels; }, [](const WvFrame &f, uint32_t &nbx, uint32_t &) { nbx = (f.lim + WV_CHUNK - 1) / WV_CHUNK; });
        for (int l = 0; l < 8; l++)
            list([l](const WvFrame &f) { return l < f.d.levels && (l == 0 ? f.level == 0 : f.level < l); },
                 [l](const WvFrame &f, uint32_t &nbx, uint32_t &nby) { level_tiles(f, l, nbx, nby); });
        for (int l = 0; l < 8; l++)
            list([l](const WvFrame &f) { return l > 0 && l < f.d.levels && f.level == l; },
                 [l](const WvFrame &f, uint32_t &nbx, uint32_t &nby) { level_tiles(f, l, nbx, nby); });
    }
};
// The chain's tables on the device, in the session's wv_tab_enc / wv_tab_dec: the frame records, then the work records.  A chain over the
// frame records the buffer holds already builds and uploads nothing -- a loop of encode and decode calls on one list of shapes, each
// with a buffer of its own, pays for its tables once.  The stream orders an upload behind the kernels of the chain before.
struct WvDevTables { const WvFrame *ft; const WvWork *wk; const uint32_t *spans; };
int wv_upload_tables(mic_hip_session *s, WvTables &t, bool encode, WvDevTables &dev) {
    DevBuf &buf = encode ? s->wv_tab_enc : s->wv_tab_dec;
    mic_hip_session::WvTabHeld &held = s->wv_tab_held[encode ? 1 : 0];
    const size_t fbytes = t.fr.size() * sizeof(WvFrame);
    const bool hit = buf.p && buf.gen == held.gen && held.key.size() == fbytes && memcmp(held.key.data(), t.fr.data(), fbytes) == 0;
    if (!hit) {
        held.gen = ~0ull;                                                 // (nothing is known of the buffer until the upload is queued)
        if (encode) t.encode_lists(); else t.decode_lists();
        // what the launches assume of their grids is checked before the first of them
        if (t.wk.size() >= ((size_t)1 << 31)) return MIC_ERR_UNSUPPORTED;
        const size_t wbytes = t.wk.size() * sizeof(WvWork);
        int rc = buf.reserve(fbytes + wbytes + 64);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(buf.p, t.fr.data(), fbytes, hipMemcpyHostToDevice, s->stream));
        if (wbytes) HIP_TRY(hipMemcpyAsync((char *)buf.p + fbytes, t.wk.data(), wbytes, hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));                         // (the host vectors go away with the call)
        held.key.assign((const uint8_t *)t.fr.data(), (const uint8_t *)t.fr.data() + fbytes);
        held.spans.swap(t.spans); held.gen = buf.gen;
    }
    dev.ft = (const WvFrame *)buf.p;
    dev.wk = (const WvWork *)((const char *)buf.p + fbytes);
    dev.spans = held.spans.data();
    return MIC_OK;
}
static_assert(sizeof(WvFrame) == 128 && sizeof(WvWork) == 16, "the work records behind the frame records are loaded 16 bytes at a time");

// THE core of every WaveletV2 encode: the frames of `t` (any shapes and level counts; their pixels at d_src + px_off) through one
// launch chain -- forward transform level by level, each level over the frames that have it; symbols; RLE + 4-state FSE.  On return
// the streams (without the 11-byte header) lie packed in the session: *d_blobs + offs[i] .. offs[i + 1], st[i] = frame i's status.
// Every unit is laid out by the largest frame (the tier-2 slabs of this path are not tiered: DESIGN.md section 7 item 6).
int wv_compress_core(mic_hip_session *s, const uint16_t *d_src, WvTables &t, std::vector<int32_t> &st, const uint8_t **d_blobs, uint64_t *offs) {
    const int nf = (int)t.fr.size();
    if (nf <= 0) return MIC_ERR_ARGS;
    int rc;
    if ((rc = s->lay_out(nf, 2 * t.n_max + 16))) return rc;              // room for 3-word escapes
    DevBuf &a = s->wv_a, &b = s->wv_b;                                   // coefficient planes: kept by the session (no hipMalloc per call)
    // b: the smooth planes between levels, two per frame (levels alternate), each (rows + 1) / 2 x (cols + 1) / 2
    if ((rc = a.reserve(t.a_elems * 4 + 64)) || (rc = b.reserve(t.b_elems * 4 + 64))) return rc;
    WvDevTables dv;
    if ((rc = wv_upload_tables(s, t, true, dv))) return rc;
    int32_t *A = (int32_t *)a.p, *B = (int32_t *)b.p;
    for (int i = 0; i < nf; i++) {
        MicUnit &u = s->h_units[(size_t)i];
        u.w = 1; u.h = 1; u.nstates = 4; u.mode = 2; u.no_fallback = 1; // FSECompressU16FourState, no fallback (:344)
    }
    auto first = [&](int list) { return dv.wk + dv.spans[2 * list]; };
    auto count = [&](int list) { return dv.spans[2 * list + 1]; };
    rc = s->run_encode([&] {
        MicUnit *U = (MicUnit *)s->units.p;
        s->timer.mark("k_wv_fwd2d");
        if (count(WV_ENC_LOAD)) hipLaunchKernelGGL(k_wv_load, dim3(count(WV_ENC_LOAD)), dim3(256), 0, s->stream, dv.ft, first(WV_ENC_LOAD), d_src, A);
        for (int l = 0; l < 8 && count(WV_ENC_FWD + l); l++) {           // a level per launch, over the frames that have it: level l's smooth plane in B, parity l
            if (l == 0) hipLaunchKernelGGL(k_wv_fwd2d<true>, dim3(count(WV_ENC_FWD)), dim3(256), 0, s->stream, dv.ft, first(WV_ENC_FWD), d_src, A, B, 0);
            else hipLaunchKernelGGL(k_wv_fwd2d<false>, dim3(count(WV_ENC_FWD + l)), dim3(256), 0, s->stream, dv.ft, first(WV_ENC_FWD + l), d_src, A, B, l);
        }
        s->timer.mark("k_wv_symbols");
        hipLaunchKernelGGL(k_wv_symbols_par, dim3(count(WV_ENC_POS)), dim3(1024), 0, s->stream, U, dv.ft, first(WV_ENC_POS), (const int32_t *)A);
        hipLaunchKernelGGL(k_wv_symbols_fin, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s->stream, U, dv.ft, nf);
        hipLaunchKernelGGL(k_wv_symbols, dim3((unsigned)nf), dim3(WV_THREADS), 0, s->stream, U, dv.ft, (const int32_t *)A);   // frames with wide coefficients
        mic_launch_encode(U, nf, s->stream, s->variant, &s->timer);
    });
    if (rc) return rc;
    std::vector<int32_t> ns((size_t)nf);
    st.assign((size_t)nf, 0);
    return session_encode_finish(s, d_blobs, offs, st.data(), ns.data());
}

// One decode chain: the frames of `t` (frame i: the FSE stream d_comp + begins[i] .. ends[i], its pixels -- the band at its `level` -- to
// d_dst + px_off) with MicUnit::sym_limit = limits[i] (0: the whole stream).
int wv_decompress_frames(mic_hip_session *s, const uint8_t *d_comp, uint16_t *d_dst, WvTables &t, const uint64_t *begins, const uint64_t *ends,
                        const uint32_t *limits, std::vector<int32_t> &st) {
    const int nf = (int)t.fr.size();
    int rc;
    // everything the launches below assume is checked before the first of them: grid limits, stream ranges
    if (nf <= 0 || nf > 65535) return MIC_ERR_UNSUPPORTED;
    for (int i = 0; i < nf; i++)
        if (ends[i] < begins[i] || ends[i] - begins[i] > 0xFFFFFFF0ull) return MIC_ERR_ARGS;
    if ((rc = s->lay_out(nf, 2 * t.n_max + 16))) return rc;
    DevBuf &a = s->wv_a, &b = s->wv_b;
    if ((rc = a.reserve(t.a_elems * 4 + 64)) || (rc = b.reserve(t.b_elems * 4 + 64))) return rc;   // (the smooth planes between levels, as in wv_compress_core)
    WvDevTables dv;
    if ((rc = wv_upload_tables(s, t, false, dv))) return rc;
    for (int i = 0; i < nf; i++) {
        MicUnit &u = s->h_units[(size_t)i];
        const WvDims &d = t.fr[(size_t)i].d;
        u.comp_in = d_comp + begins[i]; u.comp_len = (uint32_t)(ends[i] - begins[i]); u.w = 1; u.h = 1; u.mode = 1; u.walk_mode = 1;
        u.sym_cap = (uint32_t)std::min<size_t>(u.sym_cap, wv_sym_ceiling((size_t)d.rows * (size_t)d.cols));   // the oracle's ceiling: DESIGN.md section 4, WaveletV2
        u.sym_limit = limits[i];
    }
    int32_t *A = (int32_t *)a.p, *B = (int32_t *)b.p;
    auto first = [&](int list) { return dv.wk + dv.spans[2 * list]; };
    auto count = [&](int list) { return dv.spans[2 * list + 1]; };
    rc = s->run_decode(mic_hip_session::FlagSlab::Idle, [&] {            // (k_rle_walk_compact's scratch)
        MicUnit *U = (MicUnit *)s->units.p;
        mic_launch_decode(U, nf, s->stream, s->variant, &s->timer, (int *)s->cls.p);
        if (s->timer.used) { s->timer.used--; s->timer.names.pop_back(); }   // (drop the chain's "end" mark: the wavelet kernels follow)
        s->timer.mark("k_rle_walk_parts+fix+compact");
        hipLaunchKernelGGL(k_rle_walk_parts, dim3(WP_PARTS, (unsigned)nf), dim3(64), 0, s->stream, U);
        hipLaunchKernelGGL(k_rle_walk_fix, dim3((unsigned)nf), dim3(64), 0, s->stream, U);
        hipLaunchKernelGGL(k_rle_walk_compact, dim3(WP_PARTS, (unsigned)nf), dim3(256), 0, s->stream, U);
        s->timer.mark("k_wv_scatter");
        hipLaunchKernelGGL(k_wv_scatter, dim3(count(WV_DEC_POS)), dim3(1024), 0, s->stream, U, dv.ft, first(WV_DEC_POS), A);
        s->timer.mark("k_wv_expand+coeffs (escape frames)");
        hipLaunchKernelGGL(k_wv_expand, dim3((unsigned)nf), dim3(WV_THREADS), 0, s->stream, U, -1, 1);
        hipLaunchKernelGGL(k_wv_coeffs, dim3((unsigned)nf), dim3(WV_THREADS), 0, s->stream, U, dv.ft, A);
        s->timer.mark("k_wv_inv2d");
        if (count(WV_DEC_STORE)) hipLaunchKernelGGL(k_wv_store, dim3(count(WV_DEC_STORE)), dim3(256), 0, s->stream, dv.ft, first(WV_DEC_STORE), (const int32_t *)A, d_dst);
        if (count(WV_DEC_BAND)) hipLaunchKernelGGL(k_wv_band, dim3(count(WV_DEC_BAND)), dim3(256), 0, s->stream, dv.ft, first(WV_DEC_BAND), (const int32_t *)A, d_dst);
        for (int l = 7; l >= 0; l--) {                                       // coarse -> fine, :519-527; a level over the frames that have it
            const int plain = WV_DEC_INV + l, sat = WV_DEC_SAT + l;
            if (count(plain)) {
                if (l == 0) hipLaunchKernelGGL(k_wv_inv2d<true>, dim3(count(plain)), dim3(256), 0, s->stream, dv.ft, first(plain), (const int32_t *)A, B, d_dst, l);
                else hipLaunchKernelGGL(k_wv_inv2d<false>, dim3(count(plain)), dim3(256), 0, s->stream, dv.ft, first(plain), (const int32_t *)A, B, d_dst, l);
            }
            if (count(sat))                                                  // reduced resolution: the band, saturated, stride nc[level]
                hipLaunchKernelGGL((k_wv_inv2d<true, true>), dim3(count(sat)), dim3(256), 0, s->stream, dv.ft, first(sat), (const int32_t *)A, B, d_dst, l);
        }
        s->timer.mark("end");
    });
    if (rc) return rc;
    st.assign((size_t)nf, 0);
    return session_decode_finish(s, st.data());
}

// The tANS ceiling of pass 1 of a decode at reduced resolution ("WaveletV2 at reduced resolution"): the image at
// level r needs the first P = nr[r] * nc[r] coefficients of the subband scan -- P RLE words when none of them is escaped -- and
// those take the first tokens of the stream: fewer than P where runs fold them, a header per literal chunk more.  P + P/4 + 512 tokens
// (whole 128-symbol chunks) cover every frame whose coefficients are not escape-heavy; a frame they do not cover is decoded again
// whole (pass 2).  P = n (level 0) is the whole stream: 0, no ceiling.
uint32_t wv_level_sym_limit(size_t P, size_t n) {
    if (P >= n) return 0;
    const size_t lim = (P + P / 4 + 512 + 127) & ~(size_t)127;
    return (uint32_t)std::min<size_t>(lim, 0xFFFFFF00u);
}

// THE core of every WaveletV2 decode: the frames of `t`, each at its own `level`, in two passes under one rule.  Pass 1 decodes every
// frame with the tANS chain stopped at the frame's wv_level_sym_limit; a frame whose prefix did not give its P coefficients --
// escape-heavy frames (every 16-bit coefficient outside +-32767 is three words), or any failure inside the prefix -- is decoded again
// in pass 2, whole (sym_limit 0), in a launch chain of its own over a sub-table of those frames, to the same place; that pass's status
// and output are the frame's.  Every other frame keeps pass 1's.  The outputs are the same whichever pass made them; only a pass-2
// (or level-0) decode checks the whole stream.  syms (nullable): tANS symbols the chain decoded per frame, both passes summed.
// redone (nullable): + the frames of pass 2 (a launch chain more when there are any).
int wv_decompress_core(mic_hip_session *s, const uint8_t *d_comp, uint16_t *d_dst, WvTables &t, const uint64_t *begins, const uint64_t *ends,
                       std::vector<int32_t> &st, uint64_t *syms, uint64_t *redone = nullptr) {
    const int nf = (int)t.fr.size();
    std::vector<uint32_t> limits((size_t)std::max(nf, 0));
    for (int i = 0; i < nf; i++) {
        const WvFrame &f = t.fr[(size_t)i];
        if (f.level < 0 || f.level > f.d.levels || f.d.levels > 8) return MIC_ERR_ARGS;
        limits[(size_t)i] = wv_level_sym_limit(f.lim, (size_t)f.d.rows * (size_t)f.d.cols);
    }
    int rc = wv_decompress_frames(s, d_comp, d_dst, t, begins, ends, limits.data(), st);
    if (rc) return rc;
    std::vector<int> redo; std::vector<uint64_t> b2, e2;
    WvTables t2;
    for (int i = 0; i < nf; i++) {
        const MicUnit &u = s->h_units[(size_t)i];                       // (read back by session_decode_finish)
        if (syms) syms[i] = u.ntok;
        if (st[(size_t)i] != MIC_OK && mic_is_prefix(u)) {
            const WvFrame &f = t.fr[(size_t)i];
            redo.push_back(i); b2.push_back(begins[i]); e2.push_back(ends[i]);
            t2.add(f.d.rows, f.d.cols, f.d.levels, f.level, f.px_off);
        }
    }
    if (redo.empty()) return MIC_OK;
    const int k = (int)redo.size();
    if (redone) *redone += (uint64_t)k;
    std::vector<int32_t> st2; const std::vector<uint32_t> whole((size_t)k, 0u);
    if ((rc = wv_decompress_frames(s, d_comp, d_dst, t2, b2.data(), e2.data(), whole.data(), st2))) return rc;
    for (int j = 0; j < k; j++) {
        const int i = redo[(size_t)j];
        st[(size_t)i] = st2[(size_t)j];
        if (syms) syms[i] += s->h_units[(size_t)j].ntok;
    }
    return MIC_OK;
}

// ---- the one-shape callers: a table of equal rows --------------------------------------------------------------------------------
// nf frames of rows x cols, contiguous on the device at d_src.  blobs[i] receives frame i's FSE stream (without the 11-byte header),
// st[i] its status.  blobs == nullptr: the streams stay on the device (session_encode_finish's packed buffer: *d_blobs_out /
// offs_out), nothing is copied to the host.
int wv_compress_frames(mic_hip_session *s, const uint16_t *d_src, int nf, int rows, int cols, int applied,
                       std::vector<std::vector<uint8_t>> *blobs, std::vector<int32_t> &st,
                       const uint8_t **d_blobs_out = nullptr, uint64_t *offs_out = nullptr) {
    const size_t n = (size_t)rows * (size_t)cols;
    WvTables t;
    for (int i = 0; i < nf; i++) t.add(rows, cols, applied, 0, (uint64_t)i * n);
    std::vector<uint64_t> offs((size_t)std::max(nf, 0) + 1); const uint8_t *d_blobs = nullptr;
    int rc = wv_compress_core(s, d_src, t, st, &d_blobs, offs.data());
    if (rc) return rc;
    if (!blobs) {
        if (d_blobs_out) *d_blobs_out = d_blobs;
        if (offs_out) memcpy(offs_out, offs.data(), sizeof(uint64_t) * ((size_t)nf + 1));
        return MIC_OK;
    }
    std::vector<uint8_t> host((size_t)offs[(size_t)nf] + 16);
    if (offs[(size_t)nf] && hipMemcpy(host.data(), d_blobs, (size_t)offs[(size_t)nf], hipMemcpyDeviceToHost) != hipSuccess) return MIC_ERR_DEVICE;
    blobs->assign((size_t)nf, std::vector<uint8_t>());
    for (int i = 0; i < nf; i++) if (st[(size_t)i] == MIC_OK) (*blobs)[(size_t)i].assign(host.begin() + (long)offs[(size_t)i], host.begin() + (long)offs[(size_t)i + 1]);
    return MIC_OK;
}

// nf FSE streams (d_comp + offs[i] .. offs[i + 1]) of frames of one shape at `level` -> frame i's nr[level] x nc[level] band (row stride
// nc[level], saturated to u16; level 0: the image) at d_dst + i * nr[level] * nc[level]
int wv_decode_level_frames(mic_hip_session *s, const uint8_t *d_comp, uint16_t *d_dst, int nf, const uint64_t *offs, int rows, int cols,
                           int levels, int level, std::vector<int32_t> &st, uint64_t *syms) {
    if (level < 0 || level > levels || levels > 8) return MIC_ERR_ARGS;
    const WvDims d = wv_dims(rows, cols, levels);
    const size_t P = (size_t)d.nr[level] * (size_t)d.nc[level];
    WvTables t;
    for (int i = 0; i < nf; i++) t.add(rows, cols, levels, level, (uint64_t)i * P);
    return wv_decompress_core(s, d_comp, d_dst, t, offs, offs + 1, st, syms);
}

}  // namespace

namespace micapi {

void wv_put_header(uint8_t *out, int rows, int cols, uint16_t max_value, int applied) {     // :346-350
    out[0] = (uint8_t)rows; out[1] = (uint8_t)(rows >> 8); out[2] = (uint8_t)(rows >> 16); out[3] = (uint8_t)((uint32_t)rows >> 24);
    out[4] = (uint8_t)cols; out[5] = (uint8_t)(cols >> 8); out[6] = (uint8_t)(cols >> 16); out[7] = (uint8_t)((uint32_t)cols >> 24);
    out[8] = (uint8_t)max_value; out[9] = (uint8_t)(max_value >> 8);
    out[10] = (uint8_t)applied;
}

// the argument gate of every entry point: MIC_OK, or why rows x cols (a decode: at `level` of a header's `levels`) is not coded here
int wv_check_shape(int rows, int cols, int levels, int level) {
    if (rows <= 0 || cols <= 0 || levels < 0 || levels > 8 || level < 0 || level > levels) return MIC_ERR_ARGS;
    return (size_t)rows * (size_t)cols > ((size_t)1 << 27) ? MIC_ERR_UNSUPPORTED : MIC_OK;
}
// the level count the header carries: `levels` clamped to 1 .. 8, stopped where a side falls below 2 (waveletfsecompressu16.go:321-330)
int wv_levels_applied(int rows, int cols, int levels) {
    levels = std::min(std::max(levels, 1), 8);
    int applied = 0;
    for (int r = rows, c = cols; applied < levels && r >= 2 && c >= 2; applied++) { r = (r + 1) / 2; c = (c + 1) / 2; }
    return applied;
}

size_t wv_next_cut(const std::function<size_t(size_t)> &px, size_t i0, size_t n, size_t budget) {
    return next_sub_batch(i0, n, px, cap_by_largest([budget](size_t mp) { return std::max<size_t>(1, budget / (unit_ws_bytes(2 * mp + 16) + 8 * mp)); }),
                          CutRule{ 65535, ~(size_t)0, (size_t)1 << 30 });
}

int wv_encode_run(mic_hip_session *s, const uint16_t *d_px, const WvEncFrame *f, int n, const uint8_t **d_blobs, uint64_t *offs, int32_t *st) {
    WvTables t;
    for (int i = 0; i < n; i++) t.add(f[i].rows, f[i].cols, f[i].applied, 0, f[i].px_off);
    std::vector<int32_t> sv;
    const int rc = wv_compress_core(s, d_px, t, sv, d_blobs, offs);
    if (rc == MIC_OK) std::copy(sv.begin(), sv.end(), st);
    return rc;
}

int wv_decode_run(mic_hip_session *s, const uint8_t *d_comp, uint16_t *d_out, const WvDecFrame *f, int n, int32_t *st, uint64_t *syms, uint64_t *redone) {
    WvTables t; std::vector<uint64_t> b((size_t)std::max(n, 0)), e((size_t)std::max(n, 0));
    for (int i = 0; i < n; i++) {
        if (wv_check_shape(f[i].rows, f[i].cols, f[i].levels, f[i].level)) return MIC_ERR_ARGS;
        t.add(f[i].rows, f[i].cols, f[i].levels, f[i].level, f[i].px_off);
        b[(size_t)i] = f[i].begin; e[(size_t)i] = f[i].end;
    }
    std::vector<int32_t> sv;
    const int rc = wv_decompress_core(s, d_comp, d_out, t, b.data(), e.data(), sv, syms, redone);
    if (rc == MIC_OK) std::copy(sv.begin(), sv.end(), st);
    return rc;
}

}  // namespace micapi

namespace {

size_t wv_frames_per_batch(size_t n) { return std::max<size_t>(1, kWorkspaceBudget / (unit_ws_bytes(2 * n + 16) + 8 * n)); }

}  // namespace

extern "C" {

// WaveletV2RLEFSECompressU16 over nframes frames of one shape in one launch chain (the reference codes one image per call; a
// WaveletV2 file is ONE serial FSE stream, so the GPU only pays off when many frames are coded side by side).
// frames: nframes x rows*cols u16, contiguous.  Frame i's file goes to out + i * out_stride, its length to out_lens[i], its
// status to status[i] (a frame that fails does not stop the others).
int mic_hip_wavelet_v2_compress_batch(const uint16_t *frames, int nframes, int rows, int cols, uint16_t max_value, int levels,
                                      uint8_t *out, size_t out_stride, size_t *out_lens, int32_t *status) try {
    if (!frames || !out || !out_lens || !status || nframes <= 0) return MIC_ERR_ARGS;
    if (const int gate = wv_check_shape(rows, cols)) return gate;
    const size_t n = (size_t)rows * (size_t)cols;
    if (out_stride < 11) return MIC_ERR_CAPACITY;
    const int applied = wv_levels_applied(rows, cols, levels);
    return over_devices(nframes, [n](int) { return (uint64_t)n; }, [&](mic_hip_session *s, int fa, int fb) -> int {   // frames [fa, fb) on one session
        int rc;
        const size_t per = wv_frames_per_batch(n);
        for (size_t f0 = (size_t)fa; f0 < (size_t)fb; f0 += per) {
            const int nf = (int)std::min(per, (size_t)fb - f0);
            if ((rc = s->ensure(nf, 2 * n + 16))) return rc;
            if ((rc = s->io_px.reserve(n * 2 * (size_t)nf + 64))) return rc;
            HIP_TRY(hipMemcpyAsync(s->io_px.p, frames + f0 * n, n * 2 * (size_t)nf, hipMemcpyHostToDevice, s->stream));
            std::vector<std::vector<uint8_t>> blobs; std::vector<int32_t> st;
            if ((rc = wv_compress_frames(s, (const uint16_t *)s->io_px.p, nf, rows, cols, applied, &blobs, st))) return rc;
            for (int i = 0; i < nf; i++) {
                uint8_t *o = out + (f0 + (size_t)i) * out_stride;
                status[f0 + (size_t)i] = st[(size_t)i]; out_lens[f0 + (size_t)i] = 0;
                if (st[(size_t)i] != MIC_OK) continue;
                if (11 + blobs[(size_t)i].size() > out_stride) { status[f0 + (size_t)i] = MIC_ERR_CAPACITY; continue; }
                wv_put_header(o, rows, cols, max_value, applied);
                memcpy(o + 11, blobs[(size_t)i].data(), blobs[(size_t)i].size());
                out_lens[f0 + (size_t)i] = 11 + blobs[(size_t)i].size();
            }
        }
        return MIC_OK;
    });
} MIC_ABI_CATCH

// WaveletV2RLEFSECompressU16 / WaveletV2SIMDRLEFSECompressU16 (waveletfsecompressu16.go:303, :374)
int mic_hip_wavelet_v2_compress(const uint16_t *pixels, int rows, int cols, uint16_t max_value, int levels,
                                uint8_t *out, size_t out_cap, size_t *out_len) try {
    if (!pixels || !out || !out_len || rows <= 0 || cols <= 0) return MIC_ERR_ARGS;
    if (out_cap < 11) return MIC_ERR_CAPACITY;
    size_t len = 0; int32_t st = 0;
    const int rc = mic_hip_wavelet_v2_compress_batch(pixels, 1, rows, cols, max_value, levels, out, out_cap, &len, &st);
    if (rc) return rc;
    if (st != MIC_OK) return st;
    *out_len = len;
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_wavelet_v2_info(const uint8_t *c, size_t len, int *rows, int *cols, int *max_value, int *levels) try {
    if (!c) return MIC_ERR_ARGS;
    if (len < 11) return MIC_ERR_CORRUPT;                                                   // :494-496
    if (rows) *rows = (int)((uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24));
    if (cols) *cols = (int)((uint32_t)c[4] | ((uint32_t)c[5] << 8) | ((uint32_t)c[6] << 16) | ((uint32_t)c[7] << 24));
    if (max_value) *max_value = c[8] | (c[9] << 8);
    if (levels) *levels = c[10];
    return MIC_OK;
} MIC_ABI_CATCH

}  // extern "C"

namespace {
// WaveletV2RLEFSEDecompressU16 over nframes files of ONE shape at resolution `level` (0: the full image): the batch entry points below
int wv_decompress_files(const uint8_t *const *files, const size_t *lens, int nframes, int level, uint16_t *pixels_out, size_t out_cap_px,
                        int32_t *status, uint64_t *syms) {
    if (!files || !lens || !pixels_out || !status || nframes <= 0) return MIC_ERR_ARGS;
    if (syms) for (int i = 0; i < nframes; i++) syms[i] = 0;
    int rows, cols, maxv, levels;
    int rc = mic_hip_wavelet_v2_info(files[0], lens[0], &rows, &cols, &maxv, &levels);
    if (rc) return rc;
    if (rows <= 0 || cols <= 0 || levels > 8) return MIC_ERR_CORRUPT;
    if (level < 0 || level > levels) return MIC_ERR_ARGS;
    if ((rc = wv_check_shape(rows, cols))) return rc;
    const size_t n = (size_t)rows * (size_t)cols;
    const WvDims dm = wv_dims(rows, cols, levels);
    const size_t P = (size_t)dm.nr[level] * (size_t)dm.nc[level];          // pixels of a frame's output (n at level 0)
    if (P * (size_t)nframes > out_cap_px) return MIC_ERR_CAPACITY;
    return over_devices(nframes, [n](int) { return (uint64_t)n; }, [&](mic_hip_session *s, int fa, int fb) -> int {   // frames [fa, fb) on one session; shape: files[0]'s
        int rc;
        const size_t per = wv_frames_per_batch(n);
        for (size_t f0 = (size_t)fa; f0 < (size_t)fb; f0 += per) {
            const int nf = (int)std::min(per, (size_t)fb - f0);
            std::vector<int> slot((size_t)nf, -1); std::vector<uint64_t> offs(1, 0); int good = 0;   // streams packed back to back
            for (int i = 0; i < nf; i++) {
                const uint8_t *c = files[f0 + (size_t)i]; const size_t len = lens[f0 + (size_t)i];
                int r2, c2, m2, l2;
                status[f0 + (size_t)i] = MIC_OK;
                if (!c) { status[f0 + (size_t)i] = MIC_ERR_ARGS; continue; }
                if (mic_hip_wavelet_v2_info(c, len, &r2, &c2, &m2, &l2) != MIC_OK) { status[f0 + (size_t)i] = MIC_ERR_CORRUPT; continue; }
                if (r2 != rows || c2 != cols || l2 != levels) { status[f0 + (size_t)i] = MIC_ERR_ARGS; continue; }
                if (len < 13 || c[11] != 0xFF || c[12] != 0x04 || len - 11 > 0xFFFFFFF0ull) { status[f0 + (size_t)i] = MIC_ERR_CORRUPT; continue; }   // FSEDecompressU16FourState only, :503
                slot[(size_t)i] = good++; offs.push_back(offs.back() + (len - 11));
            }
            if (!good) continue;
            if ((rc = s->ensure(good, 2 * n + 16))) return rc;
            if ((rc = s->io_comp.reserve((size_t)offs.back() + 64)) || (rc = s->io_px.reserve(P * 2 * (size_t)good + 64))) return rc;
            for (int i = 0; i < nf; i++) if (slot[(size_t)i] >= 0)
                HIP_TRY(hipMemcpyAsync((uint8_t *)s->io_comp.p + offs[(size_t)slot[(size_t)i]], files[f0 + (size_t)i] + 11, lens[f0 + (size_t)i] - 11,
                                       hipMemcpyHostToDevice, s->stream));
            std::vector<int32_t> st; std::vector<uint64_t> sy((size_t)good, 0);
            if ((rc = wv_decode_level_frames(s, (const uint8_t *)s->io_comp.p, (uint16_t *)s->io_px.p, good, offs.data(), rows, cols, levels, level, st,
                                             sy.data()))) return rc;
            for (int i = 0; i < nf; i++) if (slot[(size_t)i] >= 0) {
                const size_t k = (size_t)slot[(size_t)i];
                status[f0 + (size_t)i] = st[k];
                if (syms) syms[f0 + (size_t)i] = sy[k];
                if (st[k] == MIC_OK)
                    HIP_TRY(hipMemcpyAsync(pixels_out + (f0 + (size_t)i) * P, (uint16_t *)s->io_px.p + k * P, P * 2, hipMemcpyDeviceToHost, s->stream));
            }
            HIP_TRY(hipStreamSynchronize(s->stream));
        }
        return MIC_OK;
    });
}
}  // namespace

extern "C" {

// WaveletV2RLEFSEDecompressU16 over nframes files of ONE shape (same rows, cols, levels) in one launch chain; pixels_out receives
// nframes x rows*cols u16, status[i] frame i's status.  Files of another shape than the first: MIC_ERR_ARGS for that frame.
int mic_hip_wavelet_v2_decompress_batch(const uint8_t *const *files, const size_t *lens, int nframes, uint16_t *pixels_out, size_t out_cap_px,
                                        int32_t *status) try {
    return wv_decompress_files(files, lens, nframes, 0, pixels_out, out_cap_px, status, nullptr);
} MIC_ABI_CATCH

// ---- the image at reduced resolution ("WaveletV2 at reduced resolution") --------------------------------------
// Level r of a file whose header carries `levels`: the nr[r] x nc[r] LL band the forward transform holds after r levels (nr[0] = rows,
// nr[l + 1] = (nr[l] + 1) / 2, nc alike), saturated to [0, 65535]; r = 0 is the decode itself.  Only the first nr[r] * nc[r] coefficients
// of the subband scan are needed, and the tANS chain stops after the symbols that hold them (wv_decode_level_frames), so a preview
// validates only the part of the stream it decodes.
int mic_hip_wavelet_v2_level_info(const uint8_t *c, size_t len, int level, int *out_rows, int *out_cols) try {
    int rows, cols, levels;
    const int rc = mic_hip_wavelet_v2_info(c, len, &rows, &cols, nullptr, &levels);
    if (rc) return rc;
    if (rows <= 0 || cols <= 0 || levels > 8) return MIC_ERR_CORRUPT;
    if (level < 0 || level > levels) return MIC_ERR_ARGS;
    const WvDims d = wv_dims(rows, cols, levels);
    if (out_rows) *out_rows = d.nr[level];
    if (out_cols) *out_cols = d.nc[level];
    return MIC_OK;
} MIC_ABI_CATCH

// mic_hip_wavelet_v2_decompress_batch at `level`: frame i's band goes to pixels_out + i * nr[level] * nc[level]; symbols_decoded
// (nullable): the tANS symbols the chain decoded per frame, both passes summed
int mic_hip_wavelet_v2_decompress_level_batch(const uint8_t *const *files, const size_t *lens, int nframes, int level, uint16_t *pixels_out,
                                              size_t out_cap_px, int32_t *status, uint64_t *symbols_decoded) try {
    return wv_decompress_files(files, lens, nframes, level, pixels_out, out_cap_px, status, symbols_decoded);
} MIC_ABI_CATCH

int mic_hip_wavelet_v2_decompress_level(const uint8_t *c, size_t len, int level, uint16_t *pixels_out, size_t out_cap_px) try {
    if (!c || !pixels_out) return MIC_ERR_ARGS;
    int32_t st = 0;
    const int rc = mic_hip_wavelet_v2_decompress_level_batch(&c, &len, 1, level, pixels_out, out_cap_px, &st, nullptr);
    return rc ? rc : st;
} MIC_ABI_CATCH

// WaveletV2RLEFSEDecompressU16 / WaveletV2SIMDRLEFSEDecompressU16 (:380-425, :493-534)
int mic_hip_wavelet_v2_decompress(const uint8_t *c, size_t len, uint16_t *pixels_out, size_t out_cap_px) try {
    if (!c || !pixels_out) return MIC_ERR_ARGS;
    int32_t st = 0;
    const int rc = mic_hip_wavelet_v2_decompress_batch(&c, &len, 1, pixels_out, out_cap_px, &st);
    return rc ? rc : st;
} MIC_ABI_CATCH

// ---- device-resident forms (what bench.py times for BASELINE config 3): frames, streams and pixels stay in HBM ----------------
// nframes frames of rows x cols u16, contiguous at d_frames -> their WaveletV2 streams WITHOUT the 11-byte file header (rows, cols,
// maxValue, levels: the caller has them), packed back to back on the device: *d_streams, h_offsets[nframes + 1], h_status[nframes];
// *levels_applied = the level count the header would carry (waveletfsecompressu16.go:321-330).
int mic_hip_session_wavelet_v2_encode(mic_hip_session *s, const uint16_t *d_frames, int nframes, int rows, int cols, int levels,
                                      const uint8_t **d_streams, uint64_t *h_offsets, int32_t *h_status, int *levels_applied) try {
    if (!s || !d_frames || !d_streams || !h_offsets || !h_status || nframes <= 0) return MIC_ERR_ARGS;
    int rc = wv_check_shape(rows, cols);
    if (rc || (rc = s->activate())) return rc;
    const int applied = wv_levels_applied(rows, cols, levels);
    if (levels_applied) *levels_applied = applied;
    std::vector<int32_t> st;
    if ((rc = wv_compress_frames(s, d_frames, nframes, rows, cols, applied, nullptr, st, d_streams, h_offsets))) return rc;
    for (int i = 0; i < nframes; i++) h_status[i] = st[(size_t)i];
    return MIC_OK;
} MIC_ABI_CATCH
// The inverse: nframes header-less streams at d_streams + h_offsets[i] (all of one shape / level count) -> pixels at d_pixels_out.
int mic_hip_session_wavelet_v2_decode(mic_hip_session *s, const uint8_t *d_streams, const uint64_t *h_offsets, int nframes,
                                      int rows, int cols, int levels, uint16_t *d_pixels_out, int32_t *h_status) try {
    if (!s || !d_streams || !h_offsets || !d_pixels_out || !h_status || nframes <= 0) return MIC_ERR_ARGS;
    int rc = wv_check_shape(rows, cols, levels);
    if (rc || (rc = s->activate())) return rc;
    std::vector<int32_t> st;
    if ((rc = wv_decode_level_frames(s, d_streams, d_pixels_out, nframes, h_offsets, rows, cols, levels, 0, st, nullptr))) return rc;
    for (int i = 0; i < nframes; i++) h_status[i] = st[(size_t)i];
    return MIC_OK;
} MIC_ABI_CATCH
// The same at `level` (mic_hip_wavelet_v2_level_info): frame i's nr[level] x nc[level] band to d_pixels_out + i * nr[level] * nc[level];
// h_symbols_decoded (nullable): the tANS symbols the chain decoded per frame, both passes summed.
int mic_hip_session_wavelet_v2_decode_level(mic_hip_session *s, const uint8_t *d_streams, const uint64_t *h_offsets, int nframes,
                                            int rows, int cols, int levels, int level, uint16_t *d_pixels_out,
                                            int32_t *h_status, uint64_t *h_symbols_decoded) try {
    if (!s || !d_streams || !h_offsets || !d_pixels_out || !h_status || nframes <= 0) return MIC_ERR_ARGS;
    int rc = wv_check_shape(rows, cols, levels, level);
    if (rc || (rc = s->activate())) return rc;
    std::vector<int32_t> st;
    if ((rc = wv_decode_level_frames(s, d_streams, d_pixels_out, nframes, h_offsets, rows, cols, levels, level, st, h_symbols_decoded))) return rc;
    for (int i = 0; i < nframes; i++) h_status[i] = st[(size_t)i];
    return MIC_OK;
} MIC_ABI_CATCH

// ---- the same pair over frames of any shapes and level counts, one launch chain (the cores above with the caller's table) ------------
int mic_hip_session_wavelet_v2_encode_mixed(mic_hip_session *s, const uint16_t *d_frames, const uint64_t *h_px_offsets, const int32_t *h_rows_cols,
                                            int nframes, int levels, const uint8_t **d_streams, uint64_t *h_offsets, int32_t *h_status,
                                            int32_t *h_levels_applied) try {
    if (!s || !d_frames || !h_px_offsets || !h_rows_cols || !d_streams || !h_offsets || !h_status || nframes <= 0) return MIC_ERR_ARGS;
    int rc = s->activate();
    if (rc) return rc;
    std::vector<WvEncFrame> F; std::vector<int> at;
    for (int i = 0; i < nframes; i++) {
        const int rows = h_rows_cols[2 * (size_t)i], cols = h_rows_cols[2 * (size_t)i + 1];
        if (h_levels_applied) h_levels_applied[i] = 0;
        if ((h_status[i] = wv_check_shape(rows, cols))) continue;
        F.push_back(WvEncFrame{ h_px_offsets[i], rows, cols, wv_levels_applied(rows, cols, levels) });
        if (h_levels_applied) h_levels_applied[i] = F.back().applied;
        at.push_back(i);
    }
    *d_streams = nullptr;
    for (int i = 0; i <= nframes; i++) h_offsets[i] = 0;
    if (F.empty()) return MIC_OK;
    std::vector<uint64_t> offs(F.size() + 1); std::vector<int32_t> st(F.size());
    if ((rc = wv_encode_run(s, d_frames, F.data(), (int)F.size(), d_streams, offs.data(), st.data()))) return rc;
    size_t k = 0;
    for (int i = 0; i < nframes; i++) {                                   // (a refused frame takes no room between its neighbours' streams)
        h_offsets[i] = offs[k];
        if (k < at.size() && at[k] == i) { h_status[i] = st[k]; k++; }
    }
    h_offsets[nframes] = offs[F.size()];
    return MIC_OK;
} MIC_ABI_CATCH
int mic_hip_session_wavelet_v2_decode_mixed(mic_hip_session *s, const uint8_t *d_streams, const uint64_t *h_offsets, const int32_t *h_rows_cols_levels,
                                            const int32_t *h_level, int nframes, uint16_t *d_pixels_out, const uint64_t *h_out_offsets,
                                            int32_t *h_status, uint64_t *h_symbols_decoded) try {
    if (!s || !d_streams || !h_offsets || !h_rows_cols_levels || !d_pixels_out || !h_out_offsets || !h_status || nframes <= 0) return MIC_ERR_ARGS;
    int rc = s->activate();
    if (rc) return rc;
    std::vector<WvDecFrame> F; std::vector<int> at;
    for (int i = 0; i < nframes; i++) {
        const int32_t *q = h_rows_cols_levels + 3 * (size_t)i;
        const int level = h_level ? h_level[i] : 0;
        if (h_symbols_decoded) h_symbols_decoded[i] = 0;
        if ((h_status[i] = wv_check_shape(q[0], q[1], q[2], level))) continue;
        if (h_offsets[i + 1] < h_offsets[i]) { h_status[i] = MIC_ERR_ARGS; continue; }
        F.push_back(WvDecFrame{ h_offsets[i], h_offsets[i + 1], h_out_offsets[i], q[0], q[1], q[2], level });
        at.push_back(i);
    }
    if (F.empty()) return MIC_OK;
    std::vector<int32_t> st(F.size()); std::vector<uint64_t> sy(F.size(), 0);
    if ((rc = wv_decode_run(s, d_streams, d_pixels_out, F.data(), (int)F.size(), st.data(), sy.data(), nullptr))) return rc;
    for (size_t k = 0; k < at.size(); k++) { h_status[at[k]] = st[k]; if (h_symbols_decoded) h_symbols_decoded[at[k]] = sy[k]; }
    return MIC_OK;
} MIC_ABI_CATCH

}  // extern "C"
