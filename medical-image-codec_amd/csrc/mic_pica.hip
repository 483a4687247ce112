// mic_pica.hip -- PICA: content-adaptive strips with a per-strip predictor choice (parallelstripsadaptive.go).
//
// CompressParallelStripsAdaptive = adaptiveStripBoundaries (equal-cost partition of the rows by summed |vertical delta|) ->
// every strip coded twice, CompressSingleFrame (avg predictor) and CompressSingleFrameGrad (gradient-adaptive predictor), the
// smaller blob kept (ties: gradient) -> "PICA" header + 16-byte entries {y0, offset, length, flags} + blobs.
// This file holds the device side: the row costs and the boundaries of every image of a sub-batch (two launches, one small
// read-back of the boundaries), and the pick of each strip's winner between the tANS walk and the pack.  The host pipeline that
// drives them -- sub-batches, staging, containers -- is with the other containers' in mic_host_io.hip.
#include "mic_session.h"
#include "mic_wave.h"

namespace {

// rowCost[y] = sum over x of |p[y][x] - p[y-1][x]|, y >= 1 (parallelstripsadaptive.go:236-247).  One group per (image, row) of the
// sub-batch: grid = the table's rows in all, block = 256.  BOUNDS: blockIdx.x < sum of tab[].rows, so the image found has
// y < rows = h and the loads stay inside rows y - 1 and y of it; cost[] has one entry per grid block.
typedef uint16_t pica_u16x4 __attribute__((ext_vector_type(4)));
typedef pica_u16x4 PicaQ __attribute__((aligned(2)));                  // (a row starts at any even address: gfx950 loads it unaligned)
__global__ void __launch_bounds__(256) k_pica_rowcost(const uint16_t *px, const MicPicaImage *tab, int nimg, unsigned long long *cost) {
    int lo = 0, hi = nimg - 1;                                          // the last image whose row0 <= this row
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tab[mid].row0 <= blockIdx.x) lo = mid; else hi = mid - 1; }
    const MicPicaImage im = tab[lo];
    const uint32_t y = blockIdx.x - im.row0;
    if (y >= im.rows) return;
    if (y == 0) { if (threadIdx.x == 0) cost[blockIdx.x] = 0; return; }
    const int w = im.w;
    const mic_gp<const uint16_t> a = mic_g(px) + im.px_off + (size_t)y * (size_t)w, b = a - w;
    unsigned long long sum = 0;
    for (int x = (int)threadIdx.x * 4; x + 4 <= w; x += 1024) {
        const pica_u16x4 va = *(mic_gp<const PicaQ>)(a + x), vb = *(mic_gp<const PicaQ>)(b + x);
        sum += __sad((unsigned)va.x, (unsigned)vb.x, __sad((unsigned)va.y, (unsigned)vb.y, __sad((unsigned)va.z, (unsigned)vb.z, __sad((unsigned)va.w, (unsigned)vb.w, 0u))));
    }
    { const int x = (w & ~3) + (int)threadIdx.x; if (x < w) sum += __sad((unsigned)a[x], (unsigned)b[x], 0u); }
    sum = mic_wave_reduce_add((uint64_t)sum);
    __shared__ unsigned long long s_part[4];
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) cost[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// adaptiveStripBoundaries (parallelstripsadaptive.go:222-289) for every image of the sub-batch: grid = images, block = 256.
// The reference works in float64; the boundaries here equal its exactly, without emulating anything:
//   * every rowCost[y] is an integer, at most 65535 w;
//   * cum[] is a float64 sum of those.  w h <= 2^31 (the entry points refuse more), so every partial sum is an integer below
//     2^47 < 2^53: the float64 sums are exact and equal a u64 prefix sum converted once -- a parallel scan is as good as the
//     reference's serial loop;
//   * target = total * float64(i) / float64(numStrips) is one IEEE multiply, then one IEEE divide: nothing there can contract into
//     an FMA, and fp64 multiply and divide are correctly rounded on gfx950 (__dmul_rn / __ddiv_rn say so to the compiler);
//   * the comparison is cum[mid] < target with cum[mid] converted from the exact integer.
// cum[] is monotone, so the reference's binary search over [starts[i-1] + 1, height) finds max(starts[i-1] + 1, t_i), t_i the first
// row of [1, height) whose cum reaches the target (height when none does): the t_i are found side by side, the running maximum and
// the clamp to height - 1 (:282-284) by one thread.  The two special cases stay: total == 0 gives i * height / numStrips (:262-268),
// numStrips >= height one row per strip (:223-229).
// BOUNDS: cost[row0 .. row0 + h) and starts[start0 .. start0 + nstrips) are the image's own; mid - 1 lies in [0, h - 2].
__global__ void __launch_bounds__(256) k_pica_partition(const MicPicaImage *tab, unsigned long long *cost, int32_t *starts) {
    const MicPicaImage im = tab[blockIdx.x];
    const mic_gp<int32_t> st = mic_g(starts) + im.start0;
    const int n = im.nstrips, h = im.h, tid = (int)threadIdx.x;
    if (n >= h) { for (int i = tid; i < h; i += 256) st[i] = i; return; }
    if (n == 1) { if (tid == 0) st[0] = 0; return; }
    const mic_gp<unsigned long long> c = mic_g(cost) + im.row0;         // becomes the inclusive prefix sum: cum[mid] = c[mid - 1]
    __shared__ unsigned long long s_part[256];
    const int per = (int)(((unsigned)h + 255u) / 256u), lo = (int)min((long long)h, (long long)tid * per), hi = (int)min((long long)h, (long long)lo + per);   // (h up to 2^31 - 1: w = 1)
    unsigned long long run = 0;
    for (int i = lo; i < hi; i++) run += c[i];
    s_part[tid] = run;
    __syncthreads();
    if (tid == 0) { unsigned long long r = 0; for (int i = 0; i < 256; i++) { const unsigned long long v = s_part[i]; s_part[i] = r; r += v; } }
    __syncthreads();
    run = s_part[tid];
    for (int i = lo; i < hi; i++) { run += c[i]; c[i] = run; }
    __threadfence(); __syncthreads();                                   // (the sums are read by other threads of the group)
    const unsigned long long total = c[h - 1];
    if (total == 0) { for (int i = tid; i < n; i += 256) st[i] = (int32_t)((long long)i * h / n); return; }
    const double tot = (double)total;
    for (int i = tid; i < n; i += 256) {
        int l = 0;
        if (i > 0) {
            const double target = __ddiv_rn(__dmul_rn(tot, (double)i), (double)n);
            int r = h; l = 1;
            while (l < r) { const int mid = (l + r) >> 1; if ((double)c[mid - 1] < target) l = mid + 1; else r = mid; }
        }
        st[i] = l;
    }
    __threadfence(); __syncthreads();
    if (tid == 0) {
        int prev = 0;
        for (int i = 1; i < n; i++) { int v = max((int)st[i], prev + 1); if (v >= h) v = h - 1; st[i] = v; prev = v; }
    }
}

// The predictor of every strip (parallelstripsadaptive.go:95-103), between the tANS walk -- which knows each candidate's final size --
// and the offset scan: units 2 p (avg) and 2 p + 1 (gradient) are strip p's candidates; the gradient one is kept when it succeeded
// and is not longer (or the avg one failed), and the other is marked skip_pack.  When both failed neither is packed anyway.
// One thread per strip; BOUNDS: p < npairs, the batch holds 2 npairs units.
__global__ void __launch_bounds__(256) k_pica_pick(MicUnit *units, int npairs) {
    const int p = (int)(blockIdx.x * 256 + threadIdx.x);
    if (p >= npairs) return;
    MicUnit &a = units[2 * p], &g = units[2 * p + 1];
    const bool grad = g.status == MICD_OK && (a.status != MICD_OK || g.blob_len <= a.blob_len);
    (grad ? a : g).skip_pack = 1u;
}

}  // namespace

void mic_launch_pica_bounds(const uint16_t *d_px, const MicPicaImage *d_tab, int nimg, uint32_t rows, unsigned long long *d_cost,
                            int32_t *d_starts, hipStream_t stream, MicTimer *t) {
    if (t) t->mark("k_pica_rowcost");
    if (rows) hipLaunchKernelGGL(k_pica_rowcost, dim3(rows), dim3(256), 0, stream, d_px, d_tab, nimg, d_cost);
    if (t) t->mark("k_pica_partition");
    hipLaunchKernelGGL(k_pica_partition, dim3((unsigned)nimg), dim3(256), 0, stream, d_tab, d_cost, d_starts);
    if (t) t->mark("end");
}
void mic_launch_pica_pick(MicUnit *d_units, int npairs, hipStream_t stream, MicTimer *t) {
    if (t) t->mark("k_pica_pick");
    hipLaunchKernelGGL(k_pica_pick, dim3((unsigned)(npairs + 255) / 256), dim3(256), 0, stream, d_units, npairs);
    if (t) t->mark("end");
}

namespace micapi {
// adaptiveStripBoundaries, parallelstripsadaptive.go:222-289 -- the rule as the reference states it: float64 throughout, evaluated in
// its order.  k_pica_partition is tested against it (mic_hip_pica_boundaries).
std::vector<int> pica_boundaries(const std::vector<unsigned long long> &cost, int height, int num_strips) {
    std::vector<int> starts;
    if (num_strips >= height) { for (int i = 0; i < height; i++) starts.push_back(i); return starts; }
    if (num_strips == 1) return std::vector<int>(1, 0);
    std::vector<double> cum((size_t)height + 1, 0.0);
    for (int y = 0; y < height; y++) cum[(size_t)y + 1] = cum[(size_t)y] + (y ? (double)cost[(size_t)y] : 0.0);
    volatile double total = cum[(size_t)height];
    starts.assign((size_t)num_strips, 0);
    if (total == 0) {
        for (int i = 1; i < num_strips; i++) starts[(size_t)i] = (int)((long long)i * height / num_strips);
        return starts;
    }
    for (int i = 1; i < num_strips; i++) {
        volatile double prod = total * (double)i;
        const double target = prod / (double)num_strips;
        int lo = starts[(size_t)i - 1] + 1, hi = height;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (cum[(size_t)mid] < target) lo = mid + 1; else hi = mid; }
        if (lo >= height) lo = height - 1;
        starts[(size_t)i] = lo;
    }
    return starts;
}

}  // namespace micapi

extern "C" {

// CompressSingleFrameGrad (multiframecompress.go:111-129): gradient-adaptive predictor, two-state FSE, one-state fallback
int mic_hip_compress_frame_grad(const uint16_t *pixels, int width, int height, uint16_t max_value,
                                uint8_t *out, size_t out_cap, size_t *out_len) try {
    if (!pixels || !out || !out_len || width <= 0 || height <= 0) return MIC_ERR_ARGS;
    const size_t npx = (size_t)width * (size_t)height;
    if (npx > ((size_t)1 << 28)) return MIC_ERR_UNSUPPORTED;
    DefaultLease lease;
    int rc = lease.acquire();
    if (rc) return rc;
    mic_hip_session *s = cur_default();
    if ((rc = s->ensure(1, npx))) return rc;
    if ((rc = s->io_px.reserve(npx * 2 + 64))) return rc;
    HIP_TRY(hipMemcpyAsync(s->io_px.p, pixels, npx * 2, hipMemcpyHostToDevice, s->stream));
    const mic_hip_unit unit{ 0, width, height, max_value, (uint16_t)(2 | MIC_HIP_PRED_GRAD) };
    if ((rc = session_encode_enqueue(s, (const uint16_t *)s->io_px.p, &unit, 1))) return rc;
    uint64_t offs[2]; int32_t st, ns; const uint8_t *d_blobs = nullptr;
    if ((rc = session_encode_finish(s, &d_blobs, offs, &st, &ns))) return rc;
    if (st != MIC_OK) return st;
    const size_t len = (size_t)(offs[1] - offs[0]);
    if (len > out_cap) return MIC_ERR_CAPACITY;
    HIP_TRY(hipMemcpy(out, d_blobs + offs[0], len, hipMemcpyDeviceToHost));
    *out_len = len;
    return MIC_OK;
} MIC_ABI_CATCH

// DecompressSingleFrameGrad (multiframecompress.go:132-142)
int mic_hip_decompress_frame_grad(const uint8_t *c, size_t len, uint16_t *pixels_out, int width, int height) try {
    if (!c || !pixels_out || width <= 0 || height <= 0) return MIC_ERR_ARGS;
    if (len == 0) return MIC_ERR_CORRUPT;
    const size_t npx = (size_t)width * (size_t)height;
    if (npx > ((size_t)1 << 28) || len > 0xFFFFFFF0ull) return MIC_ERR_UNSUPPORTED;
    DefaultLease lease;
    int rc = lease.acquire();
    if (rc) return rc;
    mic_hip_session *s = cur_default();
    if ((rc = s->ensure(1, npx))) return rc;
    if ((rc = s->io_px.reserve(npx * 2 + 64))) return rc;
    if ((rc = s->io_comp.reserve(len + 64))) return rc;
    HIP_TRY(hipMemcpyAsync(s->io_comp.p, c, len, hipMemcpyHostToDevice, s->stream));
    const mic_hip_unit unit{ 0, width, height, 0, (uint16_t)(2 | MIC_HIP_PRED_GRAD) };
    const uint64_t offs[2] = { 0, len };
    if ((rc = session_decode_enqueue(s, (const uint8_t *)s->io_comp.p, offs, &unit, 1, (uint16_t *)s->io_px.p))) return rc;
    int32_t st;
    if ((rc = session_decode_finish(s, &st))) return rc;
    if (st != MIC_OK) return st;
    HIP_TRY(hipMemcpy(pixels_out, s->io_px.p, npx * 2, hipMemcpyDeviceToHost));
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_pica_info(const uint8_t *c, size_t len, int *width, int *height, int *num_strips) try {
    if (!c) return MIC_ERR_ARGS;
    if (len < 16 || memcmp(c, "PICA", 4) != 0) return MIC_ERR_CORRUPT;                      // :142-144
    const int w = (int)get_u32(c + 4), h = (int)get_u32(c + 8), n = (int)get_u32(c + 12);
    if (n < 0 || (size_t)n > (len - 16) / 16) return MIC_ERR_CORRUPT;                       // truncated header, :150-153
    if (w <= 0 || h <= 0 || n <= 0) return MIC_ERR_CORRUPT;                                 // :154-156
    if (width) *width = w; if (height) *height = h; if (num_strips) *num_strips = n;
    return MIC_OK;
} MIC_ABI_CATCH

}  // extern "C"
