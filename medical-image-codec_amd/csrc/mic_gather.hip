// mic_gather.hip -- what the readers of many rectangles per call share (MIC3 patches: mic_api_ext.hip, MIC2 crops: mic_mic2_crops.hip,
// strip-file crops: mic_strip_crops.hip).  Each of them plans on the host, decodes the touched units in sub-batches into a slab and
// copies the pieces, the (rectangle, unit) overlaps, out of the slab into the output tensor.  Here: the kernels that copy and their
// launcher, the judgement of the output pointer, the crop doors' way to a session, and the packing of a sub-batch's streams.
#include "mic_session.h"
#include "mic_pieces.h"

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

// YCoCgRInverse of the piece's pixels, as k_wsi_planes_to_rgb does it; three byte stores per pixel at whatever byte offset the
// tensor's row has.  src: the piece in plane 0, the other two pstride samples on each; out: u8, three a pixel.  Lanes along x of a
// piece row: a wave reads 64 neighbouring samples of each plane and writes 192 neighbouring bytes.
__global__ void __launch_bounds__(256) k_gather_pieces_rgb(const uint16_t *slab, const GatherPiece *pieces, uint8_t *out) {
    const GatherPiece pc = pieces[blockIdx.x];
    const PieceLanes ln = piece_lanes(pc.w);
    const mic_gp<const uint16_t> py = mic_g(slab + pc.src), pco = py + pc.pstride, pcg = pco + pc.pstride;
    const mic_gp<uint8_t> o = mic_g(out + pc.dst * 3);
    for (int y = ln.row; y < pc.h; y += ln.rstep) {
        const size_t si = (size_t)y * pc.sstride, di = (size_t)y * pc.dstride * 3;
        for (int x = ln.col; x < pc.w; x += ln.lw) {
            const int yv = py[si + x];
            const uint32_t uco = pco[si + x], ucg = pcg[si + x];
            const int co = (int)(int16_t)((uco >> 1) ^ (uint16_t)(-(int)(uco & 1)));       // UnZigZag, deltazigzagcompressu16.go:113-116
            const int cg = (int)(int16_t)((ucg >> 1) ^ (uint16_t)(-(int)(ucg & 1)));
            const int t = yv - (cg >> 1);                                                   // YCoCgRInverse, asm_amd64.go:106-121
            const int g = cg + t;
            const int b = t - (co >> 1);
            const int r = co + b;
            const size_t d = di + (size_t)x * 3;
            o[d] = (uint8_t)r; o[d + 1] = (uint8_t)g; o[d + 2] = (uint8_t)b;
        }
    }
}

}  // namespace

namespace micapi {

void launch_gather(hipStream_t stream, GatherKind kind, const uint16_t *slab, const GatherPiece *pieces, size_t np, int mw, int mh, void *out) {
    constexpr size_t kMaxGridX = 0x7FFFFFFF;
    const unsigned gy = row_chunks(mw, mh);
    for (size_t q = 0; q < np; q += kMaxGridX) {
        const dim3 grid((unsigned)std::min(np - q, kMaxGridX), gy), block(256);
        if (kind == kGatherRGB) hipLaunchKernelGGL(k_gather_pieces_rgb, grid, block, 0, stream, slab, pieces + q, (uint8_t *)out);
        else if (kind == kGatherU16) hipLaunchKernelGGL(k_gather_pieces<uint16_t>, grid, block, 0, stream, slab, pieces + q, (uint16_t *)out);
        else hipLaunchKernelGGL(k_gather_pieces<uint8_t>, grid, block, 0, stream, slab, pieces + q, (uint8_t *)out);
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

int crop_door(mic_hip_session **s, DefaultLease &lease, void **d_out, size_t need) {
    int rc;
    if (!*s) { if ((rc = lease.acquire())) return rc; *s = cur_default(); }
    else if ((rc = (*s)->activate())) return rc;
    rc = patch_pointer(*s, d_out, need);                                                    // judged before anything is launched
    if (rc == MIC_ERR_CAPACITY || ((size_t)*d_out & 1)) rc = MIC_ERR_ARGS;
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
