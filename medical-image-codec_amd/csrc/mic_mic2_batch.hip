// mic_mic2_batch.hip -- MIC2: the unit chains of whole volumes.  One temporal volume per call (mic2_temporal_compress / _decompress,
// behind mic_hip_mic2_compress_temporal, mic_hip_mic2_decompress and mic_hip_mic2_decompress_frame) and many volumes per call
// (mic_hip_mic2_compress_batch / _decompress_batch, whose host pipeline is in mic_host_io.hip; mic_hip_session_mic2_encode / _decode;
// mic_hip_mic2_batch_plan; the many-volume calls have no reference counterpart).  Every volume is CompressMultiFrame /
// DecompressMultiFrame (multiframecompress.go:179-261) in the MIC2 container (multiframe.go:49-142).
//
// A temporal volume (flags 0x01 | 0x02, multiframecompress.go:179-224): frame 0 is a spatial frame; frame i > 0 is
// TemporalDeltaEncode(frame i, frame i-1) = ZigZag(cur - prev) (temporaldelta.go:11-23) coded by compressResidualFrame = RleCompressU16
// + FSE 2-state with the 1-state fallback (multiframecompress.go:146-163).  DecompressMultiFrame (:227-261) inverts it frame by frame.
// Both directions are parallel over frames here: the encoder differences ORIGINAL frames, and on the decode side
// frame_i = frame_0 + sum_{j<=i} UnZigZag(res_j)  (mod 2^16) is a running sum along the frame axis, so every residual stream is
// entropy-decoded at once and one kernel accumulates per pixel.
//
// The units of a call's volumes -- volume order, then frame order -- go through the unit codec in sub-batches cut by their sizes
// alone (mic2_batch_cuts: next_strip_cut's rule), so a sub-batch holds frames of independent volumes, frame 0 of temporal ones and
// residual units of any sizes side by side, and a dataset of small volumes is one chain.  Every caller -- the single calls, the
// batches, the crop readers (mic_mic2_crops.hip) -- runs its sub-batches through mic2_batch_encode_units / mic2_batch_decode_units,
// the one place where the MIC2 unit chain is written out.  On the device:
//   k_mic2_residual    one launch over the residual units of a sub-batch whatever their sizes: a tile list of (unit, first pixel)
//                      entries balances a 245-pixel frame against a 15 360-pixel one; every unit brings its own cur / prev pointers.
//   k_mic2_accumulate  frame_i = frame_{i-1} + UnZigZag(res_i) for the temporal volumes a sub-batch holds parts of: a span per
//                      volume says which units, where the carry lies and where the frames go -- straight to their final place.
//   k_mic2_assemble    the session form's files: headers, frame tables and the streams moved to their final byte offsets.
#include <climits>
#include "mic_session.h"
#include "mic_wave.h"
#include "mic_pieces.h"

void mic_launch_rle_expand(MicUnit *d_units, int n, hipStream_t stream, int mode_filter);   // mic_wavelet.hip

namespace {

// ---- encode: residuals ----------------------------------------------------------------------------------------------------------
// A residual unit of the sub-batch: unit `unit` codes ZigZag(cur - prev) over npx pixels (temporaldelta.go:11-23).
struct ResUnit { const uint16_t *cur, *prev; uint32_t unit, npx; };
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kResTile = 2048;                  // pixels a block takes: 256 lanes x 8 pixels, one 16-byte load of each frame

// tiles[b] = (index into res, first pixel of the tile).  The symbols go to the unit's symbol slab, their maximum -- reduced over the
// wave first -- into dec_thr (free on the encode side, zero from lay_out).  Frames whose two pointers are 16-byte aligned are read
// with vector loads; a frame of an odd width behind an odd number of pixels is only 2-byte aligned and takes the scalar path, as
// does the last, partial group of eight of any frame.  (The slab is 256-byte aligned and a group starts at a multiple of 8.)
__global__ void __launch_bounds__(256) k_mic2_residual(MicUnit *units, const ResUnit *__restrict__ res, const uint2 *__restrict__ tiles) {
    const uint2 t = tiles[blockIdx.x];
    const ResUnit r = res[t.x];
    const mic_gp<uint16_t> sym = mic_g(units[r.unit].sym);
    const mic_gp<const uint16_t> cur = mic_g(r.cur), prev = mic_g(r.prev);
    const uint32_t k = t.y + threadIdx.x * 8;
    const bool vec = ((((uintptr_t)r.cur) | ((uintptr_t)r.prev)) & 15u) == 0;
    uint32_t m = 0;
    if (k < r.npx) {
        if (vec && k + 8 <= r.npx) {
            const u32x4 cw = *(mic_gp<const u32x4>)(cur + k), pw = *(mic_gp<const u32x4>)(prev + k);
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t lo = zigzag16((int32_t)(cw[j] & 0xFFFFu) - (int32_t)(pw[j] & 0xFFFFu));
                const uint32_t hi = zigzag16((int32_t)(cw[j] >> 16) - (int32_t)(pw[j] >> 16));
                m = max(m, max(lo, hi));
                o[j] = lo | (hi << 16);
            }
            *(mic_gp<u32x4>)(sym + k) = o;
        } else {
            const uint32_t e = min(k + 8, r.npx);
            for (uint32_t q = k; q < e; q++) {
                const uint32_t z = zigzag16((int32_t)cur[q] - (int32_t)prev[q]);
                sym[q] = (uint16_t)z;
                m = max(m, z);
            }
        }
    }
    m = mic_wave_reduce_max(m);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&units[r.unit].dec_thr, m);
}
// a residual unit's max_value is its largest symbol (multiframecompress.go:146-163)
__global__ void k_mic2_set_max(MicUnit *units, const ResUnit *__restrict__ res, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { MicUnit &u = units[res[i].unit]; u.max_value = (uint16_t)u.dec_thr; }
}

// ---- decode: residual lengths, running sums -------------------------------------------------------------------------------------
// a residual stream must expand to exactly its own frame (multiframecompress.go:170-172)
__global__ void k_mic2_check_units(MicUnit *units, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && units[i].mode == 3 && units[i].status == MICD_OK && units[i].nsym != (uint32_t)units[i].w * (uint32_t)units[i].h) units[i].status = MICD_ERR_CORRUPT;
}

// pixels a block takes: a lane each, which walks the frame axis of its pixel.  The walk is a chain of dependent stores as long as the
// span has frames, so the launch wants lanes, not work per lane: at 1024 pixels a block (four a lane) the one span of a single
// 128 x 512 x 512 volume took 215 us, at 256 it takes 72 us (kernel trace; a batch of sixteen such volumes fills the device either way)
constexpr uint32_t kAccTile = 256;

// tiles[b] = (index into spans, first pixel).  One lane per pixel along the frame axis: consecutive lanes read consecutive symbols of
// a unit and store consecutive samples of a frame.  The sum starts from frame 0, which the span's first unit decoded into dst
// (f0 == 0), or from the carry, and stops in front of the volume's first failed frame.
__global__ void __launch_bounds__(256) k_mic2_accumulate(const MicUnit *__restrict__ units, const Mic2DecSpan *__restrict__ spans, const uint2 *__restrict__ tiles) {
    const uint2 t = tiles[blockIdx.x];
    const Mic2DecSpan v = spans[t.x];
    const MicUnit *vu = units + v.u0;
    const int r0 = v.f0 ? 0 : 1, iend = min(v.nb, v.fbad - v.f0);
    const mic_gp<uint16_t> dst = mic_g(v.dst);
    const uint32_t e = min(t.y + kAccTile, v.npx);
    for (uint32_t k = t.y + threadIdx.x; k < e; k += 256) {
        uint32_t acc = v.f0 ? (uint32_t)mic_g(v.carry)[k] : (uint32_t)dst[k];
        for (int i = r0; i < iend; i++) {
            acc = (acc + unzigzag16(mic_g(vu[i].sym)[k])) & 0xFFFFu;                        // temporaldelta.go:27-37
            dst[(size_t)i * v.npx + k] = (uint16_t)acc;
        }
    }
}

// ---- the session form's files ---------------------------------------------------------------------------------------------------
// A file of the call: header and table at `file` of the destination; its frames are streams first .. first + n - 1.
struct AsmFile { uint64_t file; uint32_t first; int32_t w, h, n, temporal, pad; };
// A stream: len bytes from src (of the source buffer) to dst (of the destination), both at any byte alignment; rel = where it lies
// behind its file's table, the table's entry for it.
struct AsmStream { uint64_t src, dst; uint32_t len, rel; };
constexpr uint32_t kAsmTile = 16384;                 // bytes of a stream a block moves

__device__ __forceinline__ void put_le32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// Blocks 0 .. nfiles - 1 write a file's 20-byte header and its frame table (multiframe.go:49-91); the blocks behind them move
// tiles[b - nfiles] = (stream, first byte): the destination's aligned words are built from two aligned words of the source (the
// source buffers are allocations of the session, 4-byte aligned with slack behind their last stream), its ragged ends byte by byte.
__global__ void __launch_bounds__(256) k_mic2_assemble(const AsmFile *__restrict__ files, int nfiles, const AsmStream *__restrict__ streams,
                                                     const uint2 *__restrict__ tiles, const uint8_t *__restrict__ src, uint8_t *dst) {
    if ((int)blockIdx.x < nfiles) {
        const AsmFile f = files[blockIdx.x];
        uint8_t *o = dst + f.file;
        if (threadIdx.x == 0) {
            o[0] = 'M'; o[1] = 'I'; o[2] = 'C'; o[3] = '2';
            put_le32(o + 4, (uint32_t)f.w); put_le32(o + 8, (uint32_t)f.h); put_le32(o + 12, (uint32_t)f.n);
            o[16] = f.temporal ? (0x01 | 0x02) : 0x01;                                       // PipelineSpatial | PipelineTemporal, multiframe.go:28-29
            o[17] = o[18] = o[19] = 0;
        }
        for (int i = threadIdx.x; i < f.n; i += blockDim.x) {
            const AsmStream st = streams[f.first + (uint32_t)i];
            put_le32(o + 20 + 8 * (size_t)i, st.rel); put_le32(o + 24 + 8 * (size_t)i, st.len);
        }
        return;
    }
    const uint2 t = tiles[blockIdx.x - (uint32_t)nfiles];
    const AsmStream st = streams[t.x];
    const uint64_t d0 = st.dst + t.y, s0 = st.src + t.y;                                    // this block: n bytes from s0 to d0
    const uint32_t n = min(kAsmTile, st.len - t.y);
    const uint32_t head = min(n, (uint32_t)((4 - (d0 & 3)) & 3)), words = (n - head) >> 2, tail = head + 4 * words;
    if (threadIdx.x < head) dst[d0 + threadIdx.x] = src[s0 + threadIdx.x];
    if (threadIdx.x < n - tail) dst[d0 + tail + threadIdx.x] = src[s0 + tail + threadIdx.x];
    const uint64_t sw = s0 + head;                                                          // the source byte of the first whole word
    const uint32_t sh = (uint32_t)(sw & 3) * 8;
    const mic_gp<const uint32_t> s32 = (mic_gp<const uint32_t>)(src + (sw & ~(uint64_t)3));
    const mic_gp<uint32_t> d32 = (mic_gp<uint32_t>)(dst + d0 + head);
    for (uint32_t j = threadIdx.x; j < words; j += 256) {
        const uint32_t lo = s32[j];
        d32[j] = sh ? (lo >> sh) | (s32[j + 1] << (32 - sh)) : lo;
    }
}

// a list of the call on the device, behind the others in s->pieces (reserved by the caller)
template <class T> int put_list(mic_hip_session *s, size_t &at, const std::vector<T> &v, const T **d) {
    at = align_up(at, 16);
    *d = (const T *)((char *)s->pieces.p + at);
    if (!v.empty()) HIP_TRY(hipMemcpyAsync((char *)s->pieces.p + at, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s->stream));
    at += v.size() * sizeof(T);
    return MIC_OK;
}
template <class T> size_t list_bytes(const std::vector<T> &v) { return align_up(v.size() * sizeof(T), 16) + 16; }

}  // namespace

namespace micapi {

std::vector<size_t> mic2_batch_cuts(const std::vector<size_t> &px, size_t budget) {
    std::vector<size_t> cuts{ 0 };
    while (cuts.back() < px.size()) cuts.push_back(next_strip_cut(px, cuts.back(), budget));
    return cuts;
}

int mic2_batch_encode_units(mic_hip_session *s, const Mic2EncUnit *u, int nb, const uint8_t **d_blobs, uint64_t *offs, int32_t *st) {
    if (nb <= 0 || nb > 65535) return MIC_ERR_INTERNAL;
    size_t max_px = 0;
    std::vector<ResUnit> res; std::vector<uint2> tiles;
    for (int i = 0; i < nb; i++) {
        const size_t npx = (size_t)u[i].w * (size_t)u[i].h;
        max_px = std::max(max_px, npx);
        if (!u[i].residual) continue;
        for (size_t k = 0; k < npx; k += kResTile) tiles.push_back(make_uint2((unsigned)res.size(), (unsigned)k));
        res.push_back(ResUnit{ u[i].cur, u[i].cur - npx, (uint32_t)i, (uint32_t)npx });
    }
    int rc;
    s->retry.kind = 0;                                                                      // (laid out here, in tier 2: no second run)
    if ((rc = s->lay_out(nb, max_px))) return rc;
    if ((rc = s->pieces.reserve(list_bytes(res) + list_bytes(tiles)))) return rc;
    size_t at = 0;
    const ResUnit *d_res = nullptr; const uint2 *d_tiles = nullptr;
    if ((rc = put_list(s, at, res, &d_res)) || (rc = put_list(s, at, tiles, &d_tiles))) return rc;
    for (int i = 0; i < nb; i++) {
        MicUnit &m = s->h_units[(size_t)i];
        const size_t npx = (size_t)u[i].w * (size_t)u[i].h;
        m.w = u[i].w; m.h = u[i].h; m.nstates = 2;
        m.tok_cap = (uint32_t)tok_cap_for(npx);                                             // (the unit's own bound, whatever the largest of the sub-batch)
        if (u[i].residual) { m.mode = 2; m.nsym = (uint32_t)npx; m.max_value = 0; }
        else { m.mode = 0; m.px_in = u[i].cur; m.max_value = u[i].max_value; }
    }
    rc = s->run_encode([&] {
        if (!res.empty()) {
            s->timer.mark("k_mic2_residual");
            hipLaunchKernelGGL(k_mic2_residual, dim3((unsigned)tiles.size()), dim3(256), 0, s->stream, (MicUnit *)s->units.p, d_res, d_tiles);
            hipLaunchKernelGGL(k_mic2_set_max, dim3((unsigned)((res.size() + 255) / 256)), dim3(256), 0, s->stream, (MicUnit *)s->units.p, d_res, (int)res.size());
        }
        mic_launch_encode((MicUnit *)s->units.p, nb, s->stream, s->variant, &s->timer);
    });
    if (rc) return rc;
    return session_encode_finish(s, d_blobs, offs, st, nullptr);
}

int mic2_batch_decode_units(mic_hip_session *s, const Mic2DecUnit *u, int nb, int32_t *st) {
    if (nb <= 0 || nb > 65535) return MIC_ERR_INTERNAL;
    size_t max_px = 0;
    for (int i = 0; i < nb; i++) max_px = std::max(max_px, (size_t)u[i].w * (size_t)u[i].h);
    int rc;
    s->retry.kind = 0;                                                                      // (laid out here, in tier 2: no second run)
    if ((rc = s->lay_out(nb, max_px))) return rc;
    bool any_sym = false;
    uint32_t pred_mask = 0;                                                                 // predictor classes (by width) of the sub-batch's frames
    for (int i = 0; i < nb; i++) {
        MicUnit &m = s->h_units[(size_t)i];
        const size_t npx = (size_t)u[i].w * (size_t)u[i].h;
        m.comp_in = u[i].comp; m.comp_len = u[i].len;
        m.w = u[i].w; m.h = u[i].h;
        m.tok_cap = (uint32_t)tok_cap_for(npx);
        m.sym_cap = (uint32_t)std::min<size_t>(tok_cap_for(npx) + 64, 0xFFFFFFF0u);
        if (u[i].residual) { m.mode = 3; any_sym = true; }                                  // FSE + RLE-of-symbols into the symbol slab
        else { m.mode = 0; m.px_out = u[i].out; pred_mask |= mic_pred_bit(m.w); }
    }
    rc = s->run_decode(mic_hip_session::FlagSlab::Clear, [&] {
        mic_launch_decode((MicUnit *)s->units.p, nb, s->stream, s->variant, &s->timer, (int *)s->cls.p, pred_mask, s->dec_classes.mask(), &s->split_cfg);
        if (any_sym) {
            mic_launch_rle_expand((MicUnit *)s->units.p, nb, s->stream, 3);
            hipLaunchKernelGGL(k_mic2_check_units, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s->stream, (MicUnit *)s->units.p, nb);
        }
    });
    if (rc) return rc;
    s->learn_decode = true;                                                                 // (frames and residuals run the same tANS classes)
    return session_decode_finish(s, st);
}

int mic2_batch_accumulate(mic_hip_session *s, const Mic2DecSpan *spans, int nspans) {
    std::vector<Mic2DecSpan> work; std::vector<uint2> tiles;
    for (int q = 0; q < nspans; q++) {
        const Mic2DecSpan &v = spans[q];
        if (std::min(v.nb, v.fbad - v.f0) <= (v.f0 ? 0 : 1)) continue;                      // no residual to add: frame 0 alone, or failed before
        for (size_t k = 0; k < v.npx; k += kAccTile) tiles.push_back(make_uint2((unsigned)work.size(), (unsigned)k));
        work.push_back(v);
    }
    if (work.empty()) return MIC_OK;
    int rc;
    if ((rc = s->pieces.reserve(list_bytes(work) + list_bytes(tiles)))) return rc;
    size_t at = 0;
    const Mic2DecSpan *d_spans = nullptr; const uint2 *d_tiles = nullptr;
    if ((rc = put_list(s, at, work, &d_spans)) || (rc = put_list(s, at, tiles, &d_tiles))) return rc;
    s->timer.reset(s->stream); s->timer.mark("k_mic2_accumulate");
    hipLaunchKernelGGL(k_mic2_accumulate, dim3((unsigned)tiles.size()), dim3(256), 0, s->stream, (const MicUnit *)s->units.p, d_spans, d_tiles);
    s->timer.mark("end");
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MIC_OK;
}

void mic2_write_head(uint8_t *out, int w, int h, int n, bool temporal, const uint32_t *lens) {
    memset(out, 0, 20);
    memcpy(out, "MIC2", 4);
    put_u32(out + 4, (uint32_t)w); put_u32(out + 8, (uint32_t)h); put_u32(out + 12, (uint32_t)n);
    out[16] = temporal ? (0x01 | 0x02) : 0x01;                                              // PipelineSpatial | PipelineTemporal, multiframe.go:28-29
    uint32_t off = 0;
    for (int i = 0; i < n; i++) {
        put_u32(out + 20 + (size_t)i * 8, off); put_u32(out + 24 + (size_t)i * 8, lens[i]);
        off += lens[i];
    }
}

int mic2_batch_parse(const uint8_t *head, size_t head_len, uint64_t file_len, Mic2Head &m) {
    if (!head) return MIC_ERR_ARGS;
    if (head_len < 20) return MIC_ERR_CORRUPT;
    const int rc = mic_hip_mic2_info(head, (size_t)file_len, &m.w, &m.h, &m.n, &m.temporal);
    if (rc) return rc;
    m.file_len = file_len;
    if (m.w <= 0 || m.h <= 0 || m.n <= 0) return MIC_ERR_CORRUPT;                            // (as mic_hip_mic2_decompress)
    if ((size_t)m.w * (size_t)m.h > ((size_t)1 << 28) || file_len > 0xFFFFFFF0ull) return MIC_ERR_UNSUPPORTED;
    if (head_len < 20 + 8 * (size_t)m.n) return MIC_ERR_ARGS;                               // (the table is not all there)
    m.table = head + 20;
    return MIC_OK;
}

// ---- one temporal volume per call -----------------------------------------------------------------------------------------------
// The single calls keep their own transfers -- plain copies of the caller's buffers on the session's stream, no staging pipeline -- and
// run their sub-batches through the cores above.  Encode: a residual needs the ORIGINAL frame before it, so a sub-batch uploads one
// frame more than it codes (its predecessor's last) and is otherwise independent of the others.  Decode: the running sum needs the
// frame before the sub-batch's first residual: it is carried on the device in the slot in front of the sub-batch's frames.
int mic2_temporal_compress(const uint16_t *frames, int width, int height, int nframes, uint16_t max_value,
                           uint8_t *out, size_t out_cap, size_t *out_len) {
    const size_t npx = (size_t)width * (size_t)height;
    if (npx > ((size_t)1 << 28)) return MIC_ERR_UNSUPPORTED;
    const size_t header = 20 + (size_t)nframes * 8;
    if (out_cap < header) return MIC_ERR_CAPACITY;
    DefaultLease lease;
    int rc = lease.acquire();
    if (rc) return rc;
    mic_hip_session *s = cur_default();
    if ((rc = s->ensure(1, 1))) return rc;                                                  // (the session's stream)
    const std::vector<size_t> cuts = mic2_batch_cuts(std::vector<size_t>((size_t)nframes, npx), kWorkspaceBudget);
    std::vector<uint32_t> lens((size_t)nframes);
    std::vector<Mic2EncUnit> eu; std::vector<uint64_t> offs; std::vector<int32_t> st;
    uint64_t total = 0;
    for (size_t b = 0; b + 1 < cuts.size(); b++) {
        const size_t f0 = cuts[b];
        const int nb = (int)(cuts[b + 1] - f0);
        const int lead = f0 ? 1 : 0;                                                        // the frame in front of the sub-batch (its residuals' reference)
        if ((rc = s->io_px.reserve(npx * 2 * (size_t)(nb + lead)))) return rc;
        HIP_TRY(hipMemcpyAsync(s->io_px.p, frames + (f0 - (size_t)lead) * npx, npx * 2 * (size_t)(nb + lead), hipMemcpyHostToDevice, s->stream));
        eu.resize((size_t)nb); offs.resize((size_t)nb + 1); st.resize((size_t)nb);
        for (int i = 0; i < nb; i++)
            eu[(size_t)i] = Mic2EncUnit{ (const uint16_t *)s->io_px.p + (size_t)(lead + i) * npx, width, height, max_value, (uint16_t)(f0 + (size_t)i > 0) };
        const uint8_t *d_blobs = nullptr;
        if ((rc = mic2_batch_encode_units(s, eu.data(), nb, &d_blobs, offs.data(), st.data()))) return rc;
        for (int i = 0; i < nb; i++) if (st[(size_t)i] != MIC_OK) return st[(size_t)i];
        const uint64_t bytes = offs[(size_t)nb];
        if (total + bytes > 0xFFFFFFFFull) return MIC_ERR_UNSUPPORTED;                      // u32 offsets, multiframe.go:75-80
        if (out_cap < header + total + bytes) return MIC_ERR_CAPACITY;
        for (int i = 0; i < nb; i++) lens[f0 + (size_t)i] = (uint32_t)(offs[(size_t)i + 1] - offs[(size_t)i]);
        if (bytes) HIP_TRY(hipMemcpy(out + header + total, d_blobs, (size_t)bytes, hipMemcpyDeviceToHost));
        total += bytes;
    }
    mic2_write_head(out, width, height, nframes, true, lens.data());
    *out_len = header + (size_t)total;
    return MIC_OK;
}

// frames 0 .. n-1 of the n_total the file holds (mic_hip_mic2_decompress_frame stops at the frame it is asked for)
int mic2_temporal_decompress(const uint8_t *c, size_t len, int w, int h, int n_total, int n, uint16_t *frames_out) {
    const size_t npx = (size_t)w * (size_t)h;
    if (npx > ((size_t)1 << 28) || len > 0xFFFFFFF0ull) return MIC_ERR_UNSUPPORTED;
    const size_t data_off = 20 + (size_t)n_total * 8;
    DefaultLease lease;
    int rc = lease.acquire();
    if (rc) return rc;
    mic_hip_session *s = cur_default();
    if ((rc = s->ensure(1, 1))) return rc;                                                  // (the session's stream)
    const std::vector<size_t> cuts = mic2_batch_cuts(std::vector<size_t>((size_t)n, npx), kWorkspaceBudget);
    std::vector<Mic2DecUnit> du; std::vector<int32_t> st;
    for (size_t b = 0; b + 1 < cuts.size(); b++) {
        const size_t f0 = cuts[b];
        const int nb = (int)(cuts[b + 1] - f0);
        const int lead = f0 ? 1 : 0;                                                        // slot 0 holds the frame in front of the sub-batch
        if ((rc = s->io_px.reserve(npx * 2 * (size_t)(nb + 1)))) return rc;                 // (grown before the carry below could be lost: sized for the first pass too)
        size_t c0 = (size_t)-1, c1 = 0;                                                     // byte range of the sub-batch's streams
        for (int i = 0; i < nb; i++) {
            const size_t fi = f0 + (size_t)i;
            const size_t start = data_off + get_u32(c + 20 + fi * 8), bl = get_u32(c + 24 + fi * 8);
            if (start + bl > len) return MIC_ERR_CORRUPT;                                   // multiframe.go:137-139
            if (bl == 0) return MIC_ERR_CORRUPT;
            c0 = std::min(c0, start); c1 = std::max(c1, start + bl);
        }
        if ((rc = s->io_comp.reserve(c1 - c0 + 64))) return rc;
        HIP_TRY(hipMemcpyAsync(s->io_comp.p, c + c0, c1 - c0, hipMemcpyHostToDevice, s->stream));
        // frames of the sub-batch at slots lead .. lead + nb - 1; slot 0 = frame f0 - 1 (carried) when lead
        uint16_t *d_frames = (uint16_t *)s->io_px.p;
        du.resize((size_t)nb); st.resize((size_t)nb);
        for (int i = 0; i < nb; i++) {
            const size_t fi = f0 + (size_t)i;
            du[(size_t)i] = Mic2DecUnit{ (const uint8_t *)s->io_comp.p + (data_off + get_u32(c + 20 + fi * 8) - c0), get_u32(c + 24 + fi * 8), w, h,
                                         fi ? nullptr : d_frames, (uint32_t)(fi > 0) };     // (frame 0 decodes into slot 0)
        }
        if ((rc = mic2_batch_decode_units(s, du.data(), nb, st.data()))) return rc;
        for (int i = 0; i < nb; i++) if (st[(size_t)i] != MIC_OK) return st[(size_t)i];
        const Mic2DecSpan span{ d_frames, d_frames + (size_t)lead * npx, (uint32_t)npx, 0, nb, (int32_t)f0, INT_MAX, 0 };
        if ((rc = mic2_batch_accumulate(s, &span, 1))) return rc;
        HIP_TRY(hipMemcpyAsync(frames_out + f0 * npx, d_frames + (size_t)lead * npx, npx * 2 * (size_t)nb, hipMemcpyDeviceToHost, s->stream));
        if (f0 + (size_t)nb < (size_t)n && lead + nb - 1 != 0)                              // carry the last frame to slot 0 for the next sub-batch
            HIP_TRY(hipMemcpyAsync(d_frames, d_frames + (size_t)(lead + nb - 1) * npx, npx * 2, hipMemcpyDeviceToDevice, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    return MIC_OK;
}

}  // namespace micapi

namespace {

// the buffer grows and keeps its first `keep` bytes (DevBuf::reserve alone forgets them); everything queued on the stream has completed
int grow_keep(DevBuf &b, size_t bytes, size_t keep, hipStream_t stream) {
    if (bytes <= b.cap) return MIC_OK;
    DevBuf nb;
    int rc = nb.reserve(bytes + bytes / 2);
    if (rc) return rc;
    if (keep) {
        HIP_TRY(hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    b.release();
    b.p = nb.p; b.cap = nb.cap;
    return MIC_OK;
}

// a volume of a session call whose arguments stand
struct SessVol { int job; int32_t w, h, n, temporal; size_t unit0; int32_t status = MIC_OK, failed = -1; };

}  // namespace

extern "C" {

int mic_hip_mic2_batch_plan(const int32_t *whn, int nvol, size_t budget_bytes,
                            uint32_t *cuts, size_t cap, uint64_t *ncuts, uint64_t *nunits) try {
    if (nvol < 0 || (nvol > 0 && !whn) || (cap > 0 && !cuts)) return MIC_ERR_ARGS;
    std::vector<size_t> px;
    for (int v = 0; v < nvol; v++) {
        const int32_t w = whn[3 * (size_t)v], h = whn[3 * (size_t)v + 1], n = whn[3 * (size_t)v + 2];
        if (w <= 0 || h <= 0 || n <= 0) return MIC_ERR_ARGS;
        px.insert(px.end(), (size_t)n, (size_t)w * (size_t)h);
    }
    if (px.size() > 0xFFFFFFFFull) return MIC_ERR_UNSUPPORTED;
    const std::vector<size_t> c = mic2_batch_cuts(px, budget_bytes ? budget_bytes : kWorkspaceBudget);
    if (!budget_bytes) (void)hipGetLastError();                                             // (the default ceiling asks the device when there is one)
    if (ncuts) *ncuts = c.size();
    if (nunits) *nunits = px.size();
    if (c.size() > cap) return MIC_ERR_CAPACITY;
    for (size_t i = 0; i < c.size(); i++) cuts[i] = (uint32_t)c[i];
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_session_mic2_encode(mic_hip_session *s, const uint16_t *d_frames, const mic_hip_mic2_volume *vols, int n,
                                const uint8_t **d_files, uint64_t *h_offsets, uint8_t *h_heads, size_t heads_cap,
                                int32_t *status, int32_t *failed_frame, mic_hip_mic2_batch_stats *stats) try {
    if (!s || n < 0 || !d_files || !h_offsets || (n > 0 && (!vols || !d_frames))) return MIC_ERR_ARGS;
    if (stats) *stats = mic_hip_mic2_batch_stats{ 0, 0, 0 };
    *d_files = nullptr;
    for (int v = 0; v <= n; v++) h_offsets[v] = 0;
    std::vector<int32_t> vst((size_t)n, MIC_OK), vff((size_t)n, -1);
    auto report = [&] {
        for (int v = 0; v < n; v++) { if (status) status[v] = vst[(size_t)v]; if (failed_frame) failed_frame[v] = vff[(size_t)v]; }
    };
    std::vector<SessVol> V; std::vector<Mic2EncUnit> U; std::vector<size_t> px;
    size_t heads_need = 0;
    for (int v = 0; v < n; v++) {
        const mic_hip_mic2_volume &j = vols[v];
        if (j.width <= 0 || j.height <= 0 || j.nframes <= 0 || j.temporal > 1) { vst[(size_t)v] = MIC_ERR_ARGS; continue; }
        const size_t npx = (size_t)j.width * (size_t)j.height;
        if (npx > ((size_t)1 << 28)) { vst[(size_t)v] = MIC_ERR_UNSUPPORTED; continue; }
        V.push_back(SessVol{ v, j.width, j.height, j.nframes, j.temporal, U.size() });
        for (int f = 0; f < j.nframes; f++) {
            U.push_back(Mic2EncUnit{ d_frames + j.px_off + (size_t)f * npx, j.width, j.height, j.max_value, (uint16_t)(j.temporal && f > 0) });
            px.push_back(npx);
        }
        heads_need += 20 + 8 * (size_t)j.nframes;
    }
    if (h_heads && heads_cap < heads_need) return MIC_ERR_CAPACITY;
    report();
    if (U.empty()) return MIC_OK;
    int rc = s->activate();
    if (rc) return rc;
    if ((rc = s->ensure(1, 1))) return rc;                                                  // (the session's stream)
    const std::vector<size_t> cuts = mic2_batch_cuts(px, kWorkspaceBudget);
    const bool one = cuts.size() == 2;                                                      // one chain: its packed streams are the assembler's source as they lie
    // the streams of the sub-batches, back to back in unit order; a unit that failed has none
    std::vector<uint64_t> src(U.size(), 0); std::vector<uint32_t> len(U.size(), 0); std::vector<int32_t> ust(U.size(), MIC_OK);
    uint64_t total = 0;
    const uint8_t *d_src = nullptr;
    for (size_t b = 0; b + 1 < cuts.size(); b++) {
        const size_t u0 = cuts[b];
        const int nb = (int)(cuts[b + 1] - u0);
        std::vector<uint64_t> offs((size_t)nb + 1);
        const uint8_t *d_blobs = nullptr;
        if ((rc = mic2_batch_encode_units(s, U.data() + u0, nb, &d_blobs, offs.data(), ust.data() + u0))) return rc;
        for (int i = 0; i < nb; i++) { src[u0 + (size_t)i] = total + offs[(size_t)i]; len[u0 + (size_t)i] = (uint32_t)(offs[(size_t)i + 1] - offs[(size_t)i]); }
        const uint64_t bytes = offs[(size_t)nb];
        if (one) d_src = d_blobs;
        else {
            if ((rc = grow_keep(s->mic2_payload, (size_t)(total + bytes) + 64, (size_t)total, s->stream))) return rc;
            if (bytes) HIP_TRY(hipMemcpyAsync((uint8_t *)s->mic2_payload.p + total, d_blobs, (size_t)bytes, hipMemcpyDeviceToDevice, s->stream));
            HIP_TRY(hipStreamSynchronize(s->stream));                                       // (the next chain packs into the buffer this copy reads)
            d_src = (const uint8_t *)s->mic2_payload.p;
        }
        total += bytes;
    }
    // every volume's fate, then the scan over the lengths: where each file and each of its streams goes
    std::vector<AsmFile> files; std::vector<AsmStream> streams; std::vector<uint2> tiles;
    uint64_t at = 0;
    size_t hat = 0;
    uint64_t done = 0;
    for (SessVol &sv : V) {
        uint64_t payload = 0;
        for (int f = 0; f < sv.n && sv.status == MIC_OK; f++) {
            if (ust[sv.unit0 + (size_t)f] != MIC_OK) { sv.status = ust[sv.unit0 + (size_t)f]; sv.failed = f; }
            payload += len[sv.unit0 + (size_t)f];
        }
        if (sv.status == MIC_OK && payload > 0xFFFFFFFFull) sv.status = MIC_ERR_UNSUPPORTED;   // u32 offsets, multiframe.go:75-80
        vst[(size_t)sv.job] = sv.status; vff[(size_t)sv.job] = sv.failed;
        h_offsets[sv.job] = at;
        if (sv.status != MIC_OK) continue;
        done++;
        const size_t header = 20 + 8 * (size_t)sv.n;
        files.push_back(AsmFile{ at, (uint32_t)streams.size(), sv.w, sv.h, sv.n, sv.temporal, 0 });
        if (h_heads) { mic2_write_head(h_heads + hat, sv.w, sv.h, sv.n, sv.temporal != 0, len.data() + sv.unit0); hat += header; }
        uint64_t rel = 0;
        for (int f = 0; f < sv.n; f++) {
            const size_t g = sv.unit0 + (size_t)f;
            for (uint32_t k = 0; k < len[g]; k += kAsmTile) tiles.push_back(make_uint2((unsigned)streams.size(), k));
            streams.push_back(AsmStream{ src[g], at + header + rel, len[g], (uint32_t)rel });
            rel += len[g];
        }
        at += header + rel;
    }
    {   // h_offsets: file v at [v] .. [v + 1]; a volume that wrote nothing has an empty range where the next file starts
        uint64_t next = at;
        h_offsets[n] = at;
        for (int v = n - 1; v >= 0; v--) { if (vst[(size_t)v] != MIC_OK) h_offsets[v] = next; next = h_offsets[v]; }
    }
    report();
    if (!files.empty()) {
        if ((rc = s->mic2_files.reserve((size_t)at + 64))) return rc;
        if ((rc = s->pieces.reserve(list_bytes(files) + list_bytes(streams) + list_bytes(tiles)))) return rc;
        size_t lat = 0;
        const AsmFile *d_f = nullptr; const AsmStream *d_s = nullptr; const uint2 *d_t = nullptr;
        if ((rc = put_list(s, lat, files, &d_f)) || (rc = put_list(s, lat, streams, &d_s)) || (rc = put_list(s, lat, tiles, &d_t))) return rc;
        s->timer.reset(s->stream); s->timer.mark("k_mic2_assemble");
        hipLaunchKernelGGL(k_mic2_assemble, dim3((unsigned)(files.size() + tiles.size())), dim3(256), 0, s->stream,
                           d_f, (int)files.size(), d_s, d_t, d_src, (uint8_t *)s->mic2_files.p);
        s->timer.mark("end");
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s->stream));
        *d_files = (const uint8_t *)s->mic2_files.p;
    }
    if (stats) *stats = mic_hip_mic2_batch_stats{ U.size(), cuts.size() - 1, done };
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_session_mic2_decode(mic_hip_session *s, const uint8_t *const *heads, const size_t *head_lens,
                                const uint8_t *const *d_files, const size_t *lens, int n,
                                uint16_t *d_frames_out, const uint64_t *px_off, size_t out_cap_px,
                                int32_t *status, int32_t *failed_frame, mic_hip_mic2_batch_stats *stats) try {
    if (!s || n < 0 || (n > 0 && (!heads || !head_lens || !d_files || !lens || !px_off || !d_frames_out))) return MIC_ERR_ARGS;
    if (stats) *stats = mic_hip_mic2_batch_stats{ 0, 0, 0 };
    std::vector<int32_t> vst((size_t)n, MIC_OK), vff((size_t)n, -1);
    auto report = [&] {
        for (int v = 0; v < n; v++) { if (status) status[v] = vst[(size_t)v]; if (failed_frame) failed_frame[v] = vff[(size_t)v]; }
    };
    struct Unit { uint32_t vol, frame; };                                                   // vol: index into V
    std::vector<SessVol> V; std::vector<Mic2Head> M; std::vector<Unit> un; std::vector<size_t> px;
    for (int v = 0; v < n; v++) {
        Mic2Head m;
        int code = mic2_batch_parse(heads[v], head_lens[v], lens[v], m);
        if (code == MIC_OK && !d_files[v]) code = MIC_ERR_ARGS;
        const size_t npx = (size_t)m.w * (size_t)m.h;
        if (code == MIC_OK && (px_off[v] > out_cap_px || npx * (size_t)m.n > out_cap_px - px_off[v])) code = MIC_ERR_CAPACITY;
        for (int f = 0; f < m.n && code == MIC_OK; f++) {                                   // as mic_hip_mic2_decompress, multiframe.go:137-139
            const uint64_t off = 20 + 8 * (uint64_t)m.n + get_u32(m.table + 8 * (size_t)f), bl = get_u32(m.table + 8 * (size_t)f + 4);
            if (bl == 0 || off + bl > m.file_len) { code = MIC_ERR_CORRUPT; vff[(size_t)v] = f; }
        }
        vst[(size_t)v] = code;
        if (code != MIC_OK) continue;
        V.push_back(SessVol{ v, m.w, m.h, m.n, m.temporal, un.size() });
        M.push_back(m);
        for (int f = 0; f < m.n; f++) { un.push_back(Unit{ (uint32_t)V.size() - 1, (uint32_t)f }); px.push_back(npx); }
    }
    report();
    if (un.empty()) return MIC_OK;
    int rc = s->activate();
    if (rc) return rc;
    if ((rc = s->ensure(1, 1))) return rc;                                                  // (the session's stream)
    const std::vector<size_t> cuts = mic2_batch_cuts(px, kWorkspaceBudget);
    auto blob = [&](size_t g) { const Mic2Head &m = M[un[g].vol]; return d_files[V[un[g].vol].job] + 20 + 8 * (size_t)m.n + get_u32(m.table + 8 * (size_t)un[g].frame); };
    auto blob_len = [&](size_t g) { return (uint64_t)get_u32(M[un[g].vol].table + 8 * (size_t)un[g].frame + 4); };
    std::vector<uint64_t> begins, ends; std::vector<Mic2DecUnit> du; std::vector<int32_t> ust; std::vector<Mic2DecSpan> spans;
    for (size_t b = 0; b + 1 < cuts.size(); b++) {
        const size_t u0 = cuts[b];
        const int nb = (int)(cuts[b + 1] - u0);
        // the streams go device to device into the session's buffer, which has the slack the decode kernels may read behind a stream
        if ((rc = pack_streams(s, nb, [&](int i) { return blob_len(u0 + (size_t)i); }, [&](int i) { return blob(u0 + (size_t)i); }, true, begins, ends))) return rc;
        du.assign((size_t)nb, Mic2DecUnit{});
        for (int i = 0; i < nb; i++) {
            const size_t g = u0 + (size_t)i;
            const SessVol &sv = V[un[g].vol];
            du[(size_t)i] = Mic2DecUnit{ (const uint8_t *)s->io_comp.p + begins[(size_t)i], (uint32_t)blob_len(g), sv.w, sv.h,
                                         d_frames_out + px_off[sv.job] + (size_t)un[g].frame * px[g], (uint32_t)(sv.temporal && un[g].frame > 0) };
        }
        ust.assign((size_t)nb, MIC_OK);
        if ((rc = mic2_batch_decode_units(s, du.data(), nb, ust.data()))) return rc;
        spans.clear();
        for (int i = 0; i < nb;) {                                                          // runs of units of one volume
            const size_t g = u0 + (size_t)i;
            SessVol &sv = V[un[g].vol];
            int j = i + 1;
            while (j < nb && un[u0 + (size_t)j].vol == un[g].vol) j++;
            for (int k = i; k < j && sv.status == MIC_OK; k++)
                if (ust[(size_t)k] != MIC_OK) { sv.status = ust[(size_t)k]; sv.failed = (int32_t)un[u0 + (size_t)k].frame; }
            if (sv.temporal) {
                uint16_t *dst = d_frames_out + px_off[sv.job] + (size_t)un[g].frame * px[g];
                spans.push_back(Mic2DecSpan{ dst - px[g], dst, (uint32_t)px[g], i, j - i, (int32_t)un[g].frame, sv.status == MIC_OK ? INT_MAX : sv.failed, 0 });
            }
            i = j;
        }
        if ((rc = mic2_batch_accumulate(s, spans.data(), (int)spans.size()))) return rc;
    }
    uint64_t done = 0;
    for (const SessVol &sv : V) { vst[(size_t)sv.job] = sv.status; vff[(size_t)sv.job] = sv.failed; done += sv.status == MIC_OK; }
    report();
    if (stats) *stats = mic_hip_mic2_batch_stats{ un.size(), cuts.size() - 1, done };
    return MIC_OK;
} MIC_ABI_CATCH

}  // extern "C"
