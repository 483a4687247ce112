// mic_mic2_crops.hip -- MIC2: many 3-D crops per call into a device tensor, of one volume (mic_hip_mic2_read_crops,
// mic_hip_mic2_reader_*, mic_hip_session_mic2_read_crops) or of many (mic_hip_mic2_multi_crop_plan, mic_hip_mic2_multi_read_crops,
// mic_hip_mic2_readers_read_crops, mic_hip_session_mic2_multi_read_crops); no reference counterpart.
//
// One core (mic2_multi_read_crops) behind the six doors; a door brings the parsed headers, the frame tables and a source that says
// where a frame's stream lies (the caller's file, the blobs a reader pulled, a file in device memory); a one-volume door makes a
// one-volume plan of its own.  The host plans every named volume (mic2_plan_crops): which frames' streams must be entropy-decoded, and
// the (crop, frame) overlaps -- pieces.  The units of all volumes, ascending by volume, then frame, go through the MIC2 decode chain
// (mic2_batch_decode_units, mic_mic2_batch.hip) in sub-batches that are cut by the units' sizes alone (next_strip_cut), so a
// sub-batch holds frames of independent volumes, frame 0 of temporal ones -- both decoded into one pixel slab -- and residual symbol
// units side by side: a batch of crops from sixteen volumes is one decode chain.  Behind each sub-batch a kernel writes into the
// crop tensor:
//   independent volumes: the shared gather (launch_gather, mic_gather.hip) copies the sub-batch's pieces out of the decoded frames;
//   temporal volumes:    frame_i = frame_0 + sum_{j<=i} UnZigZag(res_j) (mod 2^16) is a running sum per pixel (mic_mic2_batch.hip), and
//                        a crop needs it under its own footprint only: k_mic2_accumulate_crops walks the sub-batch's residual
//                        symbols with one lane per footprint pixel and stores the sums that fall into the crop's z range.  Frame 0,
//                        the spatial unit, is the only full image of the volume on the device; the carry from one sub-batch to the
//                        next lives in the tensor itself.
// A reader call in which some reader has a frame cache (mic_hip_mic2_reader_set_cache, mic_tile_cache.h) takes another core,
// mic2_cached_read_crops: it keeps reconstructed frames in the cache's slots, decodes only what is not resident -- a temporal file
// from the nearest resident frame below -- and builds whole frames (k_mic2_accumulate_frames).  No cache in the call: the core above.
// Shared with the MIC3 patch and strip-file crop readers (mic_rects.h): the piece record, the sub-batch layout, the gather list and
// its launch, the independent volumes' status fold, the tensor check.  Here: the plans, the decode chain, everything temporal.
#include <climits>
#include <memory>
#include "mic_rects.h"
#include "mic_tile_cache.h"

namespace {

// What a sub-batch holds of one temporal volume: its units u0 .. u0 + nb - 1 are the volume's frames f0 .. f0 + nb - 1 (unit u0 of the
// volume's first sub-batch, f0 = 0, is the spatial frame, at frame0 of the pixel slab; every other unit a residual whose symbols lie
// in its sym slab), fbad the volume's first failed frame so far (INT_MAX: none), fw its width.  A footprint names its volume by its
// slot among the call's temporal volumes (the list is sorted by it) and finds the span at spans[slot - slot0]; the launch covers the
// footprints of the volumes present, and everything a block loops over is uniform in it.
// fp = a crop's footprint: w x h pixels at (sx, sy) of every frame, the crop's frames inside the volume zf = fp.frame .. fp.k, slice
// dz the one of zf.  One lane per footprint pixel:
//   acc = frame f0 - 1 of that pixel -- frame 0's sample, or the carry the sub-batch before left in the tensor: in slice(zf) while the
//         sum has not reached zf, in slice(f0 - 1) from then on;
//   acc = (acc + UnZigZag(res_f)) & 0xFFFF for f = f0 .. min(f0 + nb - 1, fp.k), stored into slice(f) when f >= zf     (k_mic2_accumulate);
//   a sum that has not reached zf at the sub-batch's end goes into slice(zf), the next sub-batch's carry.
// A crop that is complete (fp.k < f0) or depends on a failed unit (fp.k >= fbad) is left alone.
struct VolPrint { CropPiece fp; int32_t slot, pad; };
struct VolSpan { uint64_t frame0; int32_t u0, nb, f0, fbad, fw, pad; };
__global__ void __launch_bounds__(256) k_mic2_accumulate_crops(const MicUnit *__restrict__ units, const VolSpan *__restrict__ spans, int slot0,
                                                             const uint16_t *__restrict__ slab, const VolPrint *__restrict__ prints,
                                                             uint16_t *out, int cw, int ch, int cd) {
    const VolPrint vp = prints[blockIdx.x];
    const CropPiece &fp = vp.fp;
    const VolSpan v = spans[vp.slot - slot0];
    const int f0 = v.f0, fw = v.fw;
    if (fp.k < f0 || fp.k >= v.fbad) return;
    const MicUnit *vu = units + v.u0;
    const PieceLanes ln = piece_lanes(fp.w);
    const int zf = fp.frame, iend = min(v.nb, fp.k - f0 + 1), r0 = f0 ? 0 : 1;
    const size_t slice = (size_t)ch * cw;
    uint16_t *dst = out + (((size_t)fp.crop * cd + fp.dz) * ch + fp.dy) * cw + fp.dx;
    for (int y = ln.row; y < fp.h; y += ln.rstep) {
        const size_t srow = (size_t)(fp.sy + y) * fw + fp.sx;
        const mic_gp<uint16_t> d = mic_g(dst + (size_t)y * cw);
        for (int x = ln.col; x < fp.w; x += ln.lw) {
            uint32_t acc;
            if (f0 == 0) {
                acc = mic_g(slab)[v.frame0 + srow + x];
                if (zf == 0) d[x] = (uint16_t)acc;
            } else acc = d[(size_t)max(f0 - 1 - zf, 0) * slice + x];
            for (int i = r0; i < iend; i++) {
                acc = (acc + unzigzag16(mic_g(vu[i].sym)[srow + x])) & 0xFFFFu;             // temporaldelta.go:27-37
                if (f0 + i >= zf) d[(size_t)(f0 + i - zf) * slice + x] = (uint16_t)acc;
            }
            if (f0 + iend - 1 < zf) d[x] = (uint16_t)acc;
        }
    }
}

// ---- whole frames, for the calls that keep them (the frame cache) ---------------------------------------------------------------
// The running sum over WHOLE frames, which the footprint kernel above avoids: a call with a frame cache keeps reconstructed frames,
// so it needs every pixel of the frames it names.  A span is a run of residual units of one temporal volume inside a sub-batch:
// units u0 .. u0 + nb - 1 of the sub-batch, in frame order.  acc starts as the frame at `anchor` -- a slot of a cache's arena, frame 0
// in the sub-batch's pixel slab, or the carry frame the sub-batch before left in the session's workspace --; anchor_dst (0: none) is
// where the anchor itself is kept (frame 0 that missed); for each unit acc = (acc + UnZigZag(sym)) & 0xFFFF, stored to dsts[unit]
// when that is not 0 (a named frame: its slot, or its place in the slab when it is bypassed; frames nobody names are summed through);
// carry_out (0: the run ends here) takes the sum behind the last unit.
// It streams: a lane owns a fixed group of eight pixels, reads 16 bytes of symbols per unit and stores 16 bytes per named frame;
// every address it is given is 16-byte aligned (slots and carries 256, the slab's places 256, symbol slabs 256) and a group starts at a
// multiple of eight pixels.  The last lane's group of fewer than eight is peeled into a loop over pixels.  Symbols, anchor and carry
// are read once.  grid = (spans, chunks of 2048 pixels of the largest frame); everything a block loops over is uniform in it.
// Traffic: 2 bytes x pixels x (residuals + stores + 1).
struct FrameSpan { uint64_t anchor, anchor_dst, carry_out; uint32_t npx; int32_t u0, nb, pad; };
typedef uint32_t fr_u32x4 __attribute__((ext_vector_type(4)));
// two samples in a dword: each half (acc + UnZigZag(sym)) mod 2^16 (temporaldelta.go:27-37)
__device__ __forceinline__ uint32_t add_unzigzag_pair(uint32_t acc, uint32_t sym) {
    const uint32_t d = ((sym >> 1) & 0x7FFF7FFFu) ^ ((sym & 0x00010001u) * 0xFFFFu);
    return ((acc + d) & 0xFFFFu) | ((acc & 0xFFFF0000u) + (d & 0xFFFF0000u));
}
__global__ void __launch_bounds__(256) k_mic2_accumulate_frames(const MicUnit *__restrict__ units, const FrameSpan *__restrict__ spans,
                                                              const uint64_t *__restrict__ dsts) {
    const FrameSpan v = spans[blockIdx.x];
    if (blockIdx.y * 2048u >= v.npx) return;                                                // (a smaller frame than the launch's largest)
    const uint32_t k = (blockIdx.y * 256u + threadIdx.x) * 8u;
    if (k >= v.npx) return;
    const MicUnit *vu = units + v.u0;
    const uint64_t *vd = dsts + v.u0;
    const mic_gp<const uint16_t> anchor = mic_g((const uint16_t *)(uintptr_t)v.anchor);
    if (k + 8 <= v.npx) {
        fr_u32x4 acc = *(mic_gp<const fr_u32x4>)(anchor + k);
        if (v.anchor_dst) *(mic_gp<fr_u32x4>)(mic_g((uint16_t *)(uintptr_t)v.anchor_dst) + k) = acc;
#pragma unroll 4
        for (int i = 0; i < v.nb; i++) {
            const fr_u32x4 sy = *(mic_gp<const fr_u32x4>)(mic_g((const uint16_t *)vu[i].sym) + k);
#pragma unroll
            for (int j = 0; j < 4; j++) acc[j] = add_unzigzag_pair(acc[j], sy[j]);
            const uint64_t d = vd[i];
            if (d) *(mic_gp<fr_u32x4>)(mic_g((uint16_t *)(uintptr_t)d) + k) = acc;
        }
        if (v.carry_out) *(mic_gp<fr_u32x4>)(mic_g((uint16_t *)(uintptr_t)v.carry_out) + k) = acc;
    } else {
        for (uint32_t q = k; q < v.npx; q++) {                                              // the frame's tail of fewer than eight pixels
            uint32_t acc = anchor[q];
            if (v.anchor_dst) mic_g((uint16_t *)(uintptr_t)v.anchor_dst)[q] = (uint16_t)acc;
            for (int i = 0; i < v.nb; i++) {
                acc = (acc + unzigzag16(mic_g((const uint16_t *)vu[i].sym)[q])) & 0xFFFFu;
                const uint64_t d = vd[i];
                if (d) mic_g((uint16_t *)(uintptr_t)d)[q] = (uint16_t)acc;
            }
            if (v.carry_out) mic_g((uint16_t *)(uintptr_t)v.carry_out)[q] = (uint16_t)acc;
        }
    }
}

}  // namespace

namespace micapi {

// The plan of n crops of cw x ch x cd in a volume of width x height x nframes: the clipped box of each crop, one piece per frame of
// it (sorted by frame, so a sub-batch of frames owns a contiguous range), one footprint per crop, and the frames to entropy-decode --
// independent: the frames some crop overlaps; temporal: 0 .. the last of them, whatever lies in between being part of the sum.
int mic2_plan_crops(int width, int height, int nframes, int temporal, const int32_t *xyz, int n, int cw, int ch, int cd, CropPlan &plan) {
    plan.frames.clear(); plan.pieces.clear(); plan.prints.clear();
    std::vector<uint32_t> per_frame((size_t)std::max(nframes, 0) + 1, 0);       // pieces of each frame, then their first index
    for (int i = 0; i < n; i++) {
        const int64_t x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        const int64_t x0 = std::max<int64_t>(x, 0), x1 = std::min<int64_t>(x + cw, width), y0 = std::max<int64_t>(y, 0), y1 = std::min<int64_t>(y + ch, height);
        const int64_t z0 = std::max<int64_t>(z, 0), z1 = std::min<int64_t>(z + cd, nframes);
        if (x1 <= x0 || y1 <= y0 || z1 <= z0) continue;
        plan.prints.push_back(CropPiece{ i, (int32_t)z0, (int32_t)x0, (int32_t)y0, (int32_t)(x0 - x), (int32_t)(y0 - y), (int32_t)(z0 - z),
                                         (int32_t)(x1 - x0), (int32_t)(y1 - y0), (int32_t)(z1 - 1) });
        for (int64_t f = z0; f < z1; f++) per_frame[(size_t)f]++;
    }
    size_t total = 0;
    int last = -1;
    for (int f = 0; f < nframes; f++) {
        const uint32_t c = per_frame[(size_t)f];
        per_frame[(size_t)f] = (uint32_t)total;
        total += c;
        if (c) last = f;
        if (c && !temporal) plan.frames.push_back((uint32_t)f);
    }
    if (total > 0xFFFFFFFFull) return MIC_ERR_UNSUPPORTED;
    if (temporal) for (int f = 0; f <= last; f++) plan.frames.push_back((uint32_t)f);
    std::vector<int32_t> place((size_t)std::max(nframes, 0), 0);                // frame -> its index in plan.frames
    for (size_t k = 0; k < plan.frames.size(); k++) place[plan.frames[k]] = (int32_t)k;
    plan.pieces.resize(total);
    for (const CropPiece &fp : plan.prints)
        for (int f = fp.frame; f <= fp.k; f++) {
            CropPiece pc = fp;
            pc.frame = f; pc.dz = fp.dz + (f - fp.frame); pc.k = place[(size_t)f];
            plan.pieces[per_frame[(size_t)f]++] = pc;
        }
    return MIC_OK;
}

// What the three crop entry points check of their arguments before a device is touched; *need = bytes of the crop tensor.
int mic2_crop_args(const Mic2Head &m, const int32_t *xyz, int n, int cw, int ch, int cd, size_t sample_bytes, size_t out_cap, size_t *need) {
    if (cw <= 0 || ch <= 0 || cd <= 0 || n < 0 || (n > 0 && !xyz)) return MIC_ERR_ARGS;
    if (m.w <= 0 || m.h <= 0) return MIC_ERR_CORRUPT;                                       // (as mic_hip_mic2_decompress)
    if ((size_t)m.w * (size_t)m.h > ((size_t)1 << 28) || m.file_len > 0xFFFFFFF0ull) return MIC_ERR_UNSUPPORTED;
    return tensor_bytes(n, cd, ch, cw, sample_bytes, out_cap, need);
}

}  // namespace micapi

struct mic_hip_mic2_reader {
    std::mutex mu;                          // one call at a time (and with it one callback at a time)
    mic_hip_read_fn read = nullptr; void *user = nullptr;
    Mic2Head m;
    std::vector<uint8_t> head;              // the fixed header and the frame table
    std::vector<uint8_t> keep;              // the blobs of the last call's plan, in plan order
    std::vector<size_t> pos;                // frame -> its blob's place in keep
    mic_hip_tile_cache *cache = nullptr; uint64_t owner = 0;   // mic_hip_mic2_reader_set_cache (guarded by mu): the crop calls' frame cache and this reader's owner number in it
    bool timing = false;                    // mic_hip_mic2_reader_set_timing: read_crops times its kernels on the session it leases ...
    std::vector<std::string> t_names; std::vector<float> t_ms;   // ... and keeps what mic_hip_session_last_timings said of the last call
    // the blobs of the plan's frames (their table entries checked by crops_call) through the callback, one read per run of neighbours
    int fetch(const CropPlan &plan, Mic2Source &src) {
        const size_t nfr = plan.frames.size(), data_off = 20 + 8 * (size_t)m.n;
        std::vector<uint64_t> off(nfr), len(nfr);
        size_t total = 0;
        for (size_t k = 0; k < nfr; k++) {
            const uint8_t *e = m.table + 8 * (size_t)plan.frames[k];
            off[k] = data_off + get_u32(e); len[k] = get_u32(e + 4);
            total += (size_t)len[k];
        }
        keep.resize(total + 1);
        pos.assign((size_t)m.n, 0);
        size_t at = 0;
        for (size_t i = 0; i < nfr;) {
            size_t j = i + 1, bytes = (size_t)len[i];
            while (j < nfr && off[j] == off[j - 1] + len[j - 1]) bytes += (size_t)len[j++];
            if (read(user, off[i], keep.data() + at, bytes) != 0) return MIC_ERR_IO;
            for (; i < j; i++) { pos[plan.frames[i]] = at; at += (size_t)len[i]; }
        }
        src.device = false;
        src.blob = [this](uint32_t f) { return (const uint8_t *)keep.data() + pos[f]; };
        return MIC_OK;
    }
};

namespace {

// the fixed 20 bytes (mic_hip_mic2_info's checks, against the whole file's length) into m; the table is the caller's to attach
int parse_mic2(const uint8_t *head, uint64_t file_len, Mic2Head &m) {
    const int rc = mic_hip_mic2_info(head, (size_t)file_len, &m.w, &m.h, &m.n, &m.temporal);
    m.file_len = file_len;
    return rc;
}

// ---- crops of many volumes per call ------------------------------------------------------------------------------------------

// a volume of the call: where its header and table are read (host), what they said, and the plan of the crops that name it
struct Mic2Vol {
    const uint8_t *head = nullptr; size_t head_len = 0; uint64_t file_len = 0;      // (the door's)
    bool named = false;                     // some crop names it: only then is it looked at
    int32_t status = MIC_OK;
    Mic2Head m;
    CropPlan plan;                          // crop = the call's index; empty for a refused volume
};
struct Mic2MultiPlan {
    std::vector<Mic2Vol> vols;
    uint64_t units = 0, pieces = 0, read = 0;   // frames to entropy-decode, (crop, frame) overlaps, named volumes that were accepted
};

// header and table of a named volume: mic_hip_mic2_info's checks against the whole file's length, and mic2_crop_args' of the volume
int parse_vol(Mic2Vol &f) {
    if (!f.head) return MIC_ERR_ARGS;
    if (f.head_len < 20) return MIC_ERR_CORRUPT;
    const int rc = parse_mic2(f.head, f.file_len, f.m);
    if (rc) return rc;
    if (f.m.w <= 0 || f.m.h <= 0) return MIC_ERR_CORRUPT;
    if ((size_t)f.m.w * (size_t)f.m.h > ((size_t)1 << 28) || f.file_len > 0xFFFFFFF0ull) return MIC_ERR_UNSUPPORTED;
    if (f.head_len < 20 + 8 * (size_t)f.m.n) return MIC_ERR_ARGS;                           // (the table is not all there)
    f.m.table = f.head + 20;
    return MIC_OK;
}

// a volume fails alone: its crops keep no pieces (their samples stay 0) and carry `code`
void refuse_vol(Mic2MultiPlan &mp, Mic2Vol &f, int code) {
    mp.units -= f.plan.frames.size(); mp.pieces -= f.plan.pieces.size(); mp.read--;
    f.status = code; f.plan = CropPlan();
}

// The plan of n crops (x, y, z, volume) of cw x ch x cd over the volumes (head, head_len, file_len set by the door): each named
// volume's own mic2_plan_crops.  MIC_ERR_ARGS for a volume index outside the list; a volume that is refused keeps its code in
// vols[v].status and no plan.
int mic2_multi_plan(Mic2MultiPlan &mp, const int32_t *xyzv, int n, int cw, int ch, int cd) {
    const int nv = (int)mp.vols.size();
    std::vector<std::vector<int32_t>> mine((size_t)nv);                                     // the crops that name volume v
    for (int i = 0; i < n; i++) {
        const int32_t v = xyzv[4 * (size_t)i + 3];
        if (v < 0 || v >= nv) return MIC_ERR_ARGS;
        mine[(size_t)v].push_back(i);
    }
    mp.units = mp.pieces = mp.read = 0;
    std::vector<int32_t> xyz;
    for (int v = 0; v < nv; v++) {
        Mic2Vol &f = mp.vols[(size_t)v];
        const std::vector<int32_t> &cr = mine[(size_t)v];
        f.named = !cr.empty(); f.status = MIC_OK; f.plan = CropPlan();
        if (!f.named || (f.status = parse_vol(f)) != MIC_OK) continue;
        xyz.resize(3 * cr.size());
        for (size_t j = 0; j < cr.size(); j++) std::copy(xyzv + 4 * (size_t)cr[j], xyzv + 4 * (size_t)cr[j] + 3, xyz.begin() + 3 * j);
        const int rc = mic2_plan_crops(f.m.w, f.m.h, f.m.n, f.m.temporal, xyz.data(), (int)cr.size(), cw, ch, cd, f.plan);
        if (rc) return rc;
        for (CropPiece &pc : f.plan.pieces) pc.crop = cr[(size_t)pc.crop];
        for (CropPiece &fp : f.plan.prints) fp.crop = cr[(size_t)fp.crop];
        mp.units += f.plan.frames.size(); mp.pieces += f.plan.pieces.size(); mp.read++;
        for (uint32_t fr : f.plan.frames) {                                                 // as mic_hip_mic2_decompress, multiframe.go:137-139
            const uint64_t off = 20 + 8 * (uint64_t)f.m.n + get_u32(f.m.table + 8 * (size_t)fr), bl = get_u32(f.m.table + 8 * (size_t)fr + 4);
            if (bl == 0 || off + bl > f.file_len) { refuse_vol(mp, f, MIC_ERR_CORRUPT); break; }
        }
    }
    return mp.pieces > 0xFFFFFFFFull ? MIC_ERR_UNSUPPORTED : MIC_OK;
}

// where the core finds the stream of a volume's frame, on the host or (device) on the session's device
struct Mic2MultiSource { bool device = false; std::function<const uint8_t *(uint32_t vol, uint32_t frame)> blob; };

// n crops into d_out ([n][cd][ch][cw] samples of o's type, an address s's device can write: patch_pointer) on a session the caller
// holds and has made current.  A typed tensor cannot carry the temporal volumes' running sums (u16, mod 2^16): they then live in a u16
// tensor of the same shape in the session's workspace (s->crop_stage, reserved before the first launch), and behind the last
// sub-batch one kernel converts the footprint of every temporal crop that is complete into d_out (launch_convert).  The units of every planned volume go through the MIC2 decode chain in plan order, in sub-batches cut by their sizes alone;
// the call stops in front of a sub-batch when every unit left belongs to a temporal volume that has already failed (a one-volume call
// whose frame failed).  status[i] / failed_frame[i] (each may be NULL): MIC_OK / -1, or the code of the first failing frame crop i
// depends on and that frame.
int mic2_multi_read_crops(mic_hip_session *s, const Mic2MultiPlan &mp, const Mic2MultiSource &src, int n, int cw, int ch, int cd, const OutFormat &o,
                          void *d_out, size_t need, int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats) {
    struct Unit { uint32_t vol, frame; };
    const size_t nv = mp.vols.size();
    std::vector<Unit> un; std::vector<size_t> px, unit0(nv, 0);
    for (size_t v = 0; v < nv; v++) {
        const Mic2Vol &f = mp.vols[v];
        unit0[v] = un.size();
        for (uint32_t fr : f.plan.frames) { un.push_back(Unit{ (uint32_t)v, fr }); px.push_back((size_t)f.m.w * (size_t)f.m.h); }
    }
    const size_t nu = un.size();
    int rc;
    if ((rc = s->ensure(1, 1))) return rc;                                                  // (the session's stream)
    if ((rc = fill_pad(s->stream, o, d_out, need))) return rc;                              // outside the volumes, refused volumes; every byte is written
    auto vol = [&](size_t u) -> const Mic2Vol & { return mp.vols[un[u].vol]; };
    auto is_frame = [&](size_t u) { return !vol(u).m.temporal || un[u].frame == 0; };       // a frame unit (mode 0), else a residual's symbols (mode 3)
    auto blob_len = [&](size_t u) { return (uint64_t)get_u32(vol(u).m.table + 8 * (size_t)un[u].frame + 4); };
    // the call's lists: independent volumes their pieces, in unit order -- the tensor as n * cd slices of ch x cw --; temporal volumes
    // their footprints, in volume order, each volume that has units a slot.  Only a frame unit has a place in its sub-batch's slab.
    std::vector<RectPiece> pieces;
    std::vector<VolPrint> prints; std::vector<size_t> pfirst;                               // the footprints of slot t
    std::vector<int32_t> slot_of(nv, -1), slot_vol;
    int tw = 1, th = 1;
    for (size_t v = 0; v < nv; v++) {
        const Mic2Vol &f = mp.vols[v];
        if (f.plan.frames.empty()) continue;
        if (!f.m.temporal) {
            if ((uint64_t)n * (uint64_t)cd > (uint64_t)INT_MAX) return MIC_ERR_UNSUPPORTED;      // (a slice's index is an int32)
            for (const CropPiece &pc : f.plan.pieces)
                pieces.push_back(RectPiece{ pc.crop * cd + pc.dz, (uint32_t)(unit0[v] + (size_t)pc.k), pc.sx, pc.sy, pc.dx, pc.dy, pc.w, pc.h });
        } else {
            slot_of[v] = (int32_t)slot_vol.size(); slot_vol.push_back((int32_t)v);
            pfirst.push_back(prints.size());
            for (const CropPiece &fp : f.plan.prints) { prints.push_back(VolPrint{ fp, slot_of[v], 0 }); tw = std::max(tw, fp.w); th = std::max(th, fp.h); }
        }
    }
    pfirst.push_back(prints.size());
    const RectBatches L = rect_batches(nu, [&](size_t i0) { return next_strip_cut(px, i0); }, [&](size_t u) { return is_frame(u) ? px[u] : (size_t)0; },
                                       pieces, cw, ch, [&](size_t u) { return UnitStride{ vol(u).m.w, 0 }; },
                                       [&](size_t u) { return un[u].vol; }, o);
    size_t comp_max = 0;                                                                    // the most stream bytes of a sub-batch
    for (size_t b = 0, comp = 0; b < L.subs(); b++, comp = 0)
        for (size_t u = L.cuts[b]; u < L.cuts[b + 1]; u++) comp_max = std::max(comp_max, comp += (size_t)blob_len(u));
    // ... and, per sub-batch, a span per temporal volume it holds a part of: written when the sub-batch's statuses are known, each
    // into a place of its own on the host and on the device
    size_t nspan = 0;
    for (size_t b = 0; b + 1 < L.cuts.size(); b++)
        for (size_t u = L.cuts[b]; u < L.cuts[b + 1]; u++) nspan += vol(u).m.temporal && (u == L.cuts[b] || un[u].vol != un[u - 1].vol);
    std::vector<VolSpan> spans; spans.reserve(nspan);
    const size_t list_bytes = gather_bytes(L), print_bytes = align_up(prints.size() * sizeof(VolPrint), 16);
    const bool staged = o.typed() && !prints.empty();                                       // temporal sums go through the u16 staging tensor
    const size_t span_bytes = align_up(nspan * sizeof(VolSpan), 16), behind = print_bytes + span_bytes + (staged ? prints.size() * sizeof(ConvertRun) : 0);
    if (staged && (rc = s->crop_stage.reserve(need / o.sample * 2 + 64))) return rc;
    uint16_t *d_sums = staged ? (uint16_t *)s->crop_stage.p : (uint16_t *)d_out;
    if (nu) {
        if ((rc = s->io_comp.reserve(comp_max + 64))) return rc;                            // (once: pack_streams then finds room for every sub-batch)
        if ((rc = s->io_px.reserve(L.slab_max * 2 + 64))) return rc;
        if ((rc = upload_gather(s, L, o, behind))) return rc;                               // (the footprints, the spans and a typed call's runs behind the list)
        if (!prints.empty()) HIP_TRY(hipMemcpyAsync((char *)s->pieces.p + list_bytes, prints.data(), prints.size() * sizeof(VolPrint), hipMemcpyHostToDevice, s->stream));
    }
    const VolPrint *d_prints = (const VolPrint *)((char *)s->pieces.p + list_bytes);
    VolSpan *d_spans = (VolSpan *)((char *)s->pieces.p + list_bytes + print_bytes);
    std::vector<int32_t> ust(nu, MIC_OK);                                                   // status of unit u
    std::vector<int32_t> fbad(slot_vol.size(), INT_MAX), bad_code(slot_vol.size(), MIC_OK); // a temporal volume's first failed frame
    std::vector<uint64_t> begins, ends; std::vector<Mic2DecUnit> du;
    uint64_t nslab = 0;                                                                     // decode chains run
    for (size_t b = 0; b + 1 < L.cuts.size(); b++) {
        const size_t u0 = L.cuts[b];
        const int nb = (int)(L.cuts[b + 1] - u0);
        // units lie in volume order: when the first and the last one left are of one volume, nothing but that volume is left, and when
        // it is a temporal one that has failed, no crop is waiting for any of them
        if (un[u0].vol == un[nu - 1].vol && slot_of[un[u0].vol] >= 0 && fbad[(size_t)slot_of[un[u0].vol]] != INT_MAX) break;
        if ((rc = pack_streams(s, nb, [&](int i) { return blob_len(u0 + (size_t)i); },
                               [&](int i) { return src.blob(un[u0 + (size_t)i].vol, un[u0 + (size_t)i].frame); }, src.device, begins, ends))) return rc;
        du.resize((size_t)nb);
        for (int i = 0; i < nb; i++) {
            const size_t g = u0 + (size_t)i;
            du[(size_t)i] = Mic2DecUnit{ (const uint8_t *)s->io_comp.p + begins[(size_t)i], (uint32_t)blob_len(g), vol(g).m.w, vol(g).m.h,
                                         is_frame(g) ? (uint16_t *)s->io_px.p + L.slab_off[g] : nullptr, (uint32_t)!is_frame(g) };
        }
        if ((rc = mic2_batch_decode_units(s, du.data(), nb, ust.data() + u0))) return rc;
        nslab++;
        // the temporal volumes of this sub-batch: runs of units of one volume
        const size_t sp0 = spans.size();
        int slot0 = 0;
        for (int i = 0; i < nb;) {
            const size_t g = u0 + (size_t)i;
            int j = i + 1;
            while (j < nb && un[u0 + (size_t)j].vol == un[g].vol) j++;
            if (vol(g).m.temporal) {
                const int t = slot_of[un[g].vol];
                if (spans.size() == sp0) slot0 = t;
                for (int k = i; k < j && fbad[(size_t)t] == INT_MAX; k++)
                    if (ust[u0 + (size_t)k] != MIC_OK) { fbad[(size_t)t] = (int32_t)un[u0 + (size_t)k].frame; bad_code[(size_t)t] = ust[u0 + (size_t)k]; }
                spans.push_back(VolSpan{ un[g].frame == 0 ? L.slab_off[g] : 0, i, j - i, (int32_t)un[g].frame, fbad[(size_t)t], vol(g).m.w, 0 });
            }
            i = j;
        }
        const size_t nsp = spans.size() - sp0;
        s->timer.reset(s->stream);
        gather_units(s, "k_mic2_gather_crops", kGatherU16, s->io_px.p, L, b, d_out, o, (size_t)ch * (size_t)cw, behind);
        if (nsp) {
            const size_t q0 = pfirst[(size_t)slot0], nq = pfirst[(size_t)slot0 + nsp] - q0;
            HIP_TRY(hipMemcpyAsync(d_spans + sp0, spans.data() + sp0, nsp * sizeof(VolSpan), hipMemcpyHostToDevice, s->stream));
            s->timer.mark("k_mic2_accumulate_crops");
            hipLaunchKernelGGL(k_mic2_accumulate_crops, dim3((unsigned)nq, row_chunks(tw, th)), dim3(256), 0, s->stream,
                               (const MicUnit *)s->units.p, (const VolSpan *)d_spans + sp0, slot0, (const uint16_t *)s->io_px.p, d_prints + q0,
                               d_sums, cw, ch, cd);
        }
        s->timer.mark("end");
        HIP_TRY(hipGetLastError());
    }
    std::vector<ConvertRun> runs;                                                           // (lives until the synchronise below)
    if (staged) {
        for (const VolPrint &vp : prints) {
            const CropPiece &fp = vp.fp;
            if (fp.k >= fbad[(size_t)vp.slot]) continue;                                    // (depends on a failed frame: unspecified, left as it is)
            runs.push_back(ConvertRun{ (((uint64_t)fp.crop * (uint64_t)cd + (uint64_t)fp.dz) * (uint64_t)ch + (uint64_t)fp.dy) * (uint64_t)cw + (uint64_t)fp.dx,
                                       fp.w, fp.h, fp.k - fp.frame + 1, slot_vol[(size_t)vp.slot] });
        }
        if (!runs.empty()) {
            ConvertRun *d_runs = (ConvertRun *)((char *)s->pieces.p + list_bytes + print_bytes + span_bytes);
            HIP_TRY(hipMemcpyAsync(d_runs, runs.data(), runs.size() * sizeof(ConvertRun), hipMemcpyHostToDevice, s->stream));
            launch_convert(s->stream, o, out_table(s, L, behind), d_sums, d_runs, runs.size(), tw, th, cd, cw, ch, d_out);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    fold_unit_status(pieces, ust, n, cd, status, failed_frame, [&](uint32_t u) { return (int32_t)un[u].frame; });   // independent volumes: pieces are in frame order
    for (size_t v = 0; v < nv; v++) {                                                       // temporal volumes: every crop that reaches the failed frame
        if (slot_of[v] < 0) continue;
        const int32_t fb = fbad[(size_t)slot_of[v]];
        for (const CropPiece &fp : mp.vols[v].plan.prints) {
            if (fp.k < fb) continue;
            if (status) status[fp.crop] = bad_code[(size_t)slot_of[v]];
            if (failed_frame) failed_frame[fp.crop] = fb;
        }
    }
    if (stats) *stats = mic_hip_multi_crop_stats{ mp.units, mp.pieces, nslab, mp.read };
    return MIC_OK;
}

// ---- the frame cache in a crop call (mic_tile_cache.h) -----------------------------------------------------------------------------
// The caches of a call: locked in address order (behind the readers' locks) until the object dies, which is behind the call's final
// synchronise; a call that fails before finish() is undone there (rollback, and what a launch of the call may have written is spoiled).
struct FrameCaches {
    struct Use {
        mic_hip_tile_cache *c; bool usable = false, planned = false;
        std::vector<SlotIndex::Key> keys; std::vector<uint8_t> outcome; std::vector<uint32_t> slot;
        std::vector<GatherPiece> pieces; int mw = 1, mh = 1;                                // hits and misses: gathered out of the arena
        std::vector<uint32_t> written;                                                      // slots a launch of this call has been queued for
    };
    std::vector<Use> uses;
    std::vector<std::unique_lock<std::mutex>> locks;
    mic_hip_session *s = nullptr; bool launched = false, done = false;
    size_t cached_pieces() const { size_t n = 0; for (const Use &u : uses) n += u.pieces.size(); return n; }
    void finish() { for (Use &us : uses) us.c->index.commit(); done = true; }
    ~FrameCaches() {
        if (done) return;
        if (launched && s && s->stream) (void)hipStreamSynchronize(s->stream);             // (the slots are not let go while something may write them)
        for (Use &us : uses) {
            if (!us.planned) continue;
            us.c->index.rollback();
            for (uint32_t q : us.written) us.c->index.spoil(q);
        }
    }
};

// The core of a reader call in which some reader has a frame cache: vol_reader[v] = the reader behind volume v of the plan.  Readers,
// not volumes, own frames: a reader listed as several volumes is one owner, its named frames the union.  Per owner the named frames
// (those some crop overlaps) are judged by its cache's index -- a reader without a cache: all bypassed --, then the streams to decode
// are chosen: independent files, the misses and the bypassed; temporal files, for each named frame f that is not a hit the residuals
// a + 1 .. f behind its anchor a, the largest frame below f that is resident once the call is planned (none: from frame 0's spatial
// stream on).  The units -- owner order, then frame order -- go through the MIC2 decode chain in sub-batches as in
// mic2_multi_read_crops.  Behind a sub-batch's decode: the independent misses go from the slab into their slots (k_cache_fill); one
// k_mic2_accumulate_frames launch sums the temporal runs into slots (misses) and slab places (bypassed); the shared gather copies the
// bypassed frames' pieces out of the slab.  Behind the last sub-batch the pieces of hits and misses are gathered out of the arenas,
// one launch per cache.  A run that goes on in the next sub-batch leaves its sum in the owner's carry frame (s->crop_stage).
int mic2_cached_read_crops(mic_hip_session *s, const Mic2MultiPlan &mp, const std::vector<mic_hip_mic2_reader *> &vol_reader, int n, int cw, int ch, int cd,
                           const OutFormat &o, void *d_out, size_t need, int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats) {
    constexpr uint8_t kNotNamed = 255;
    struct Owner {
        mic_hip_mic2_reader *r; int use = -1; size_t key0 = 0;
        std::vector<uint32_t> named, decode;                                                // ascending
        std::vector<uint8_t> oc; std::vector<uint32_t> slot; std::vector<int64_t> unit;     // per frame of the file: outcome (kNotNamed), slot, unit of the call (-1)
        std::vector<int32_t> code, failed;                                                  // per frame: what a crop that needs it gets
        size_t carry = 0;                                                                   // its carry frame, bytes into s->crop_stage
        // the walk over its units (temporal): the frame before, whether the run stands, the frame that felled it
        int64_t prev = -2; bool alive = false; int32_t bad_code = MIC_OK, bad_frame = -1;
    };
    const size_t nv = mp.vols.size();
    std::vector<Owner> own; std::vector<int32_t> owner_of(nv, -1);
    for (size_t v = 0; v < nv; v++) {
        const Mic2Vol &f = mp.vols[v];
        if (f.plan.pieces.empty()) continue;
        size_t w = 0;
        while (w < own.size() && own[w].r != vol_reader[v]) w++;
        if (w == own.size()) {
            own.emplace_back();
            Owner &ow = own.back();
            ow.r = vol_reader[v];
            const size_t nf = (size_t)ow.r->m.n;
            ow.oc.assign(nf, kNotNamed); ow.slot.assign(nf, SlotIndex::kNoSlot); ow.unit.assign(nf, -1); ow.code.assign(nf, MIC_OK); ow.failed.assign(nf, -1);
        }
        owner_of[v] = (int32_t)w;
        for (const CropPiece &pc : f.plan.pieces) own[w].oc[(size_t)pc.frame] = (uint8_t)SlotIndex::kBypass;
    }
    if ((uint64_t)n * (uint64_t)cd > (uint64_t)INT_MAX) return MIC_ERR_UNSUPPORTED;         // (a slice's index is an int32)
    int rc;
    if ((rc = s->ensure(1, 1))) return rc;                                                  // (the session's stream)
    // the caches: locked, their arenas, their keys -- owner order, frames ascending --, the policy
    FrameCaches fc;
    fc.s = s;
    {
        std::vector<mic_hip_tile_cache *> cs;
        for (const Owner &ow : own) if (ow.r->cache) cs.push_back(ow.r->cache);
        std::sort(cs.begin(), cs.end(), std::less<mic_hip_tile_cache *>());
        cs.erase(std::unique(cs.begin(), cs.end()), cs.end());
        fc.uses.resize(cs.size());
        fc.locks.reserve(cs.size());
        for (size_t k = 0; k < cs.size(); k++) { fc.uses[k].c = cs[k]; fc.locks.emplace_back(cs[k]->mu); }
        for (FrameCaches::Use &us : fc.uses) if ((rc = us.c->ensure_arena(s->device, &us.usable))) return rc;
        for (Owner &ow : own) {
            for (size_t f = 0; f < ow.oc.size(); f++) if (ow.oc[f] != kNotNamed) ow.named.push_back((uint32_t)f);
            if (!ow.r->cache) continue;
            ow.use = (int)(std::lower_bound(cs.begin(), cs.end(), ow.r->cache, std::less<mic_hip_tile_cache *>()) - cs.begin());
            FrameCaches::Use &us = fc.uses[(size_t)ow.use];
            ow.key0 = us.keys.size();
            for (uint32_t f : ow.named) us.keys.push_back(SlotIndex::Key{ ow.r->owner, f });
        }
        for (FrameCaches::Use &us : fc.uses) {
            us.outcome.assign(us.keys.size(), SlotIndex::kBypass); us.slot.assign(us.keys.size(), SlotIndex::kNoSlot);
            if (us.usable) us.c->index.plan(us.keys.data(), us.keys.size(), us.outcome.data(), us.slot.data());
            else us.c->index.bypass_all(us.keys.size());
            us.planned = true;
        }
    }
    // per owner: the outcomes, the streams to decode
    struct Unit { uint32_t owner, frame; };
    std::vector<Unit> un; std::vector<size_t> px;
    for (size_t w = 0; w < own.size(); w++) {
        Owner &ow = own[w];
        const FrameCaches::Use *us = ow.use >= 0 ? &fc.uses[(size_t)ow.use] : nullptr;
        if (us) for (size_t i = 0; i < ow.named.size(); i++) { ow.oc[ow.named[i]] = us->outcome[ow.key0 + i]; ow.slot[ow.named[i]] = us->slot[ow.key0 + i]; }
        std::vector<char> indec(ow.oc.size(), 0);
        for (uint32_t f : ow.named) {
            if (ow.oc[f] == SlotIndex::kHit) continue;
            if (!ow.r->m.temporal) { indec[f] = 1; continue; }
            for (uint32_t g = f;; g--) {                                                    // down to the anchor, or to what an earlier frame's chain holds
                if (indec[g]) break;
                indec[g] = 1;
                if (g == 0 || (us && us->usable && us->c->index.has(SlotIndex::Key{ ow.r->owner, g - 1 }))) break;
            }
        }
        for (size_t f = 0; f < indec.size(); f++)
            if (indec[f]) { ow.decode.push_back((uint32_t)f); ow.unit[f] = (int64_t)un.size(); un.push_back(Unit{ (uint32_t)w, (uint32_t)f }); px.push_back((size_t)ow.r->m.w * (size_t)ow.r->m.h); }
    }
    const size_t nu = un.size();
    auto head = [&](size_t u) -> const Mic2Head & { return own[un[u].owner].r->m; };
    auto is_frame = [&](size_t u) { return !head(u).temporal || un[u].frame == 0; };        // a frame unit (mode 0), else a residual's symbols (mode 3)
    auto in_slab = [&](size_t u) { return is_frame(u) || own[un[u].owner].oc[un[u].frame] == SlotIndex::kBypass; };   // (a bypassed named frame is summed into the slab)
    auto blob_len = [&](size_t u) { return (uint64_t)get_u32(head(u).table + 8 * (size_t)un[u].frame + 4); };
    // only the streams to decode are pulled
    {
        CropPlan want; Mic2Source one;
        for (Owner &ow : own) {
            if (ow.decode.empty()) continue;
            want.frames = ow.decode;
            if ((rc = ow.r->fetch(want, one))) return rc;
        }
    }
    if ((rc = fill_pad(s->stream, o, d_out, need))) return rc;                              // outside the volumes, refused volumes; every byte is written
    // the pieces: of a bypassed frame out of its sub-batch's slab (by unit), of a hit or a miss out of its cache's arena
    std::vector<RectPiece> pieces; std::vector<int32_t> piece_src;
    {
        std::vector<std::pair<RectPiece, int32_t>> by_unit;
        for (size_t v = 0; v < nv; v++) {
            if (owner_of[v] < 0) continue;
            Owner &ow = own[(size_t)owner_of[v]];
            for (const CropPiece &pc : mp.vols[v].plan.pieces) {
                const RectPiece rp{ pc.crop * cd + pc.dz, (uint32_t)std::max<int64_t>(ow.unit[(size_t)pc.frame], 0), pc.sx, pc.sy, pc.dx, pc.dy, pc.w, pc.h };
                if (ow.oc[(size_t)pc.frame] == SlotIndex::kBypass) { by_unit.emplace_back(rp, (int32_t)v); continue; }
                FrameCaches::Use &us = fc.uses[(size_t)ow.use];
                const PieceDst pd = piece_dst(rp, cw, ch, o);
                us.pieces.push_back(GatherPiece{ (uint64_t)ow.slot[(size_t)pc.frame] * us.c->slot_bytes + ((uint64_t)pc.sy * (uint64_t)ow.r->m.w + (uint64_t)pc.sx) * 2, pd.dst,
                                                 ow.r->m.w, pd.dstride, pc.w, pc.h, 0, (int32_t)v });
                us.mw = std::max(us.mw, pc.w); us.mh = std::max(us.mh, pc.h);
            }
        }
        std::stable_sort(by_unit.begin(), by_unit.end(), [](const std::pair<RectPiece, int32_t> &a, const std::pair<RectPiece, int32_t> &b) { return a.first.unit < b.first.unit; });
        for (const auto &p : by_unit) { pieces.push_back(p.first); piece_src.push_back(p.second); }
    }
    // a unit's place in the slab is a multiple of 128 samples: the frame kernel's 16-byte accesses
    RectBatches L = rect_batches(nu, [&](size_t i0) { return next_strip_cut(px, i0); }, [&](size_t u) { return in_slab(u) ? align_up(px[u], 128) : (size_t)0; },
                                 pieces, cw, ch, [&](size_t u) { return UnitStride{ head(u).w, 0 }; }, [&](size_t) { return 0u; }, o);
    for (size_t q = 0; q < pieces.size(); q++) L.list[q].source = piece_src[q];             // (a reader listed twice: the piece's own volume)
    size_t comp_max = 0;                                                                    // the most stream bytes of a sub-batch
    for (size_t b = 0, comp = 0; b < L.subs(); b++, comp = 0)
        for (size_t u = L.cuts[b]; u < L.cuts[b + 1]; u++) comp_max = std::max(comp_max, comp += (size_t)blob_len(u));
    size_t carry_bytes = 0;
    for (Owner &ow : own) if (ow.r->m.temporal && !ow.decode.empty()) { ow.carry = carry_bytes; carry_bytes += align_up((size_t)ow.r->m.w * (size_t)ow.r->m.h * 2, 256); }
    // behind the gather list: the cached pieces, cache by cache; the fills of the independent misses; a destination per unit; the spans
    std::vector<CacheFill> fills; std::vector<size_t> fill_first{ 0 };                      // fills[fill_first[u] .. fill_first[u + 1]): unit u's (0 or 1)
    std::vector<uint64_t> dsts(nu, 0);
    std::vector<FrameSpan> spans; spans.reserve(nu + 1);
    const size_t cached_bytes = align_up(fc.cached_pieces() * sizeof(GatherPiece), 16);
    size_t nfill = 0;
    for (size_t u = 0; u < nu; u++) nfill += !head(u).temporal && own[un[u].owner].oc[un[u].frame] == SlotIndex::kMiss;
    const size_t fill_bytes = align_up(nfill * sizeof(CacheFill), 16), dst_bytes = align_up(nu * sizeof(uint64_t), 16), span_bytes = align_up((nu + 1) * sizeof(FrameSpan), 16);
    const size_t behind = cached_bytes + fill_bytes + dst_bytes + span_bytes;
    if (nu) {
        if ((rc = s->io_comp.reserve(comp_max + 64))) return rc;                            // (once: pack_streams then finds room for every sub-batch)
        if ((rc = s->io_px.reserve(L.slab_max * 2 + 64))) return rc;
        if (carry_bytes && (rc = s->crop_stage.reserve(carry_bytes + 64))) return rc;
    }
    if ((rc = upload_gather(s, L, o, behind))) return rc;
    char *const d_behind = (char *)s->pieces.p + gather_bytes(L);
    const GatherPiece *d_cached = (const GatherPiece *)d_behind;
    const CacheFill *d_fills = (const CacheFill *)(d_behind + cached_bytes);
    uint64_t *d_dsts = (uint64_t *)(d_behind + cached_bytes + fill_bytes);
    FrameSpan *d_spans = (FrameSpan *)(d_behind + cached_bytes + fill_bytes + dst_bytes);
    auto slot_addr = [&](const Owner &ow, uint32_t q) { const mic_hip_tile_cache *c = fc.uses[(size_t)ow.use].c; return (uint64_t)(uintptr_t)c->arena + (uint64_t)q * c->slot_bytes; };
    auto slab_addr = [&](size_t u) { return (uint64_t)(uintptr_t)((const uint16_t *)s->io_px.p + L.slab_off[u]); };
    for (size_t u = 0; u < nu; u++) {
        const Owner &ow = own[un[u].owner];
        const uint32_t f = un[u].frame;
        const uint8_t oc = ow.oc[f];
        if (!head(u).temporal) { if (oc == SlotIndex::kMiss) fills.push_back(CacheFill{ L.slab_off[u], slot_addr(ow, ow.slot[f]), (uint32_t)px[u], 0 }); }
        else if (f != 0 && oc != kNotNamed) dsts[u] = oc == SlotIndex::kMiss ? slot_addr(ow, ow.slot[f]) : slab_addr(u);
        fill_first.push_back(fills.size());
    }
    {
        const GatherPiece *at = d_cached;
        for (const FrameCaches::Use &us : fc.uses) {
            if (!us.pieces.empty()) HIP_TRY(hipMemcpyAsync((void *)at, us.pieces.data(), us.pieces.size() * sizeof(GatherPiece), hipMemcpyHostToDevice, s->stream));
            at += us.pieces.size();
        }
        if (!fills.empty()) HIP_TRY(hipMemcpyAsync((void *)d_fills, fills.data(), fills.size() * sizeof(CacheFill), hipMemcpyHostToDevice, s->stream));
        if (nu) HIP_TRY(hipMemcpyAsync(d_dsts, dsts.data(), nu * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
    }
    std::vector<int32_t> ust(nu, MIC_OK);
    std::vector<uint64_t> begins, ends; std::vector<Mic2DecUnit> du;
    uint64_t nslab = 0;
    for (size_t b = 0; b < L.subs(); b++) {
        const size_t u0 = L.cuts[b];
        const int nb = (int)(L.cuts[b + 1] - u0);
        if ((rc = pack_streams(s, nb, [&](int i) { return blob_len(u0 + (size_t)i); },
                               [&](int i) { const Unit &x = un[u0 + (size_t)i]; return (const uint8_t *)own[x.owner].r->keep.data() + own[x.owner].r->pos[x.frame]; },
                               false, begins, ends))) return rc;
        du.resize((size_t)nb);
        for (int i = 0; i < nb; i++) {
            const size_t g = u0 + (size_t)i;
            du[(size_t)i] = Mic2DecUnit{ (const uint8_t *)s->io_comp.p + begins[(size_t)i], (uint32_t)blob_len(g), head(g).w, head(g).h,
                                         is_frame(g) ? (uint16_t *)s->io_px.p + L.slab_off[g] : nullptr, (uint32_t)!is_frame(g) };
        }
        if ((rc = mic2_batch_decode_units(s, du.data(), nb, ust.data() + u0))) return rc;
        nslab++;
        // the statuses are known: what failed, and the temporal runs of this sub-batch
        const size_t sp0 = spans.size();
        size_t span_px = 0;
        for (int i = 0; i < nb;) {
            const size_t g0 = u0 + (size_t)i;
            Owner &ow = own[un[g0].owner];
            int j = i + 1;
            while (j < nb && un[u0 + (size_t)j].owner == un[g0].owner) j++;
            if (!ow.r->m.temporal) {
                for (int k = i; k < j; k++) {
                    const size_t g = u0 + (size_t)k;
                    if (ust[g] != MIC_OK) { ow.code[un[g].frame] = ust[g]; ow.failed[un[g].frame] = (int32_t)un[g].frame; }
                    if (ow.oc[un[g].frame] == SlotIndex::kMiss) fc.uses[(size_t)ow.use].written.push_back(ow.slot[un[g].frame]);
                }
                i = j;
                continue;
            }
            const uint32_t npx = (uint32_t)px[g0];
            bool open = false;
            FrameSpan sp{};
            auto close = [&](uint64_t carry_out) {
                if (!open) return;
                open = false;
                sp.carry_out = carry_out;
                if (sp.nb || sp.anchor_dst || sp.carry_out) { spans.push_back(sp); span_px = std::max<size_t>(span_px, npx); }
            };
            for (int k = i; k < j; k++) {
                const size_t g = u0 + (size_t)k;
                const uint32_t f = un[g].frame;
                const bool named_miss = ow.oc[f] == SlotIndex::kMiss;
                if (f == 0 || (int64_t)f - 1 != ow.prev) {                                  // a run begins: at frame 0 in the slab, or behind an anchor in the arena
                    close(0);
                    ow.alive = true;
                    if (f == 0) {
                        if (ust[g] != MIC_OK) { ow.alive = false; ow.bad_code = ust[g]; ow.bad_frame = 0; }
                        else { sp = FrameSpan{ slab_addr(g), named_miss ? slot_addr(ow, ow.slot[0]) : 0, 0, npx, k + 1, 0, 0 }; open = true; }
                    } else {
                        const uint32_t q = ow.use >= 0 ? fc.uses[(size_t)ow.use].c->index.slot_of(SlotIndex::Key{ ow.r->owner, f - 1 }) : SlotIndex::kNoSlot;
                        if (q == SlotIndex::kNoSlot) return MIC_ERR_INTERNAL;               // (the plan stopped at a resident frame)
                        sp = FrameSpan{ slot_addr(ow, q), 0, 0, npx, k, 0, 0 };
                        open = true;
                    }
                } else if (!open && ow.alive) {                                             // the run goes on from the sub-batch before
                    sp = FrameSpan{ (uint64_t)(uintptr_t)s->crop_stage.p + ow.carry, 0, 0, npx, k, 0, 0 };
                    open = true;
                }
                if (f != 0 && ow.alive) {
                    if (ust[g] != MIC_OK) { ow.alive = false; ow.bad_code = ust[g]; ow.bad_frame = (int32_t)f; close(0); }
                    else sp.nb++;
                }
                if (!ow.alive && ow.oc[f] != kNotNamed) { ow.code[f] = ow.bad_code; ow.failed[f] = ow.bad_frame; }
                else if (named_miss) fc.uses[(size_t)ow.use].written.push_back(ow.slot[f]);
                ow.prev = (int64_t)f;
            }
            // the run goes on when the owner's next unit, in the sub-batch behind this one, is the next frame
            const size_t gn = u0 + (size_t)j;
            const bool goes_on = ow.alive && (size_t)j == (size_t)nb && gn < nu && un[gn].owner == un[g0].owner && (int64_t)un[gn].frame == ow.prev + 1;
            close(goes_on ? (uint64_t)(uintptr_t)s->crop_stage.p + ow.carry : 0);
            i = j;
        }
        const size_t nsp = spans.size() - sp0;
        s->timer.reset(s->stream);
        if (fill_first[u0 + (size_t)nb] > fill_first[u0]) {                                 // the independent misses of this sub-batch into their slots
            const size_t f0 = fill_first[u0], nf = fill_first[u0 + (size_t)nb] - f0;
            size_t max_px = 0;
            for (size_t q = f0; q < f0 + nf; q++) max_px = std::max<size_t>(max_px, fills[q].npx);
            fc.launched = true;
            s->timer.mark("k_mic2_cache_fill");
            launch_cache_fill(s->stream, kGatherPxU16, (const uint16_t *)s->io_px.p, d_fills + f0, nf, max_px);
        }
        if (nsp) {
            HIP_TRY(hipMemcpyAsync(d_spans + sp0, spans.data() + sp0, nsp * sizeof(FrameSpan), hipMemcpyHostToDevice, s->stream));
            fc.launched = true;
            s->timer.mark("k_mic2_accumulate_frames");
            hipLaunchKernelGGL(k_mic2_accumulate_frames, dim3((unsigned)nsp, (unsigned)((span_px + 2047) / 2048)), dim3(256), 0, s->stream,
                               (const MicUnit *)s->units.p, (const FrameSpan *)d_spans + sp0, (const uint64_t *)d_dsts + u0);
        }
        gather_units(s, "k_mic2_gather_crops", kGatherU16, s->io_px.p, L, b, d_out, o, (size_t)ch * (size_t)cw, behind);
        s->timer.mark("end");
        HIP_TRY(hipGetLastError());
    }
    if (fc.cached_pieces()) {                                                               // hits and fresh frames alike out of the arenas: one launch per cache
        if (L.subs() == 0) s->timer.reset(s->stream);
        const GatherPiece *at = d_cached;
        s->timer.mark("k_mic2_gather_cached");
        for (const FrameCaches::Use &us : fc.uses) {
            if (us.pieces.empty()) continue;
            fc.launched = true;
            launch_gather(s->stream, kGatherPxU16, (const uint16_t *)us.c->arena, at, us.pieces.size(), us.mw, us.mh, d_out, o.dtype,
                          o.params(out_table(s, L, behind), (size_t)ch * (size_t)cw));
            at += us.pieces.size();
        }
        s->timer.mark("end");
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    // a frame that failed, or whose chain passed a failed residual, is not kept; a crop carries the code of the first such frame it needs
    for (Owner &ow : own)
        for (uint32_t f : ow.named)
            if (ow.code[f] != MIC_OK && ow.oc[f] == SlotIndex::kMiss) fc.uses[(size_t)ow.use].c->index.release(SlotIndex::Key{ ow.r->owner, f });
    fc.finish();
    for (int i = 0; i < n; i++) { if (status) status[i] = MIC_OK; if (failed_frame) failed_frame[i] = -1; }
    std::vector<char> seen((size_t)n, 0);
    for (size_t v = 0; v < nv; v++) {
        if (owner_of[v] < 0) continue;
        const Owner &ow = own[(size_t)owner_of[v]];
        for (const CropPiece &pc : mp.vols[v].plan.pieces) {                                // (in frame order)
            if (seen[(size_t)pc.crop] || ow.code[(size_t)pc.frame] == MIC_OK) continue;
            seen[(size_t)pc.crop] = 1;
            if (status) status[pc.crop] = ow.code[(size_t)pc.frame];
            if (failed_frame) failed_frame[pc.crop] = ow.failed[(size_t)pc.frame];
        }
    }
    if (stats) *stats = mic_hip_multi_crop_stats{ nu, mp.pieces, nslab, mp.read };
    return MIC_OK;
}

// a one-volume door's call on its parsed file: arguments, n == 0, the plan, the session (leased here when s is NULL), the table
// entries of the plan's frames, `source`, then the core on a plan of that one volume
int crops_call(mic_hip_session *s, const Mic2Head &m, const std::function<int(const CropPlan &, Mic2Source &)> &source,
               const int32_t *xyz, int n, int cw, int ch, int cd, void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats,
               const mic_hip_out_spec *spec, mic_hip_mic2_reader *cached = nullptr) {
    size_t need = 0;
    OutFormat o;
    int rc = o.make(spec, 1, 16, 1);
    if (rc) return rc;
    if ((rc = mic2_crop_args(m, xyz, n, cw, ch, cd, o.pixel(), out_cap, &need))) return rc;
    if (stats) *stats = mic_hip_crop_stats{ 0, 0, 0 };
    if (n == 0) return MIC_OK;
    if (!d_out) return MIC_ERR_ARGS;
    Mic2MultiPlan mp;
    mp.vols.resize(1);
    Mic2Vol &f = mp.vols[0];
    f.named = true; f.m = m;
    if ((rc = mic2_plan_crops(m.w, m.h, m.n, m.temporal, xyz, n, cw, ch, cd, f.plan))) return rc;
    mp.units = f.plan.frames.size(); mp.pieces = f.plan.pieces.size(); mp.read = 1;
    DefaultLease lease;
    // the pointer and the table are judged before a source is asked for a byte, and before anything is launched
    if ((rc = crop_door(&s, lease, &d_out, need, o))) return rc;
    for (uint32_t fr : f.plan.frames) {                                                     // as mic_hip_mic2_decompress, multiframe.go:137-139
        const uint64_t off = 20 + 8 * (uint64_t)m.n + get_u32(m.table + 8 * (size_t)fr), bl = get_u32(m.table + 8 * (size_t)fr + 4);
        if (bl == 0 || off + bl > m.file_len) return MIC_ERR_CORRUPT;
    }
    mic_hip_multi_crop_stats ms{ 0, 0, 0, 0 };
    if (cached) {                                                                           // the reader has a frame cache: only what is not resident is fetched and decoded
        if ((rc = mic2_cached_read_crops(s, mp, std::vector<mic_hip_mic2_reader *>{ cached }, n, cw, ch, cd, o, d_out, need, status, nullptr, &ms))) return rc;
        if (stats) *stats = mic_hip_crop_stats{ ms.frames_decoded, ms.pieces, ms.slabs };
        return MIC_OK;
    }
    Mic2Source one;
    if ((rc = source(f.plan, one))) return rc;
    Mic2MultiSource src;
    src.device = one.device;
    src.blob = [&one](uint32_t, uint32_t frame) { return one.blob(frame); };
    if ((rc = mic2_multi_read_crops(s, mp, src, n, cw, ch, cd, o, d_out, need, status, nullptr, &ms))) return rc;
    if (stats) *stats = mic_hip_crop_stats{ ms.frames_decoded, ms.pieces, ms.slabs };
    return MIC_OK;
}

// what the doors check of their arguments before a file is looked at; o = the output description, *need = bytes of the crop tensor
int multi_crop_args(const void *files, const size_t *lens, int nfiles, const int32_t *xyzv, int n, int cw, int ch, int cd,
                    const mic_hip_out_spec *spec, OutFormat &o, size_t out_cap, size_t *need) {
    if (cw <= 0 || ch <= 0 || cd <= 0 || n < 0 || nfiles < 0 || (n > 0 && !xyzv) || (nfiles > 0 && (!files || !lens))) return MIC_ERR_ARGS;
    int rc = o.make(spec, 1, 16, nfiles);
    if (rc) return rc;
    if ((rc = tensor_bytes(n, cd, ch, cw, o.pixel(), out_cap, need))) return rc;
    for (int i = 0; i < n; i++) if (xyzv[4 * (size_t)i + 3] < 0 || xyzv[4 * (size_t)i + 3] >= nfiles) return MIC_ERR_ARGS;
    return MIC_OK;
}

// a door's call once its arguments stand (multi_crop_args): n == 0, the pointer and the session (leased here when s is NULL), the plan,
// `source` -- which may still refuse a volume (refuse_vol) or fail the call --, the core, then the refused volumes' codes
int multi_call(mic_hip_session *s, Mic2MultiPlan &mp, const std::function<int(Mic2MultiSource &)> &source,
               const int32_t *xyzv, int n, int cw, int ch, int cd, const OutFormat &o, void *d_out, size_t need,
               int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats, const std::vector<mic_hip_mic2_reader *> *cached = nullptr) {
    if (stats) *stats = mic_hip_multi_crop_stats{ 0, 0, 0, 0 };
    if (n == 0) return MIC_OK;
    if (!d_out) return MIC_ERR_ARGS;
    DefaultLease lease;
    int rc = crop_door(&s, lease, &d_out, need, o);                                          // judged before a file is looked at
    if (rc) return rc;
    if ((rc = mic2_multi_plan(mp, xyzv, n, cw, ch, cd))) return rc;
    if (cached) {                                                                           // some reader has a frame cache (*cached: the reader behind each volume)
        if ((rc = mic2_cached_read_crops(s, mp, *cached, n, cw, ch, cd, o, d_out, need, status, failed_frame, stats))) return rc;
    } else {
        Mic2MultiSource src;
        if ((rc = source(src))) return rc;
        if ((rc = mic2_multi_read_crops(s, mp, src, n, cw, ch, cd, o, d_out, need, status, failed_frame, stats))) return rc;
    }
    container_codes(n, status, [&](int i) { return mp.vols[(size_t)xyzv[4 * (size_t)i + 3]].status; });
    return MIC_OK;
}

}  // namespace

extern "C" {

int mic_hip_mic2_crop_plan(int width, int height, int nframes, int temporal, const int32_t *xyz, int n, int cw, int ch, int cd,
                           uint32_t *frames, size_t cap, uint64_t *nframes_out, uint64_t *npieces) try {
    if (width <= 0 || height <= 0 || nframes < 0 || n < 0 || (n > 0 && !xyz) || cw <= 0 || ch <= 0 || cd <= 0 || (cap > 0 && !frames)) return MIC_ERR_ARGS;
    CropPlan plan;
    const int rc = mic2_plan_crops(width, height, nframes, temporal != 0, xyz, n, cw, ch, cd, plan);
    if (rc) return rc;
    if (nframes_out) *nframes_out = plan.frames.size();
    if (npieces) *npieces = plan.pieces.size();
    if (plan.frames.size() > cap) return MIC_ERR_CAPACITY;
    std::copy(plan.frames.begin(), plan.frames.end(), frames);
    return MIC_OK;
} MIC_ABI_CATCH

// n crops of a MIC2 file in host memory, into a tensor on the default session's device
int mic_hip_mic2_read_crops_as(const uint8_t *c, size_t len, const int32_t *xyz, int n, int cw, int ch, int cd,
                               void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats, const mic_hip_out_spec *spec) try {
    Mic2Head m;
    int rc = parse_mic2(c, len, m);
    if (rc) return rc;
    m.table = c + 20;
    return crops_call(nullptr, m, [&](const CropPlan &, Mic2Source &src) {
        src.device = false;
        src.blob = [&m, c](uint32_t f) { return c + 20 + 8 * (size_t)m.n + get_u32(m.table + 8 * (size_t)f); };
        return MIC_OK;
    }, xyz, n, cw, ch, cd, d_out, out_cap, status, stats, spec);
} MIC_ABI_CATCH
int mic_hip_mic2_read_crops(const uint8_t *c, size_t len, const int32_t *xyz, int n, int cw, int ch, int cd,
                            void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats) {
    return mic_hip_mic2_read_crops_as(c, len, xyz, n, cw, ch, cd, d_out, out_cap, status, stats, nullptr);
}

int mic_hip_mic2_reader_open(mic_hip_read_fn read, void *user, uint64_t file_len, mic_hip_mic2_reader **out) try {
    if (!read || !out) return MIC_ERR_ARGS;
    *out = nullptr;
    std::unique_ptr<mic_hip_mic2_reader> r(new mic_hip_mic2_reader());
    r->read = read; r->user = user;
    if (file_len < 20) return MIC_ERR_CORRUPT;
    r->head.resize(20);
    if (read(user, 0, r->head.data(), 20) != 0) return MIC_ERR_IO;
    int rc = parse_mic2(r->head.data(), file_len, r->m);
    if (rc) return rc;
    r->head.resize(20 + 8 * (size_t)r->m.n);
    if (r->m.n > 0 && read(user, 20, r->head.data() + 20, 8 * (size_t)r->m.n) != 0) return MIC_ERR_IO;
    r->m.table = r->head.data() + 20;
    *out = r.release();
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_mic2_reader_info(const mic_hip_mic2_reader *r, int *width, int *height, int *nframes, int *temporal) {
    if (!r) return MIC_ERR_ARGS;
    if (width) *width = r->m.w; if (height) *height = r->m.h; if (nframes) *nframes = r->m.n; if (temporal) *temporal = r->m.temporal;
    return MIC_OK;
}

int mic_hip_mic2_reader_read_crops_as(mic_hip_mic2_reader *r, const int32_t *xyz, int n, int cw, int ch, int cd,
                                      void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats, const mic_hip_out_spec *spec) try {
    if (!r) return MIC_ERR_ARGS;
    std::lock_guard<std::mutex> lk(r->mu);
    const auto call = [&] {
        return crops_call(nullptr, r->m, [&](const CropPlan &plan, Mic2Source &src) { return r->fetch(plan, src); },
                          xyz, n, cw, ch, cd, d_out, out_cap, status, stats, spec, r->cache ? r : nullptr);
    };
    if (!r->timing) return call();
    // timed: the session is leased here, so that the call's own lease nests in it and the timer is this call's alone
    r->t_names.clear(); r->t_ms.clear();
    DefaultLease lease;
    int rc = lease.acquire();
    if (rc) return rc;
    mic_hip_session *s = cur_default();
    (void)mic_hip_session_set_timing(s, 2);
    rc = call();
    const char *names[96]; float ms[96];
    const int k = mic_hip_session_last_timings(s, names, ms, 96);
    r->t_names.assign(names, names + k); r->t_ms.assign(ms, ms + k);
    (void)mic_hip_session_set_timing(s, 0);
    return rc;
} MIC_ABI_CATCH
int mic_hip_mic2_reader_read_crops(mic_hip_mic2_reader *r, const int32_t *xyz, int n, int cw, int ch, int cd,
                                   void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats) {
    return mic_hip_mic2_reader_read_crops_as(r, xyz, n, cw, ch, cd, d_out, out_cap, status, stats, nullptr);
}

void mic_hip_mic2_reader_close(mic_hip_mic2_reader *r) {
    if (r && r->cache) r->cache->detach(r->owner);                                          // (its entries go with it)
    delete r;
}

int mic_hip_mic2_reader_set_cache(mic_hip_mic2_reader *r, mic_hip_tile_cache *c) try {
    if (!r) return MIC_ERR_ARGS;
    std::lock_guard<std::mutex> lk(r->mu);
    if (c == r->cache) return MIC_OK;
    if (c && (c->tw != r->m.w || c->th != r->m.h || c->channels != 1 || c->bps != 16)) return MIC_ERR_ARGS;
    if (r->cache) r->cache->detach(r->owner);
    r->cache = c;
    if (c) { std::lock_guard<std::mutex> lc(c->mu); c->attached++; r->owner = tile_cache_new_owner(); }
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_mic2_reader_set_timing(mic_hip_mic2_reader *r, int enabled) try {
    if (!r) return MIC_ERR_ARGS;
    std::lock_guard<std::mutex> lk(r->mu);
    r->timing = enabled != 0;
    r->t_names.clear(); r->t_ms.clear();
    return MIC_OK;
} MIC_ABI_CATCH
int mic_hip_mic2_reader_last_timings(mic_hip_mic2_reader *r, const char **names, float *ms, int cap) try {
    if (!r || cap < 0 || (cap > 0 && (!names || !ms))) return 0;
    std::lock_guard<std::mutex> lk(r->mu);
    const int k = std::min<int>(cap, (int)r->t_names.size());
    for (int i = 0; i < k; i++) { names[i] = r->t_names[(size_t)i].c_str(); ms[i] = r->t_ms[(size_t)i]; }
    return k;
} catch (...) { return 0; }

int mic_hip_mic2_reader_cache_probe(mic_hip_mic2_reader *r, const uint32_t *frames, size_t n, uint8_t *resident) try {
    if (!r || (n > 0 && (!frames || !resident))) return MIC_ERR_ARGS;
    std::lock_guard<std::mutex> lk(r->mu);
    mic_hip_tile_cache *c = r->cache;
    if (!c) { std::fill(resident, resident + n, (uint8_t)0); return MIC_OK; }
    std::lock_guard<std::mutex> lc(c->mu);
    for (size_t i = 0; i < n; i++) resident[i] = c->index.has(SlotIndex::Key{ r->owner, frames[i] }) ? 1 : 0;
    return MIC_OK;
} MIC_ABI_CATCH

// n crops of a MIC2 file that lies on the session's device: the streams go device to device
int mic_hip_session_mic2_read_crops_as(mic_hip_session *s, const uint8_t *head, size_t head_len, const uint8_t *d_file, size_t file_len,
                                       const int32_t *xyz, int n, int cw, int ch, int cd,
                                       void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats, const mic_hip_out_spec *spec) try {
    if (!s || !head) return MIC_ERR_ARGS;
    if (head_len < 20) return MIC_ERR_CORRUPT;
    Mic2Head m;
    int rc = parse_mic2(head, file_len, m);
    if (rc) return rc;
    if (head_len < 20 + 8 * (size_t)m.n) return MIC_ERR_ARGS;                            // (the table is not all there)
    m.table = head + 20;
    return crops_call(s, m, [&](const CropPlan &plan, Mic2Source &src) {
        if (!d_file && !plan.frames.empty()) return (int)MIC_ERR_ARGS;
        src.device = true;
        src.blob = [&m, d_file](uint32_t f) { return d_file + 20 + 8 * (size_t)m.n + get_u32(m.table + 8 * (size_t)f); };
        return (int)MIC_OK;
    }, xyz, n, cw, ch, cd, d_out, out_cap, status, stats, spec);
} MIC_ABI_CATCH
int mic_hip_session_mic2_read_crops(mic_hip_session *s, const uint8_t *head, size_t head_len, const uint8_t *d_file, size_t file_len,
                                    const int32_t *xyz, int n, int cw, int ch, int cd,
                                    void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats) {
    return mic_hip_session_mic2_read_crops_as(s, head, head_len, d_file, file_len, xyz, n, cw, ch, cd, d_out, out_cap, status, stats, nullptr);
}

int mic_hip_mic2_multi_crop_plan(const uint8_t *const *files, const size_t *lens, int nfiles, const int32_t *xyzv, int n, int cw, int ch, int cd,
                                 uint32_t *volume_of, uint32_t *frame_of, size_t cap, uint64_t *nframes_out, uint64_t *npieces, int32_t *file_status) try {
    size_t need = 0;
    OutFormat o;
    int rc = multi_crop_args(files, lens, nfiles, xyzv, n, cw, ch, cd, nullptr, o, ~(size_t)0, &need);
    if (rc) return rc;
    if (cap > 0 && (!volume_of || !frame_of)) return MIC_ERR_ARGS;
    Mic2MultiPlan mp;
    mp.vols.resize((size_t)nfiles);
    for (int v = 0; v < nfiles; v++) { mp.vols[(size_t)v].head = files[v]; mp.vols[(size_t)v].head_len = mp.vols[(size_t)v].file_len = lens[v]; }
    rc = mic2_multi_plan(mp, xyzv, n, cw, ch, cd);
    if (rc) return rc;
    if (file_status) for (int v = 0; v < nfiles; v++) file_status[v] = mp.vols[(size_t)v].status;
    if (nframes_out) *nframes_out = mp.units;
    if (npieces) *npieces = mp.pieces;
    if (mp.units > cap) return MIC_ERR_CAPACITY;
    size_t k = 0;
    for (int v = 0; v < nfiles; v++)
        for (uint32_t fr : mp.vols[(size_t)v].plan.frames) { volume_of[k] = (uint32_t)v; frame_of[k++] = fr; }
    return MIC_OK;
} MIC_ABI_CATCH

// n crops of MIC2 files in host memory, into a tensor on the default session's device
int mic_hip_mic2_multi_read_crops_as(const uint8_t *const *files, const size_t *lens, int nfiles, const int32_t *xyzv, int n, int cw, int ch, int cd,
                                     void *d_out, size_t out_cap, int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats,
                                     const mic_hip_out_spec *spec) try {
    size_t need = 0;
    OutFormat o;
    const int rc = multi_crop_args(files, lens, nfiles, xyzv, n, cw, ch, cd, spec, o, out_cap, &need);
    if (rc) return rc;
    Mic2MultiPlan mp;
    mp.vols.resize((size_t)nfiles);
    for (int v = 0; v < nfiles; v++) { mp.vols[(size_t)v].head = files[v]; mp.vols[(size_t)v].head_len = mp.vols[(size_t)v].file_len = lens[v]; }
    return multi_call(nullptr, mp, [&](Mic2MultiSource &src) {
        src.device = false;
        src.blob = [&mp](uint32_t v, uint32_t f) { const Mic2Head &m = mp.vols[v].m; return m.table + 8 * (size_t)m.n + get_u32(m.table + 8 * (size_t)f); };
        return (int)MIC_OK;
    }, xyzv, n, cw, ch, cd, o, d_out, need, status, failed_frame, stats);
} MIC_ABI_CATCH
int mic_hip_mic2_multi_read_crops(const uint8_t *const *files, const size_t *lens, int nfiles, const int32_t *xyzv, int n, int cw, int ch, int cd,
                                  void *d_out, size_t out_cap, int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats) {
    return mic_hip_mic2_multi_read_crops_as(files, lens, nfiles, xyzv, n, cw, ch, cd, d_out, out_cap, status, failed_frame, stats, nullptr);
}

// the same through readers (volume = an index into readers[]): every named reader's blobs are pulled before anything is launched
int mic_hip_mic2_readers_read_crops_as(mic_hip_mic2_reader *const *readers, int nreaders, const int32_t *xyzv, int n, int cw, int ch, int cd,
                                       void *d_out, size_t out_cap, int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats,
                                       const mic_hip_out_spec *spec) try {
    static const size_t no_lens = 0;                                                        // (readers bring their lengths)
    size_t need = 0;
    OutFormat o;
    const int rc = multi_crop_args(readers, &no_lens, nreaders, xyzv, n, cw, ch, cd, spec, o, out_cap, &need);
    if (rc) return rc;
    std::vector<mic_hip_mic2_reader *> named;                                               // distinct, in address order: locked once each
    for (int i = 0; i < n; i++) if (readers[xyzv[4 * (size_t)i + 3]]) named.push_back(readers[xyzv[4 * (size_t)i + 3]]);
    std::sort(named.begin(), named.end(), std::less<mic_hip_mic2_reader *>());
    named.erase(std::unique(named.begin(), named.end()), named.end());
    std::vector<std::unique_lock<std::mutex>> locks;
    locks.reserve(named.size());
    for (mic_hip_mic2_reader *r : named) locks.emplace_back(r->mu);
    Mic2MultiPlan mp;
    mp.vols.resize((size_t)nreaders);
    for (int i = 0; i < n; i++) {
        const size_t v = (size_t)xyzv[4 * (size_t)i + 3];
        if (const mic_hip_mic2_reader *r = readers[v]) { mp.vols[v].head = r->head.data(); mp.vols[v].head_len = r->head.size(); mp.vols[v].file_len = r->m.file_len; }
    }
    bool any_cache = false;
    for (mic_hip_mic2_reader *r : named) any_cache = any_cache || r->cache != nullptr;
    const std::vector<mic_hip_mic2_reader *> vol_reader(readers, readers + nreaders);
    return multi_call(nullptr, mp, [&](Mic2MultiSource &src) {
        // a reader listed as several volumes pulls the union of their frames, once
        CropPlan all;
        Mic2Source one;
        for (mic_hip_mic2_reader *r : named) {
            all.frames.clear();
            for (int v = 0; v < nreaders; v++) if (readers[v] == r) all.frames.insert(all.frames.end(), mp.vols[(size_t)v].plan.frames.begin(), mp.vols[(size_t)v].plan.frames.end());
            std::sort(all.frames.begin(), all.frames.end());
            all.frames.erase(std::unique(all.frames.begin(), all.frames.end()), all.frames.end());
            if (all.frames.empty()) continue;
            const int frc = r->fetch(all, one);
            if (frc) return frc;
        }
        src.device = false;
        src.blob = [readers](uint32_t v, uint32_t f) { return (const uint8_t *)readers[v]->keep.data() + readers[v]->pos[f]; };
        return (int)MIC_OK;
    }, xyzv, n, cw, ch, cd, o, d_out, need, status, failed_frame, stats, any_cache ? &vol_reader : nullptr);
} MIC_ABI_CATCH
int mic_hip_mic2_readers_read_crops(mic_hip_mic2_reader *const *readers, int nreaders, const int32_t *xyzv, int n, int cw, int ch, int cd,
                                    void *d_out, size_t out_cap, int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats) {
    return mic_hip_mic2_readers_read_crops_as(readers, nreaders, xyzv, n, cw, ch, cd, d_out, out_cap, status, failed_frame, stats, nullptr);
}

// n crops of MIC2 files that lie on the session's device: the streams go device to device
int mic_hip_session_mic2_multi_read_crops_as(mic_hip_session *s, const uint8_t *const *heads, const size_t *head_lens,
                                             const uint8_t *const *d_files, const size_t *lens, int nfiles,
                                             const int32_t *xyzv, int n, int cw, int ch, int cd, void *d_out, size_t out_cap,
                                             int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats, const mic_hip_out_spec *spec) try {
    if (!s) return MIC_ERR_ARGS;
    size_t need = 0;
    if (nfiles > 0 && (!head_lens || !d_files)) return MIC_ERR_ARGS;
    OutFormat o;
    const int rc = multi_crop_args(heads, lens, nfiles, xyzv, n, cw, ch, cd, spec, o, out_cap, &need);
    if (rc) return rc;
    Mic2MultiPlan mp;
    mp.vols.resize((size_t)nfiles);
    for (int v = 0; v < nfiles; v++) { mp.vols[(size_t)v].head = heads[v]; mp.vols[(size_t)v].head_len = head_lens[v]; mp.vols[(size_t)v].file_len = lens[v]; }
    return multi_call(s, mp, [&](Mic2MultiSource &src) {
        for (int v = 0; v < nfiles; v++)                                                    // (a file whose frames are needed is not there)
            if (!d_files[v] && !mp.vols[(size_t)v].plan.frames.empty()) refuse_vol(mp, mp.vols[(size_t)v], MIC_ERR_ARGS);
        src.device = true;
        src.blob = [&mp, d_files](uint32_t v, uint32_t f) { const Mic2Head &m = mp.vols[v].m; return d_files[v] + 20 + 8 * (size_t)m.n + get_u32(m.table + 8 * (size_t)f); };
        return (int)MIC_OK;
    }, xyzv, n, cw, ch, cd, o, d_out, need, status, failed_frame, stats);
} MIC_ABI_CATCH
int mic_hip_session_mic2_multi_read_crops(mic_hip_session *s, const uint8_t *const *heads, const size_t *head_lens,
                                          const uint8_t *const *d_files, const size_t *lens, int nfiles,
                                          const int32_t *xyzv, int n, int cw, int ch, int cd, void *d_out, size_t out_cap,
                                          int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats) {
    return mic_hip_session_mic2_multi_read_crops_as(s, heads, head_lens, d_files, lens, nfiles, xyzv, n, cw, ch, cd, d_out, out_cap, status, failed_frame, stats, nullptr);
}

}  // extern "C"
