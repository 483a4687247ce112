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
// Shared with the MIC3 patch and strip-file crop readers (mic_rects.h): the piece record, the sub-batch layout, the gather list and
// its launch, the independent volumes' status fold, the tensor check.  Here: the plans, the decode chain, everything temporal.
#include <climits>
#include <memory>
#include "mic_rects.h"

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

// a one-volume door's call on its parsed file: arguments, n == 0, the plan, the session (leased here when s is NULL), the table
// entries of the plan's frames, `source`, then the core on a plan of that one volume
int crops_call(mic_hip_session *s, const Mic2Head &m, const std::function<int(const CropPlan &, Mic2Source &)> &source,
               const int32_t *xyz, int n, int cw, int ch, int cd, void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats,
               const mic_hip_out_spec *spec) {
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
    Mic2Source one;
    if ((rc = source(f.plan, one))) return rc;
    Mic2MultiSource src;
    src.device = one.device;
    src.blob = [&one](uint32_t, uint32_t frame) { return one.blob(frame); };
    mic_hip_multi_crop_stats ms{ 0, 0, 0, 0 };
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
               int32_t *status, int32_t *failed_frame, mic_hip_multi_crop_stats *stats) {
    if (stats) *stats = mic_hip_multi_crop_stats{ 0, 0, 0, 0 };
    if (n == 0) return MIC_OK;
    if (!d_out) return MIC_ERR_ARGS;
    DefaultLease lease;
    int rc = crop_door(&s, lease, &d_out, need, o);                                          // judged before a file is looked at
    if (rc) return rc;
    if ((rc = mic2_multi_plan(mp, xyzv, n, cw, ch, cd))) return rc;
    Mic2MultiSource src;
    if ((rc = source(src))) return rc;
    if ((rc = mic2_multi_read_crops(s, mp, src, n, cw, ch, cd, o, d_out, need, status, failed_frame, stats))) return rc;
    container_codes(n, status, [&](int i) { return mp.vols[(size_t)xyzv[4 * (size_t)i + 3]].status; });
    return MIC_OK;
}

}  // namespace

struct mic_hip_mic2_reader {
    std::mutex mu;                          // one call at a time (and with it one callback at a time)
    mic_hip_read_fn read = nullptr; void *user = nullptr;
    Mic2Head m;
    std::vector<uint8_t> head;              // the fixed header and the frame table
    std::vector<uint8_t> keep;              // the blobs of the last call's plan, in plan order
    std::vector<size_t> pos;                // frame -> its blob's place in keep
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
    return crops_call(nullptr, r->m, [&](const CropPlan &plan, Mic2Source &src) { return r->fetch(plan, src); },
                      xyz, n, cw, ch, cd, d_out, out_cap, status, stats, spec);
} MIC_ABI_CATCH
int mic_hip_mic2_reader_read_crops(mic_hip_mic2_reader *r, const int32_t *xyz, int n, int cw, int ch, int cd,
                                   void *d_out, size_t out_cap, int32_t *status, mic_hip_crop_stats *stats) {
    return mic_hip_mic2_reader_read_crops_as(r, xyz, n, cw, ch, cd, d_out, out_cap, status, stats, nullptr);
}

void mic_hip_mic2_reader_close(mic_hip_mic2_reader *r) { delete r; }

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
    }, xyzv, n, cw, ch, cd, o, d_out, need, status, failed_frame, stats);
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
