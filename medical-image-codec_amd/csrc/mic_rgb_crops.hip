// mic_rgb_crops.hip -- single-frame RGB files (CompressRGB blobs, MICR files): many 2-D crops of many files per call into a device
// tensor (mic_hip_rgb_crop_plan, mic_hip_rgb_read_crops, mic_hip_session_rgb_read_crops; no reference counterpart).
//
// One core (rgb_read_crops) behind the two doors; a door judges the files some crop cites, brings the heads of the named ones (the
// host's bytes; k_rgb_batch_heads for blobs in device memory) and says where a blob is copied from.  The host plans (rgb_plan_crops):
// an image is one unit, so the plan is the accepted files some crop overlaps with non-empty area, each once, and those overlaps,
// pieces -- at most one per crop.  The units go through the unit codec in sub-batches under the workspace ceiling.  What is new
// against the other readers: a sub-batch's slab holds the CODED planes alone (mode 2), and the cut counts only their samples -- a grey
// ultrasound frame has one, its constant Co and Cg take no room and no fill launch --, and the gather (kGatherRGBModes, mic_gather.hip)
// takes every plane of a piece from where it is: the slab, a constant in the piece's record, the raw samples of a mode 3 plane in
// place in the blob, which lies in the compressed-input buffer for its streams' sake anyway.
// Shared with the MIC3 patch, MIC2 crop and strip-file crop readers (mic_rects.h): the piece record, the sub-batch layout, the gather
// list and its launch, the status fold and the tensor check.  Here: the judgement of a file, the plan, the cut and the decode.
#include "mic_rects.h"

namespace {

constexpr size_t kRgbCropMaxPx = (size_t)1 << 26;      // as mic_hip_rgb_decompress_batch
constexpr uint32_t kNoUnit = 0xFFFFFFFFu;

// a file of the call.  cited: some crop carries its index, so the door judges it (blob, len, w, h, status); named: it stands and
// some crop overlaps it with non-empty area, so its head is read (pl, status, failed_plane) and, when that stands too, it is a unit.
struct RgbCropFile {
    const uint8_t *blob = nullptr; uint64_t len = 0;        // the CompressRGB blob (behind a MICR header): host memory, or the session's device
    int32_t w = 0, h = 0;
    int32_t status = MIC_OK, failed_plane = -1;
    bool cited = false, named = false;
    uint32_t unit = kNoUnit;
    RgbPlaneRec pl[3];
    size_t coded() const { return (size_t)(pl[0].mode == 2) + (pl[1].mode == 2) + (pl[2].mode == 2); }
};
struct RgbCropPlan {
    std::vector<RgbCropFile> files;
    std::vector<uint32_t> units;            // the files to decode, ascending, each once
    std::vector<RectPiece> pieces;          // rect: the crop; sorted by unit (stable: crop order inside a unit)
    uint64_t planes_coded = 0;              // the units' mode 2 planes
};
typedef std::function<void(size_t f, RgbCropFile &file)> RgbJudge;                                   // blob, len, w, h and status of a cited file
typedef std::function<int(const std::vector<uint32_t> &named, std::vector<RgbHead> &heads)> RgbHeads;   // heads[k] = RgbHead of file named[k]

// what the entry points check of their arguments before a file is looked at
int rgb_crop_args(const void *files, int nfiles, const int32_t *xyf, int n, int cw, int ch) {
    if (cw <= 0 || ch <= 0 || n < 0 || nfiles < 0 || (n > 0 && !xyf) || (nfiles > 0 && !files)) return MIC_ERR_ARGS;
    return MIC_OK;
}
int rgb_crop_indices(const int32_t *xyf, int n, int nfiles) {
    for (int i = 0; i < n; i++) if (xyf[3 * (size_t)i + 2] < 0 || xyf[3 * (size_t)i + 2] >= nfiles) return MIC_ERR_ARGS;
    return MIC_OK;
}

// The plan of n crops of cw x ch over plan.files (file indices checked: rgb_crop_indices).  A file that is refused keeps its code in
// files[f].status and its crops have no pieces.
int rgb_plan_crops(RgbCropPlan &plan, const int32_t *xyf, int n, int cw, int ch, const RgbJudge &judge, const RgbHeads &heads_of) {
    plan.units.clear(); plan.pieces.clear(); plan.planes_coded = 0;
    for (int i = 0; i < n; i++) plan.files[(size_t)xyf[3 * (size_t)i + 2]].cited = true;
    for (size_t f = 0; f < plan.files.size(); f++) if (plan.files[f].cited) judge(f, plan.files[f]);
    // the clipped columns and rows of crop i in its image, when its file stands and they are not empty
    struct Clip { int64_t x0, x1, y0, y1; };
    auto clip = [&](int i, Clip &c) {
        const RgbCropFile &f = plan.files[(size_t)xyf[3 * (size_t)i + 2]];
        if (f.status != MIC_OK) return false;
        const int64_t x = xyf[3 * (size_t)i], y = xyf[3 * (size_t)i + 1];
        c.x0 = std::max<int64_t>(x, 0); c.x1 = std::min<int64_t>(x + cw, f.w); c.y0 = std::max<int64_t>(y, 0); c.y1 = std::min<int64_t>(y + ch, f.h);
        return c.x1 > c.x0 && c.y1 > c.y0;
    };
    Clip c;
    std::vector<uint32_t> named;
    for (int i = 0; i < n; i++) {
        RgbCropFile &f = plan.files[(size_t)xyf[3 * (size_t)i + 2]];
        if (!f.named && clip(i, c)) f.named = true;
    }
    for (size_t f = 0; f < plan.files.size(); f++) if (plan.files[f].named) named.push_back((uint32_t)f);
    std::vector<RgbHead> heads(named.size());
    const int rc = named.empty() ? MIC_OK : heads_of(named, heads);
    if (rc) return rc;
    for (size_t k = 0; k < named.size(); k++) {
        RgbCropFile &f = plan.files[named[k]];
        f.status = rgb_parse_head(heads[k], f.len, (size_t)f.w * (size_t)f.h, f.pl, &f.failed_plane);
        if (f.status) continue;
        f.unit = (uint32_t)plan.units.size();
        plan.units.push_back(named[k]);
        plan.planes_coded += f.coded();
    }
    std::vector<size_t> first(plan.units.size() + 1, 0);                                    // unit -> its first piece, then the next free one
    for (int i = 0; i < n; i++) if (clip(i, c)) first[(size_t)plan.files[(size_t)xyf[3 * (size_t)i + 2]].unit + 1]++;
    for (size_t u = 0; u < plan.units.size(); u++) first[u + 1] += first[u];
    plan.pieces.resize(first.back());
    for (int i = 0; i < n; i++) {
        if (!clip(i, c)) continue;
        const uint32_t u = plan.files[(size_t)xyf[3 * (size_t)i + 2]].unit;
        const int64_t x = xyf[3 * (size_t)i], y = xyf[3 * (size_t)i + 1];
        plan.pieces[first[u]++] = RectPiece{ i, u, (int32_t)c.x0, (int32_t)c.y0, (int32_t)(c.x0 - x), (int32_t)(c.y0 - y), (int32_t)(c.x1 - c.x0), (int32_t)(c.y1 - c.y0) };
    }
    return MIC_OK;
}

// Units [i0, return) of the next sub-batch: next_sub_batch over the files, a file counting the pixels of its coded planes alone.  The
// ceiling is the strip and MIC2 readers' -- a plane's tier-2 slabs and its place in the staging slab, by the largest so far -- and
// what one launch chain takes, both counted in PLANES: the capacity keeps the coded planes of the items it has been asked about.
size_t rgb_crop_cut(const std::vector<size_t> &npx, const std::vector<size_t> &coded, size_t i0, size_t budget) {
    size_t planes = 0;
    return next_sub_batch(i0, npx.size(), [&](size_t i) { return coded[i] ? npx[i] : (size_t)0; },
                          [&](size_t i, size_t mp) {
                              planes += coded[i];
                              const size_t room = std::min<size_t>(65535, budget / (unit_ws_bytes(std::max<size_t>(mp, 1)) + 2 * mp));
                              return planes <= room ? ~(size_t)0 : (size_t)0;
                          }, CutRule{ ~(size_t)0 });
}

// n crops into d_out ([n][ch][cw][3] u8, or o's tensor; an address s's device can write: patch_pointer) on a session the caller holds
// and has made current.  device: the blobs lie on the session's device.
int rgb_read_crops(mic_hip_session *s, const RgbCropPlan &plan, bool device, int n, int cw, int ch, const OutFormat &o,
                   void *d_out, size_t need, int32_t *status, int32_t *failed_plane, mic_hip_rgb_crop_stats *stats) {
    const size_t nu = plan.units.size();
    int rc;
    if ((rc = s->ensure(1, 1))) return rc;                                                  // (the session's stream)
    if ((rc = fill_pad(s->stream, o, d_out, need))) return rc;                              // outside the images, refused files
    auto file = [&](size_t u) -> const RgbCropFile & { return plan.files[plan.units[u]]; };
    std::vector<size_t> npx(nu), coded(nu);
    for (size_t u = 0; u < nu; u++) { npx[u] = (size_t)file(u).w * (size_t)file(u).h; coded[u] = file(u).coded(); }
    const size_t budget = kWorkspaceBudget;
    const RectBatches L = rect_batches(nu, [&](size_t i0) { return rgb_crop_cut(npx, coded, i0, budget); },
                                       [&](size_t u) { return coded[u] * rgb_stride(npx[u]); }, plan.pieces, cw, ch,
                                       [&](size_t u) { return UnitStride{ file(u).w, 0 }; }, [&](size_t u) { return plan.units[u]; }, o);
    // a sub-batch's blobs lie back to back in s->io_comp, as pack_streams puts them: unit u's at comp_off[u]
    std::vector<uint64_t> comp_off(nu);
    size_t comp_max = 0;
    for (size_t b = 0; b < L.subs(); b++) {
        uint64_t comp = 0;
        for (size_t u = L.cuts[b]; u < L.cuts[b + 1]; u++) { comp_off[u] = comp; comp += file(u).len; }
        comp_max = std::max<size_t>(comp_max, (size_t)comp);
    }
    // the reader's own records behind the gather list: where each plane of piece q is (RgbPlaneSrc)
    std::vector<RgbPlaneSrc> recs(plan.pieces.size());
    for (size_t q = 0; q < recs.size(); q++) {
        const RectPiece &p = plan.pieces[q];
        const RgbCropFile &f = file(p.unit);
        const uint64_t at = (uint64_t)p.sy * (uint64_t)f.w + (uint64_t)p.sx;                  // the piece's first sample in a plane of its image
        RgbPlaneSrc r;
        memset(&r, 0, sizeof r);
        for (size_t k = 0, c = 0; k < 3; k++) {
            const RgbPlaneRec &pr = f.pl[k];
            if (pr.mode == 2) { r.kind[k] = kPlaneSlab; r.at[k] = L.slab_off[p.unit] + c++ * rgb_stride(npx[p.unit]) + at; }
            else if (pr.mode == 3) { r.kind[k] = kPlaneRaw; r.at[k] = comp_off[p.unit] + pr.off + 2 * at; }   // (rgb_parse_head: 2 npx bytes from pr.off lie inside the blob)
            else { r.kind[k] = kPlaneConst; r.value[k] = pr.mode == 1 ? pr.value : 0; }
        }
        recs[q] = r;
    }
    const size_t behind = recs.size() * sizeof(RgbPlaneSrc);
    if (nu) {
        if ((rc = s->io_comp.reserve(comp_max + 64))) return rc;                            // (once: pack_streams then finds room for every sub-batch)
        if ((rc = s->io_px.reserve(L.slab_max * 2 + 64))) return rc;
        if ((rc = upload_gather(s, L, o, behind))) return rc;
        HIP_TRY(hipMemcpyAsync((char *)s->pieces.p + gather_bytes(L), recs.data(), behind, hipMemcpyHostToDevice, s->stream));
    }
    std::vector<int32_t> ust(nu, MIC_OK), uplane(nu, -1);                                   // unit u: its first failing plane's code, and that plane
    std::vector<uint64_t> begins, ends, sb, se; std::vector<mic_hip_unit> units; std::vector<uint32_t> plane_of; std::vector<int32_t> pst;
    uint64_t nslab = 0;                                                                     // decode chains run
    for (size_t b = 0; b < L.subs(); b++) {
        const size_t u0 = L.cuts[b];
        const int nb = (int)(L.cuts[b + 1] - u0);
        if ((rc = pack_streams(s, nb, [&](int i) { return file(u0 + (size_t)i).len; }, [&](int i) { return file(u0 + (size_t)i).blob; }, device, begins, ends))) return rc;
        units.clear(); sb.clear(); se.clear(); plane_of.clear();
        for (int i = 0; i < nb; i++) {
            const size_t u = u0 + (size_t)i;
            const RgbCropFile &f = file(u);
            for (size_t k = 0, c = 0; k < 3; k++) {
                if (f.pl[k].mode != 2) continue;
                units.push_back(mic_hip_unit{ L.slab_off[u] + c++ * rgb_stride(npx[u]), f.w, f.h, 0, 0 });
                sb.push_back(begins[(size_t)i] + f.pl[k].off); se.push_back(begins[(size_t)i] + f.pl[k].off + f.pl[k].len);
                plane_of.push_back((uint32_t)(3 * u + k));
            }
        }
        if (!units.empty()) {                                                               // ONE unit decode over every mode-2 plane of the sub-batch
            if ((rc = session_decode_enqueue_spans(s, (const uint8_t *)s->io_comp.p, sb.data(), se.data(), units.data(), (int)units.size(), (uint16_t *)s->io_px.p))) return rc;
            pst.assign(units.size(), MIC_OK);
            if ((rc = session_decode_finish(s, pst.data()))) return rc;
            nslab++;
            for (size_t q = 0; q < pst.size(); q++) {
                const size_t u = plane_of[q] / 3;
                if (pst[q] != MIC_OK && ust[u] == MIC_OK) { ust[u] = pst[q]; uplane[u] = (int32_t)(plane_of[q] % 3); }   // "Y plane: %w", wsicompress.go:446-461
            }
        }
        s->timer.reset(s->stream);
        gather_units(s, "k_rgb_gather_crops", kGatherRGBModes, s->io_px.p, L, b, d_out, o, (size_t)ch * (size_t)cw, behind, s->io_comp.p);
        s->timer.mark("end");
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    fold_unit_status(plan.pieces, ust, n, 1, status, failed_plane, [&](uint32_t u) { return uplane[u]; });
    if (stats) *stats = mic_hip_rgb_crop_stats{ plan.planes_coded, 3 * (uint64_t)nu, plan.pieces.size(), nslab };
    return MIC_OK;
}

// a door's call: the tensor, the file indices, n == 0, the pointer, the plan, then the core on session s (leased here when s is NULL)
int rgb_call(mic_hip_session *s, RgbCropPlan &plan, const RgbJudge &judge, const RgbHeads &heads_of, bool device,
             const int32_t *xyf, int n, int cw, int ch, void *d_out, size_t out_cap, int32_t *status, int32_t *failed_plane,
             mic_hip_rgb_crop_stats *stats, const mic_hip_out_spec *spec) {
    size_t need = 0;
    OutFormat o;
    int rc = o.make(spec, 3, 8, (int)plan.files.size());
    if (rc) return rc;
    if ((rc = tensor_bytes(n, 1, ch, cw, o.pixel(), out_cap, &need))) return rc;
    if ((rc = rgb_crop_indices(xyf, n, (int)plan.files.size()))) return rc;
    if (stats) *stats = mic_hip_rgb_crop_stats{ 0, 0, 0, 0 };
    if (n == 0) return MIC_OK;
    if (!d_out) return MIC_ERR_ARGS;
    DefaultLease lease;
    if ((rc = crop_door(&s, lease, &d_out, need, o))) return rc;                            // (the pointer is judged before a blob's head is asked for)
    if ((rc = rgb_plan_crops(plan, xyf, n, cw, ch, judge, heads_of))) return rc;
    if ((rc = rgb_read_crops(s, plan, device, n, cw, ch, o, d_out, need, status, failed_plane, stats))) return rc;
    container_codes(n, status, [&](int i) { return plan.files[(size_t)xyf[3 * (size_t)i + 2]].status; });
    for (int i = 0; failed_plane && i < n; i++) {                                           // (... and the plane the file's code is about)
        const RgbCropFile &f = plan.files[(size_t)xyf[3 * (size_t)i + 2]];
        if (f.status != MIC_OK) failed_plane[i] = f.failed_plane;
    }
    return MIC_OK;
}

// the host doors' files: mic_hip_rgb_decompress_batch's judgement of a job, less its output buffer
RgbJudge host_judge(const mic_hip_rgb_file *files) {
    return [files](size_t k, RgbCropFile &f) {
        const mic_hip_rgb_file &j = files[k];
        f.failed_plane = -1;
        if (!j.data || j.width < 0 || j.height < 0 || (j.container != 0 && j.container != 1)) { f.status = MIC_ERR_ARGS; return; }
        f.blob = j.data; f.len = j.len; f.w = j.width; f.h = j.height;
        if (j.container) {                                                                  // readMICRFile: the header names the size
            int w = 0, h = 0;
            if ((f.status = mic_hip_micr_info(j.data, j.len, &w, &h))) return;
            if ((j.width || j.height) && (j.width != w || j.height != h)) { f.status = MIC_ERR_ARGS; return; }
            f.blob += 12; f.len -= 12; f.w = w; f.h = h;
        } else if (j.width == 0 || j.height == 0) { f.status = MIC_ERR_ARGS; return; }
        f.status = (size_t)f.w * (size_t)f.h > kRgbCropMaxPx ? MIC_ERR_UNSUPPORTED : MIC_OK;
    };
}
RgbHeads host_heads(const RgbCropPlan &plan) {
    return [&plan](const std::vector<uint32_t> &named, std::vector<RgbHead> &heads) {
        for (size_t k = 0; k < named.size(); k++) rgb_head_of(plan.files[named[k]].blob, plan.files[named[k]].len, heads[k]);
        return MIC_OK;
    };
}

}  // namespace

extern "C" {

int mic_hip_rgb_crop_plan(const mic_hip_rgb_file *files, int nfiles, const int32_t *xyf, int n, int cw, int ch,
                          uint32_t *file_of, size_t cap, uint64_t *nfiles_out, uint64_t *nplanes_coded, uint64_t *npieces, int32_t *file_status) try {
    int rc = rgb_crop_args(files, nfiles, xyf, n, cw, ch);
    if (rc) return rc;
    if (cap > 0 && !file_of) return MIC_ERR_ARGS;
    if ((rc = rgb_crop_indices(xyf, n, nfiles))) return rc;
    RgbCropPlan plan;
    plan.files.resize((size_t)nfiles);
    if ((rc = rgb_plan_crops(plan, xyf, n, cw, ch, host_judge(files), host_heads(plan)))) return rc;
    if (file_status) for (int f = 0; f < nfiles; f++) file_status[f] = plan.files[(size_t)f].status;
    if (nfiles_out) *nfiles_out = plan.units.size();
    if (nplanes_coded) *nplanes_coded = plan.planes_coded;
    if (npieces) *npieces = plan.pieces.size();
    if (plan.units.size() > cap) return MIC_ERR_CAPACITY;
    std::copy(plan.units.begin(), plan.units.end(), file_of);
    return MIC_OK;
} MIC_ABI_CATCH

// n crops of RGB files in host memory, into a tensor on the default session's device
int mic_hip_rgb_read_crops_as(const mic_hip_rgb_file *files, int nfiles, const int32_t *xyf, int n, int cw, int ch,
                              void *d_out, size_t out_cap, int32_t *status, int32_t *failed_plane, mic_hip_rgb_crop_stats *stats,
                              const mic_hip_out_spec *spec) try {
    const int rc = rgb_crop_args(files, nfiles, xyf, n, cw, ch);
    if (rc) return rc;
    RgbCropPlan plan;
    plan.files.resize((size_t)nfiles);
    return rgb_call(nullptr, plan, host_judge(files), host_heads(plan), false, xyf, n, cw, ch, d_out, out_cap, status, failed_plane, stats, spec);
} MIC_ABI_CATCH
int mic_hip_rgb_read_crops(const mic_hip_rgb_file *files, int nfiles, const int32_t *xyf, int n, int cw, int ch,
                           void *d_out, size_t out_cap, int32_t *status, int32_t *failed_plane, mic_hip_rgb_crop_stats *stats) {
    return mic_hip_rgb_read_crops_as(files, nfiles, xyf, n, cw, ch, d_out, out_cap, status, failed_plane, stats, nullptr);
}

// n crops of CompressRGB blobs that lie on the session's device: the heads come down through k_rgb_batch_heads, the blobs go device to device
int mic_hip_session_rgb_read_crops_as(mic_hip_session *s, const uint8_t *d_blobs, const uint64_t *h_offsets,
                                      const mic_hip_rgb_image *imgs, int nfiles, const int32_t *xyf, int n, int cw, int ch,
                                      void *d_out, size_t out_cap, int32_t *status, int32_t *failed_plane, mic_hip_rgb_crop_stats *stats,
                                      const mic_hip_out_spec *spec) try {
    if (!s) return MIC_ERR_ARGS;
    const int rc = rgb_crop_args(imgs, nfiles, xyf, n, cw, ch);
    if (rc) return rc;
    if (nfiles > 0 && (!d_blobs || !h_offsets)) return MIC_ERR_ARGS;
    RgbCropPlan plan;
    plan.files.resize((size_t)nfiles);
    const RgbJudge judge = [&](size_t k, RgbCropFile &f) {
        f.failed_plane = -1;
        if (imgs[k].width <= 0 || imgs[k].height <= 0 || h_offsets[k + 1] < h_offsets[k]) { f.status = MIC_ERR_ARGS; return; }
        f.blob = d_blobs + h_offsets[k]; f.len = h_offsets[k + 1] - h_offsets[k]; f.w = imgs[k].width; f.h = imgs[k].height;
        f.status = (size_t)f.w * (size_t)f.h > kRgbCropMaxPx ? MIC_ERR_UNSUPPORTED : MIC_OK;
    };
    // the heads of the named blobs (asked for once the session is current): their ranges up, one thread per blob, the heads down in one copy
    const RgbHeads heads_of = [&](const std::vector<uint32_t> &named, std::vector<RgbHead> &heads) -> int {
        const size_t m = named.size(), range_b = 2 * m * 8, head_b = m * sizeof(RgbHead);
        int rc2;
        if ((rc2 = s->ensure(1, 1))) return rc2;                                            // (the session's stream)
        if ((rc2 = s->rgb_aux.reserve(range_b + head_b + 64)) || (rc2 = s->rgb_pin.reserve((range_b + head_b) / 8 + 1))) return rc2;
        uint64_t *h_range = s->rgb_pin.p;                                                   // m begins, then m ends
        for (size_t k = 0; k < m; k++) { h_range[k] = h_offsets[named[k]]; h_range[m + k] = h_offsets[named[k] + 1]; }
        RgbHead *h_heads = (RgbHead *)(s->rgb_pin.p + 2 * m);
        uint64_t *d_range = (uint64_t *)s->rgb_aux.p;
        RgbHead *d_heads = (RgbHead *)((char *)s->rgb_aux.p + range_b);
        HIP_TRY(hipMemcpyAsync(d_range, h_range, range_b, hipMemcpyHostToDevice, s->stream));
        if ((rc2 = rgb_heads_enqueue(s->stream, d_blobs, d_range, d_range + m, (int)m, d_heads))) return rc2;
        HIP_TRY(hipMemcpyAsync(h_heads, d_heads, head_b, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        std::copy(h_heads, h_heads + m, heads.begin());
        return MIC_OK;
    };
    return rgb_call(s, plan, judge, heads_of, true, xyf, n, cw, ch, d_out, out_cap, status, failed_plane, stats, spec);
} MIC_ABI_CATCH
int mic_hip_session_rgb_read_crops(mic_hip_session *s, const uint8_t *d_blobs, const uint64_t *h_offsets,
                                   const mic_hip_rgb_image *imgs, int nfiles, const int32_t *xyf, int n, int cw, int ch,
                                   void *d_out, size_t out_cap, int32_t *status, int32_t *failed_plane, mic_hip_rgb_crop_stats *stats) {
    return mic_hip_session_rgb_read_crops_as(s, d_blobs, h_offsets, imgs, nfiles, xyf, n, cw, ch, d_out, out_cap, status, failed_plane, stats, nullptr);
}

}  // extern "C"
