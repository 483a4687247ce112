// mic_strip_crops.hip -- strip files (PICS, PICA): many 2-D crops of many files per call into a device tensor
// (mic_hip_strips_crop_plan, mic_hip_strips_read_crops, mic_hip_session_strips_read_crops; no reference counterpart).
//
// One core (strips_read_crops) behind the two doors; a door brings, per file, the bytes its header and table are read from and the
// address its streams are copied from (the caller's file, a file in device memory).  The host plans (strips_plan_crops): a strip is a
// unit of its own, so a crop needs the strips it overlaps and no others -- the plan is those (file, strip) units, each once, and the
// (crop, strip) overlaps, pieces.  The units go through the unit codec in sub-batches under the workspace ceiling, each into a slab
// of decoded strips, and behind each sub-batch the shared gather copies its pieces out of the slab into the crop tensor.
// Shared with the MIC3 patch and MIC2 crop readers (mic_rects.h): the piece record, the sub-batch layout, the gather list and its
// launch, the status fold and the tensor check.  Here: the strip tables, the plan, the capacity of a sub-batch and its decode.
#include "mic_rects.h"

namespace {

// a file of the call: where its header and table are read (host) and what they said
struct StripFile {
    const uint8_t *head = nullptr; size_t head_len = 0, len = 0;
    bool named = false;                     // some crop names it: only then is it looked at
    int32_t status = MIC_OK;
    int w = 0, h = 0, n = 0;
    std::vector<StripEntry> e;              // its strips (status == MIC_OK): rows ascending and disjoint, which strip_entry_check's non-empty ranges make them in both containers
    std::vector<uint32_t> count;            // pieces of each strip, then the strip's unit (kNoUnit: no crop overlaps it)
};
constexpr uint32_t kNoUnit = 0xFFFFFFFFu;
struct StripUnit { uint32_t file, strip; };
struct StripPlan {
    std::vector<StripFile> files;
    std::vector<StripUnit> units;           // the strips to entropy-decode, ascending by file, then strip, each once
    std::vector<RectPiece> pieces;          // rect: the crop; sorted by unit (stable: crop order inside a unit)
    uint64_t strips_total = 0;              // strips of the files some crop names
};

// header and table of file f: PICS or PICA by the magic, the checks of mic_hip_pics_info / mic_hip_pica_info against the whole file's
// length and those the whole-image decoders make of every entry (strip_entry_check)
void parse_strip_file(StripFile &f) {
    f.status = MIC_OK;
    if (!f.head) { f.status = MIC_ERR_ARGS; return; }
    if (f.head_len < 16) { f.status = MIC_ERR_CORRUPT; return; }
    const bool pica = memcmp(f.head, "PICA", 4) == 0;
    if (!pica && f.head_len < 20) { f.status = MIC_ERR_CORRUPT; return; }
    f.status = pica ? mic_hip_pica_info(f.head, f.len, &f.w, &f.h, &f.n) : mic_hip_pics_info(f.head, f.len, &f.w, &f.h, &f.n, nullptr);
    if (f.status) return;
    if (f.head_len < (pica ? 16 + 16 * (size_t)f.n : 20 + 8 * (size_t)f.n)) { f.status = MIC_ERR_ARGS; return; }   // (the table is not all there)
    f.e.resize((size_t)f.n);
    for (int k = 0; k < f.n && f.status == MIC_OK; k++) {
        f.e[(size_t)k] = pica ? pica_strip_entry(f.head, f.h, f.n, k) : pics_strip_entry(f.head, f.h, f.n, k);
        f.status = strip_entry_check(f.e[(size_t)k], f.w, f.h, f.len);
    }
    if (f.status) f.e.clear();
}

// The plan of n crops of cw x ch over the files (head, head_len, len set by the caller).  MIC_ERR_ARGS for a file index outside the
// list; a file that is refused keeps its code in files[f].status and its crops have no pieces.
int strips_plan_crops(StripPlan &plan, const int32_t *xyf, int n, int cw, int ch) {
    const int nfiles = (int)plan.files.size();
    plan.units.clear(); plan.pieces.clear(); plan.strips_total = 0;
    for (int i = 0; i < n; i++) {
        const int32_t f = xyf[3 * (size_t)i + 2];
        if (f < 0 || f >= nfiles) return MIC_ERR_ARGS;
        plan.files[(size_t)f].named = true;
    }
    for (StripFile &f : plan.files) {
        if (!f.named) continue;
        parse_strip_file(f);
        if (f.status == MIC_OK) { plan.strips_total += (uint64_t)f.n; f.count.assign((size_t)f.n, 0); }
    }
    // the strips [k0, k1) crop i overlaps with non-empty area, and its clipped columns and rows
    struct Clip { int64_t x0, x1, y0, y1; size_t k0, k1; };
    auto clip = [&](int i, Clip &c) {
        const StripFile &f = plan.files[(size_t)xyf[3 * (size_t)i + 2]];
        if (f.status != MIC_OK) return false;
        const int64_t x = xyf[3 * (size_t)i], y = xyf[3 * (size_t)i + 1];
        c.x0 = std::max<int64_t>(x, 0); c.x1 = std::min<int64_t>(x + cw, f.w); c.y0 = std::max<int64_t>(y, 0); c.y1 = std::min<int64_t>(y + ch, f.h);
        if (c.x1 <= c.x0 || c.y1 <= c.y0) return false;
        c.k0 = (size_t)(std::partition_point(f.e.begin(), f.e.end(), [&](const StripEntry &e) { return e.y1 <= c.y0; }) - f.e.begin());
        c.k1 = (size_t)(std::partition_point(f.e.begin(), f.e.end(), [&](const StripEntry &e) { return e.y0 < c.y1; }) - f.e.begin());
        return c.k0 < c.k1;
    };
    Clip c;
    for (int i = 0; i < n; i++)
        if (clip(i, c)) for (size_t k = c.k0; k < c.k1; k++) plan.files[(size_t)xyf[3 * (size_t)i + 2]].count[k]++;
    std::vector<size_t> first;                                                              // unit -> its first piece, then the next free one
    size_t total = 0;
    for (size_t fi = 0; fi < plan.files.size(); fi++) {
        StripFile &f = plan.files[fi];
        for (size_t k = 0; k < f.count.size(); k++) {
            const uint32_t cnt = f.count[k];
            f.count[k] = cnt ? (uint32_t)plan.units.size() : kNoUnit;
            if (!cnt) continue;
            if (plan.units.size() >= kNoUnit - 1) return MIC_ERR_UNSUPPORTED;
            plan.units.push_back(StripUnit{ (uint32_t)fi, (uint32_t)k });
            first.push_back(total);
            total += cnt;
        }
    }
    plan.pieces.resize(total);
    for (int i = 0; i < n; i++) {
        if (!clip(i, c)) continue;
        const StripFile &f = plan.files[(size_t)xyf[3 * (size_t)i + 2]];
        const int64_t x = xyf[3 * (size_t)i], y = xyf[3 * (size_t)i + 1];
        for (size_t k = c.k0; k < c.k1; k++) {
            const StripEntry &e = f.e[k];
            const int64_t r0 = std::max<int64_t>(c.y0, e.y0), r1 = std::min<int64_t>(c.y1, e.y1);
            plan.pieces[first[f.count[k]]++] = RectPiece{ i, f.count[k], (int32_t)c.x0, (int32_t)(r0 - e.y0), (int32_t)(c.x0 - x), (int32_t)(r0 - y),
                                                          (int32_t)(c.x1 - c.x0), (int32_t)(r1 - r0) };
        }
    }
    return MIC_OK;
}

// what the entry points check of their arguments before a file is looked at
int strips_crop_args(const void *files, const size_t *lens, int nfiles, const int32_t *xyf, int n, int cw, int ch) {
    if (cw <= 0 || ch <= 0 || n < 0 || nfiles < 0 || (n > 0 && !xyf) || (nfiles > 0 && (!files || !lens))) return MIC_ERR_ARGS;
    return MIC_OK;
}

}  // namespace

// Units [i0, i1) of the next sub-batch: as many as the workspace ceiling holds of the largest of them -- a unit's tier-2 slabs and its
// strip in the staging slab, as every MIC2 chain counts a frame (mic2_batch_cuts) -- and at most what one launch chain takes.
size_t micapi::next_strip_cut(const std::vector<size_t> &px, size_t i0, size_t budget) {
    return next_sub_batch(i0, px.size(), [&](size_t i) { return px[i]; },
                          [&](size_t, size_t mp) { return budget / (unit_ws_bytes(mp) + 2 * mp); }, CutRule{ 65535 });
}
size_t micapi::next_strip_cut(const std::vector<size_t> &px, size_t i0) { return next_strip_cut(px, i0, kWorkspaceBudget); }

namespace {

// n crops into d_out ([n][ch][cw] samples of o's type, an address s's device can write: patch_pointer) on a session the caller holds
// and has made current.  base[f]: where file f's bytes lie -- on the host, or (device) on the session's device.
int strips_read_crops(mic_hip_session *s, const StripPlan &plan, const uint8_t *const *base, bool device, int n, int cw, int ch, const OutFormat &o,
                      void *d_out, size_t need, int32_t *status, int32_t *failed_strip, mic_hip_strip_crop_stats *stats) {
    const size_t nu = plan.units.size();
    int rc;
    if ((rc = s->ensure(1, 1))) return rc;                                                  // (the session's stream)
    if ((rc = fill_pad(s->stream, o, d_out, need))) return rc;                              // outside the images, rows no strip covers, refused files
    auto entry = [&](size_t u) -> const StripEntry & { return plan.files[plan.units[u].file].e[plan.units[u].strip]; };
    auto width = [&](size_t u) { return plan.files[plan.units[u].file].w; };
    std::vector<size_t> px(nu);
    for (size_t u = 0; u < nu; u++) px[u] = (size_t)width(u) * (size_t)(entry(u).y1 - entry(u).y0);
    const RectBatches L = rect_batches(nu, [&](size_t i0) { return next_strip_cut(px, i0); }, [&](size_t u) { return px[u]; },
                                       plan.pieces, cw, ch, [&](size_t u) { return UnitStride{ width(u), 0 }; },
                                       [&](size_t u) { return plan.units[u].file; }, o);
    size_t comp_max = 0;                                                                    // the most stream bytes of a sub-batch
    for (size_t b = 0, comp = 0; b < L.subs(); b++, comp = 0)
        for (size_t u = L.cuts[b]; u < L.cuts[b + 1]; u++) comp_max = std::max(comp_max, comp += entry(u).len);
    if (nu) {
        if ((rc = s->io_comp.reserve(comp_max + 64))) return rc;                            // (once: pack_streams then finds room for every sub-batch)
        if ((rc = s->io_px.reserve(L.slab_max * 2 + 64))) return rc;
        if ((rc = upload_gather(s, L, o))) return rc;
    }
    std::vector<int32_t> ust(nu, MIC_OK);                                                   // status of unit u
    std::vector<uint64_t> begins, ends; std::vector<mic_hip_unit> units;
    for (size_t b = 0; b < L.subs(); b++) {
        const size_t u0 = L.cuts[b];
        const int nb = (int)(L.cuts[b + 1] - u0);
        if ((rc = pack_streams(s, nb, [&](int i) { return (uint64_t)entry(u0 + (size_t)i).len; },
                               [&](int i) { return base[plan.units[u0 + (size_t)i].file] + entry(u0 + (size_t)i).start; }, device, begins, ends))) return rc;
        units.resize((size_t)nb);
        for (int i = 0; i < nb; i++) {
            const StripEntry &e = entry(u0 + (size_t)i);
            units[(size_t)i] = mic_hip_unit{ L.slab_off[u0 + (size_t)i], width(u0 + (size_t)i), (int32_t)(e.y1 - e.y0), 0, e.flags };
        }
        if ((rc = session_decode_enqueue_spans(s, (const uint8_t *)s->io_comp.p, begins.data(), ends.data(), units.data(), nb, (uint16_t *)s->io_px.p))) return rc;
        if ((rc = session_decode_finish(s, ust.data() + u0))) return rc;
        s->timer.reset(s->stream);
        gather_units(s, "k_strips_gather_crops", kGatherU16, s->io_px.p, L, b, d_out, o, (size_t)ch * (size_t)cw);
        s->timer.mark("end");
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    fold_unit_status(plan.pieces, ust, n, 1, status, failed_strip, [&](uint32_t u) { return (int32_t)plan.units[u].strip; });   // (pieces are in strip order inside a crop's file)
    if (stats) *stats = mic_hip_strip_crop_stats{ nu, plan.strips_total, plan.pieces.size(), L.subs() };
    return MIC_OK;
}

// a door's call: arguments, n == 0, the plan, the pointer, then the core on session s (leased here when s is NULL)
int strips_call(mic_hip_session *s, StripPlan &plan, const uint8_t *const *base, bool device, const int32_t *xyf, int n, int cw, int ch,
                void *d_out, size_t out_cap, int32_t *status, int32_t *failed_strip, mic_hip_strip_crop_stats *stats, const mic_hip_out_spec *spec) {
    size_t need = 0;
    OutFormat o;
    int rc = o.make(spec, 1, 16, (int)plan.files.size());
    if (rc) return rc;
    if ((rc = tensor_bytes(n, 1, ch, cw, o.pixel(), out_cap, &need))) return rc;
    if ((rc = strips_plan_crops(plan, xyf, n, cw, ch))) return rc;
    if (stats) *stats = mic_hip_strip_crop_stats{ 0, 0, 0, 0 };
    if (n == 0) return MIC_OK;
    if (!d_out) return MIC_ERR_ARGS;
    if (device) for (const StripUnit &u : plan.units) if (!base[u.file]) return MIC_ERR_ARGS;    // (a file whose strips are needed is not there)
    DefaultLease lease;
    if ((rc = crop_door(&s, lease, &d_out, need, o))) return rc;
    if ((rc = strips_read_crops(s, plan, base, device, n, cw, ch, o, d_out, need, status, failed_strip, stats))) return rc;
    container_codes(n, status, [&](int i) { return plan.files[(size_t)xyf[3 * (size_t)i + 2]].status; });
    return MIC_OK;
}

}  // namespace

extern "C" {

int mic_hip_strips_crop_plan(const uint8_t *const *files, const size_t *lens, int nfiles, const int32_t *xyf, int n, int cw, int ch,
                             uint32_t *file_of, uint32_t *strip_of, size_t cap, uint64_t *nstrips_out, uint64_t *npieces, int32_t *file_status) try {
    int rc = strips_crop_args(files, lens, nfiles, xyf, n, cw, ch);
    if (rc) return rc;
    if (cap > 0 && (!file_of || !strip_of)) return MIC_ERR_ARGS;
    StripPlan plan;
    plan.files.resize((size_t)nfiles);
    for (int f = 0; f < nfiles; f++) { plan.files[(size_t)f].head = files[f]; plan.files[(size_t)f].head_len = plan.files[(size_t)f].len = lens[f]; }
    if ((rc = strips_plan_crops(plan, xyf, n, cw, ch))) return rc;
    if (file_status) for (int f = 0; f < nfiles; f++) file_status[f] = plan.files[(size_t)f].status;
    if (nstrips_out) *nstrips_out = plan.units.size();
    if (npieces) *npieces = plan.pieces.size();
    if (plan.units.size() > cap) return MIC_ERR_CAPACITY;
    for (size_t u = 0; u < plan.units.size(); u++) { file_of[u] = plan.units[u].file; strip_of[u] = plan.units[u].strip; }
    return MIC_OK;
} MIC_ABI_CATCH

// n crops of strip files in host memory, into a tensor on the default session's device
int mic_hip_strips_read_crops_as(const uint8_t *const *files, const size_t *lens, int nfiles, const int32_t *xyf, int n, int cw, int ch,
                                 void *d_out, size_t out_cap, int32_t *status, int32_t *failed_strip, mic_hip_strip_crop_stats *stats,
                                 const mic_hip_out_spec *spec) try {
    const int rc = strips_crop_args(files, lens, nfiles, xyf, n, cw, ch);
    if (rc) return rc;
    StripPlan plan;
    plan.files.resize((size_t)nfiles);
    for (int f = 0; f < nfiles; f++) { plan.files[(size_t)f].head = files[f]; plan.files[(size_t)f].head_len = plan.files[(size_t)f].len = lens[f]; }
    return strips_call(nullptr, plan, files, false, xyf, n, cw, ch, d_out, out_cap, status, failed_strip, stats, spec);
} MIC_ABI_CATCH
int mic_hip_strips_read_crops(const uint8_t *const *files, const size_t *lens, int nfiles, const int32_t *xyf, int n, int cw, int ch,
                              void *d_out, size_t out_cap, int32_t *status, int32_t *failed_strip, mic_hip_strip_crop_stats *stats) {
    return mic_hip_strips_read_crops_as(files, lens, nfiles, xyf, n, cw, ch, d_out, out_cap, status, failed_strip, stats, nullptr);
}

// n crops of strip files that lie on the session's device: the streams go device to device
int mic_hip_session_strips_read_crops_as(mic_hip_session *s, const uint8_t *const *heads, const size_t *head_lens,
                                         const uint8_t *const *d_files, const size_t *lens, int nfiles,
                                         const int32_t *xyf, int n, int cw, int ch,
                                         void *d_out, size_t out_cap, int32_t *status, int32_t *failed_strip, mic_hip_strip_crop_stats *stats,
                                         const mic_hip_out_spec *spec) try {
    if (!s) return MIC_ERR_ARGS;
    const int rc = strips_crop_args(heads, lens, nfiles, xyf, n, cw, ch);
    if (rc) return rc;
    if (nfiles > 0 && (!head_lens || !d_files)) return MIC_ERR_ARGS;
    StripPlan plan;
    plan.files.resize((size_t)nfiles);
    for (int f = 0; f < nfiles; f++) { plan.files[(size_t)f].head = heads[f]; plan.files[(size_t)f].head_len = head_lens[f]; plan.files[(size_t)f].len = lens[f]; }
    return strips_call(s, plan, d_files, true, xyf, n, cw, ch, d_out, out_cap, status, failed_strip, stats, spec);
} MIC_ABI_CATCH
int mic_hip_session_strips_read_crops(mic_hip_session *s, const uint8_t *const *heads, const size_t *head_lens,
                                      const uint8_t *const *d_files, const size_t *lens, int nfiles,
                                      const int32_t *xyf, int n, int cw, int ch,
                                      void *d_out, size_t out_cap, int32_t *status, int32_t *failed_strip, mic_hip_strip_crop_stats *stats) {
    return mic_hip_session_strips_read_crops_as(s, heads, head_lens, d_files, lens, nfiles, xyf, n, cw, ch, d_out, out_cap, status, failed_strip, stats, nullptr);
}

}  // extern "C"
