// mic_rects.h -- the host core of the readers of many rectangles per call (MIC3 patches: mic_api_ext.hip; strip-file crops:
// mic_strip_crops.hip; MIC2 crops: mic_mic2_crops.hip; RGB file crops: mic_rgb_crops.hip), written once.  A reader plans for
// itself -- the units to entropy-decode and the (rectangle, unit) overlaps, pieces -- and decodes a sub-batch its own way; around
// that it calls, in this order: rect_batches, upload_gather; per sub-batch gather_units behind the decode; after the call's one
// synchronise fold_unit_status and container_codes.
#pragma once
#include "mic_session.h"
#include "mic_pieces.h"
#include "mic_staged.h"

namespace micapi {

// One overlap of rectangle `rect` of the call with unit `unit` of the plan: w x h samples from (sx, sy) of the unit to (dx, dy) of the
// rectangle.  The output is rectangles of ch x cw back to back: a MIC2 crop of cd slices brings rect = crop * cd + slice.  A plan's
// pieces are sorted by unit (stable: rectangle order inside a unit).
struct RectPiece { int32_t rect; uint32_t unit; int32_t sx, sy, dx, dy, w, h; };

// *need = the bytes of a tensor of n x d x h x w samples (each factor >= 0), which out_cap must hold
inline int tensor_bytes(int n, int d, int h, int w, size_t sample_bytes, size_t out_cap, size_t *need) {
    const unsigned __int128 bytes = (unsigned __int128)n * (unsigned)d * (unsigned)h * (unsigned)w * sample_bytes;
    *need = (size_t)bytes;
    return bytes > out_cap ? MIC_ERR_CAPACITY : MIC_OK;
}

// Sub-batch b = units [cuts[b], cuts[b + 1]); unit u starts slab_off[u] samples into its sub-batch's slab; slab_max: the largest slab.
// list[q]: piece q as the kernels read it; first[u] .. first[u + 1]: the pieces of unit u; mw[b] x mh[b]: the largest piece of
// sub-batch b, which sizes its launch's grid y.
struct RectBatches {
    std::vector<size_t> cuts{ 0 }, first; std::vector<uint64_t> slab_off; size_t slab_max = 0;
    std::vector<GatherPiece> list; std::vector<int> mw, mh;  size_t subs() const { return cuts.size() - 1; }
};
// A piece's place in a tensor of rectangles of ch x cw laid out as o says, and the samples between its rows there: a typed RGB tensor
// counts in samples, not pixels -- interleaved, three a pixel; channels first, three planes of ch x cw a rectangle and the place the
// one in plane 0.  Multiplied out in 64 bits.
struct PieceDst { uint64_t dst; int32_t dstride; };
inline PieceDst piece_dst(const RectPiece &p, int cw, int ch, const OutFormat &o) {
    const uint64_t per_px = o.typed() && !o.planar() ? (uint64_t)o.channels : 1, per_rect = o.planar() ? (uint64_t)o.channels : 1;
    return PieceDst{ (((uint64_t)p.rect * per_rect * (uint64_t)ch + (uint64_t)p.dy) * (uint64_t)cw + (uint64_t)p.dx) * per_px, (int32_t)(cw * (int)per_px) };
}
struct UnitStride { int32_t row, plane; };          // samples between a unit's rows in the slab, and between its planes (RGB tiles; else 0)
// nu units: next(i0) ends the sub-batch that starts at i0 (next_sub_batch under the reader's rule); samples(u) is what unit u takes of
// the slab (P planes of a tile, a strip, a frame; 0: not decoded into it).  A piece's two places are multiplied out in 64 bits.
// source(u): the source unit u belongs to, which a piece carries to the typed kernels.  o: the tensor's layout -- a typed RGB tensor
// counts a piece's place in samples, not pixels: interleaved, three a pixel; channels first, three planes of ch x cw a rectangle
// and the place the one in plane 0.
template <class Next, class Samples, class Stride, class Source>
RectBatches rect_batches(size_t nu, Next &&next, Samples &&samples, const std::vector<RectPiece> &pieces, int cw, int ch, Stride &&stride,
                         Source &&source, const OutFormat &o) {
    RectBatches B;
    B.slab_off.resize(nu); B.first.assign(nu + 1, 0); B.list.resize(pieces.size());
    while (B.cuts.back() < nu) {
        const size_t u0 = B.cuts.back(), u1 = next(u0);
        size_t off = 0;
        for (size_t u = u0; u < u1; u++) { B.slab_off[u] = off; off += samples(u); }
        B.slab_max = std::max(B.slab_max, off);
        B.cuts.push_back(u1);
    }
    B.mw.assign(B.subs(), 1); B.mh.assign(B.subs(), 1);
    for (size_t q = 0, b = 0; q < pieces.size(); q++) {
        const RectPiece &p = pieces[q];
        while (p.unit >= B.cuts[b + 1]) b++;
        const UnitStride st = stride((size_t)p.unit);
        const PieceDst pd = piece_dst(p, cw, ch, o);
        B.list[q] = GatherPiece{ B.slab_off[p.unit] + (uint64_t)p.sy * (uint64_t)st.row + (uint64_t)p.sx, pd.dst, st.row,
                                 pd.dstride, p.w, p.h, st.plane, (int32_t)source((size_t)p.unit) };
        B.first[(size_t)p.unit + 1]++;
        B.mw[b] = std::max(B.mw[b], p.w); B.mh[b] = std::max(B.mh[b], p.h);
    }
    for (size_t u = 0; u < nu; u++) B.first[u + 1] += B.first[u];
    return B;
}
// the list at the head of s->pieces (gather_bytes of it), which is reserved for it and `behind` bytes more (a reader's own records);
// a typed call's affine table lies behind both (out_table)
inline size_t gather_bytes(const RectBatches &B) { return align_up(B.list.size() * sizeof(GatherPiece), 16); }
inline const void *out_table(const mic_hip_session *s, const RectBatches &B, size_t behind) { return (const char *)s->pieces.p + gather_bytes(B) + align_up(behind, 16); }
inline int upload_gather(mic_hip_session *s, const RectBatches &B, const OutFormat &o, size_t behind = 0) {
    const int rc = s->pieces.reserve(gather_bytes(B) + align_up(behind, 16) + (o.typed() ? o.table_bytes() : 0) + 64);
    if (rc == MIC_OK && !B.list.empty()) HIP_TRY(hipMemcpyAsync(s->pieces.p, B.list.data(), B.list.size() * sizeof(GatherPiece), hipMemcpyHostToDevice, s->stream));
    if (rc == MIC_OK && o.typed()) HIP_TRY(hipMemcpyAsync((void *)out_table(s, B, behind), o.table.data(), o.table_bytes(), hipMemcpyHostToDevice, s->stream));
    return rc;
}
// the pieces of sub-batch b out of its decoded slab into d_out, timed as `label`; the caller resets the timer before and marks "end" behind.
// plane: the samples of one rectangle's plane (ch x cw), which a channels-first tensor's kernel steps by.  raw (kGatherRGBModes): the
// buffer the raw planes lie in; the pieces' RgbPlaneSrc records are the first thing behind the list.
inline void gather_units(mic_hip_session *s, const char *label, GatherKind kind, const void *slab, const RectBatches &B, size_t b, void *d_out,
                         const OutFormat &o, size_t plane, size_t behind = 0, const void *raw = nullptr) {
    const size_t p0 = B.first[B.cuts[b]], np = B.first[B.cuts[b + 1]] - p0;
    if (!np) return;
    s->timer.mark(label);
    launch_gather(s->stream, kind, (const uint16_t *)slab, (const GatherPiece *)s->pieces.p + p0, np, B.mw[b], B.mh[b], d_out, o.dtype,
                  o.params(out_table(s, B, behind), plane),
                  RgbModeArgs{ (const uint8_t *)raw, (const RgbPlaneSrc *)((const char *)s->pieces.p + gather_bytes(B)) + p0 });
}

// status[r] / failed[r] (may be NULL) of rectangle r = piece.rect / per of n: MIC_OK / -1, or its first failing unit's in piece order / label(it)
template <class Label>
void fold_unit_status(const std::vector<RectPiece> &pieces, const std::vector<int32_t> &unit_status, int n, int per, int32_t *status, int32_t *failed, Label &&label) {
    std::vector<char> seen((size_t)n, 0);
    for (int i = 0; i < n; i++) { if (status) status[i] = MIC_OK; if (failed) failed[i] = -1; }
    for (const RectPiece &p : pieces) {
        const size_t r = (size_t)(p.rect / per);
        if (seen[r] || unit_status[p.unit] == MIC_OK) continue;
        seen[r] = 1;
        if (status) status[r] = unit_status[p.unit];
        if (failed) failed[r] = label(p.unit);
    }
}
// status[i] = code(i) where that is not MIC_OK: a rectangle of a refused container has no pieces and carries the container's code
template <class Code>
void container_codes(int n, int32_t *status, Code &&code) {
    for (int i = 0; status && i < n; i++) { const int32_t c = code(i); if (c != MIC_OK) status[i] = c; }
}

}  // namespace micapi
