// mic_rlewalk.h -- the RLE header rule of the token stream (rledecompressu16.go:59-85) in one place, and the serial header walk of
// the entropy kernels.  Token 0 fixes midCount; a header h <= midCount is a RUN of h symbols of the token behind it, a larger one a
// LITERAL chunk of the h - midCount tokens behind it; the next header follows the payload.  Record: {payload token | run << 31, first symbol}.
#pragma once
#include "mic_dev.h"
// midCount from token 0 (rledecompressu16.go:21-25); false: a zero token, which no stream may start with
__device__ __forceinline__ bool mic_rle_mid(uint32_t tok0, uint32_t &mid) {
    const int d0 = mic_len16(tok0 & 0xFFFFu);
    mid = d0 ? (1u << (d0 - 1)) - 1u : 0u;
    return d0 != 0;
}
// One header, classified.  h = 0 is the caller's to judge first: MicRleWalk stops at it, the kernels that report errors read it as 65536.
struct MicRleHdr {
    bool run; uint32_t len, adv;                   // run or literal chunk, the symbols it yields, the tokens to the next header
    __device__ __forceinline__ uint32_t rec(uint32_t pos) const { return (pos + 1u) | (run ? 0x80000000u : 0u); }   // record .x of the header at token pos
};
__device__ __forceinline__ MicRleHdr mic_rle_hdr(uint32_t h, uint32_t mid) {
    const bool run = h <= mid;
    const uint32_t len = run ? h : h - mid;
    return MicRleHdr{ run, len, run ? 2u : 1u + len };
}
// The serial walk of a frame's headers by one wave (all values uniform): k_dec_tans_gl and the header-to-header branch of
// k_dec_translate feed it one header at a time, each from its own registers.  It stops WITHOUT an error when the stream has the symbols
// its pixels can use, and WITH one at a zero header, a full segment slab or a run whose value lies behind the last token: the
// segments are then dropped and k_dec_pixels_wg walks the stream itself and reports it.
struct MicRleWalk {
    typedef uint32_t v2 __attribute__((ext_vector_type(2)));
    bool on, err;
    uint32_t pos, out, nseg, mid;                  // the next header's token, symbols and records in front of it, midCount
    uint32_t ntok, symcap, segcap;                 // tokens of the stream, symbols the pixels can use, records the slab holds
    mic_gp<v2> seg;
    __device__ __forceinline__ void init(const MicUnit &u, bool on_, uint32_t ntok_) {
        on = on_; err = false; pos = out = nseg = mid = 0; ntok = ntok_;
        symcap = min(u.sym_cap, 2u * (uint32_t)u.w * (uint32_t)u.h + 2u); segcap = u.seg_cap;
        seg = (mic_gp<v2>)u.seg;
    }
    __device__ __forceinline__ void fail() { on = false; err = true; }
    // token 0 (pos == 0)
    __device__ __forceinline__ void first(uint32_t tok0) { if (mic_rle_mid(tok0, mid)) pos = 1; else fail(); }
    // the header at token pos; returns the tokens to the next header, 0 when the walk has stopped
    __device__ __forceinline__ uint32_t step(uint32_t h, uint32_t lane) {
        if (out >= symcap) { on = false; return 0; }
        if (h == 0 || nseg >= segcap) { fail(); return 0; }
        const MicRleHdr hd = mic_rle_hdr(h, mid);
        if (hd.run && pos + 1 >= ntok) { fail(); return 0; }
        if (lane == 0) { v2 r; r.x = hd.rec(pos); r.y = out; seg[nseg] = r; }
        nseg++; out += hd.len; pos += hd.adv;
        return hd.adv;
    }
    __device__ __forceinline__ void finish(MicUnit &u) const { u.nseg = nseg; u.nsym = min(out, symcap); u.dec_stage = MIC_STAGE_SEGS; }   // (one lane, no error)
};
