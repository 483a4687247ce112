// mic_decode.hip -- decode kernels of the MIC unit codec for gfx950.
//
//   k_dec_tans_gl      one wave per N-state stream, table in L2: what the lane-per-state kernels of mic_decode_ls.hip leave
//                      (tableLog-16 tables with 0-bit entries); walks a frame's RLE headers as it goes (mic_rlewalk.h)
//   k_dec_tans_serial  one lane per stream: 1-state streams (fsedecompressu16.go:267-377) and whatever nobody else took
//   k_dec_gap_check    gap removal's checking decode path (mic_gap.hip); and mic_launch_decode, the decode chain's launcher
//   Tables: mic_tables.hip; tANS per lane, states -> symbols: mic_decode_ls.hip; tokens -> pixels: mic_decode_px.hip, _rows.hip, _fused.hip.
//
// Launch shape: blockIdx.x = unit.
#include "mic_dev.h"
#include "mic_fse_tables.h"
#include "mic_launch.h"
#include "mic_rlewalk.h"

// Reverse bit reader (bitreader.go): the highest set bit of the last byte is the end mark;
// bits are consumed from there towards the front.  `cursor` = number of unread bits.
struct BitR {
    const uint8_t *in; uint64_t cursor; bool over;
    __device__ bool init(const uint8_t *p, uint32_t len) {            // bitreader.go:27-47
        if (len < 1) return false;
        uint8_t v = p[len - 1];
        if (v == 0) return false;
        in = p; over = false;
        cursor = 8ull * (len - 1) + (uint32_t)(31 - __clz((uint32_t)v));
        return true;
    }
    __device__ uint32_t get(uint32_t n) {                             // getBits32, :49-61
        if (n == 0) return 0;
        if (cursor < n) { over = true; cursor = 0; return 0; }
        cursor -= n;
        uint64_t byte = cursor >> 3;
        uint32_t sh = (uint32_t)(cursor & 7);
        uint64_t w = 0;
        for (uint32_t k = 0; k < 4; k++) {                            // n <= 16 -> at most 3 bytes
            w |= (uint64_t)in[byte + k] << (8 * k);
            if (8 * (k + 1) >= sh + n) break;
        }
        return (uint32_t)((w >> sh) & ((1ull << n) - 1));
    }
};

// v0: one lane decodes the stream (the caller's lane 0; u.status == MICD_OK, u.ntok == 0): u.tok[0, u.ntok) or an error status.
__device__ __noinline__ void dec_tans_serial_body(MicUnit &u) {
    const uint32_t tl = u.table_log;
    const uint32_t *dt = u.tt_nb;
    const uint16_t *ds = u.tab_sym;
    BitR br;
    if (u.bits_off > u.comp_len || !br.init(u.comp_in + u.bits_off, u.comp_len - u.bits_off)) { u.status = MICD_ERR_CORRUPT; return; }
    uint16_t *out = u.tok;
    if (u.flavour == 1) {
        // decompress(), fsedecompressu16.go:267-377: run until the bits are used up and the
        // current state needs more; a non-zero final state contributes one more symbol.
        // (a one-state stream does not say how many tokens it holds: the token slab is found full only here.  Tier 1's holds what a
        // well-formed frame of few escapes needs; a frame of more tokens -- two per escaped pixel, or one of many short segments -- runs
        // again in tier 2 like a stream of the other flavours whose count says so, mic_tables.hip)
        const int32_t full = u.tier == 1 ? MICD_INT_GROW : MICD_ERR_CORRUPT;
        uint32_t state = br.get(tl);
        uint32_t n = 0;
        for (;;) {
            uint32_t e = dt[state];
            uint32_t nb = e >> 16;
            if (br.cursor == 0 && nb > 0) {
                if (state != 0) { if (n >= u.tok_cap) { u.status = full; return; } out[n++] = ds[state]; }
                break;
            }
            uint32_t low = br.get(nb);
            if (br.over) { u.status = MICD_ERR_CORRUPT; return; }
            if (n >= u.tok_cap) { u.status = full; return; }
            out[n++] = ds[state];
            state = (e & 0xFFFF) + low;
        }
        u.ntok = n;
        return;
    }
    const uint32_t lanes = (u.flavour == 108) ? 8 : u.flavour;
    uint32_t st[8];
    for (uint32_t k = 0; k < lanes; k++) st[k] = br.get(tl);
    if (br.over) { u.status = MICD_ERR_CORRUPT; return; }
    const uint32_t count = u.count;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t k = i & (lanes - 1);
        uint32_t e = dt[st[k]];
        uint32_t low = br.get(e >> 16);
        if (br.over) { u.status = MICD_ERR_CORRUPT; return; }
        out[i] = ds[st[k]];
        st[k] = (e & 0xFFFF) + low;
    }
    u.ntok = count;
}
// grid = units, block = 64
__global__ void __launch_bounds__(64) k_dec_tans_serial(MicUnit *units) {
    MicUnit &u = units[blockIdx.x];
    if (threadIdx.x != 0 || u.status != MICD_OK) return;
    if (u.ntok != 0) return;                                           // a fast variant already decoded it
    dec_tans_serial_body(u);
    u.dec_kernel = MIC_DEC_BY_SERIAL;
}

// Gap removal's checking path (mic_gap.hip: k_dec_gap_expand parks a unit whose table gives weight to a compact symbol >= numSymbols
// in MICD_GAP_CHECK, its tab_sym left compact, so that no other decoder takes it): lane 0 decodes the compact symbols serially,
// then the wave expands them through the map -- MIC_ERR_CORRUPT exactly when one of them is out of range, as
// gapremovalcompressu16.go:270-273 fails.  The pixel kernels behind take the tokens as they take a one-state stream's.
__global__ void __launch_bounds__(64) k_dec_gap_check(MicUnit *units) {
    MicUnit &u = units[blockIdx.x];
    if (u.status != MICD_GAP_CHECK) return;
    const uint32_t lane = threadIdx.x;
    int st = 0; uint32_t ntok = 0;
    if (lane == 0) { u.status = MICD_OK; u.ntok = 0; dec_tans_serial_body(u); st = u.status; ntok = u.ntok; }
    MIC_GROUP_HANDOFF();                                               // (lane 0's token stores, then every lane reads them)
    st = __shfl(st, 0, 64); ntok = (uint32_t)__shfl((int)ntok, 0, 64);
    if (st != MICD_OK) return;
    const uint32_t lim = min(u.gap_nsym, u.tab_cap);                   // (the expand table holds the map's first tab_cap entries)
    mic_gp<uint16_t> tok = mic_g(u.tok);
    const mic_gp<const uint16_t> ex = mic_g((const uint16_t *)u.gap_buf);
    bool bad = false;
    for (uint32_t i = lane; i < ntok; i += 64) {
        const uint32_t c = tok[i];
        if (c >= lim) bad = true;
        else tok[i] = ex[c];
    }
    if (__any(bad) && lane == 0) u.status = MICD_ERR_CORRUPT;
}

// ==========================================================================================
// One wave per stream, the transition table left in HBM / L2 (u32 entries newState | nbBits << 16, as the
// tables kernel writes them): for tableLog 16 -- every 16-bit-depth frame, CT above all -- the table has
// 65536 entries and a 17-bit nextState, too much for LDS.  A chain step is then an L2 round trip instead
// of an LDS one, but a wave needs only the 1.3 KiB ring + stage, so a CU holds as many streams as it has
// wave slots and hides that latency with them.  64-symbol chunks (a chunk may take 64 x 16 bits off the
// ring).  Takes every N-state stream the LDS classes left (tableLog > 15); 1-state streams stay serial.
#define TD_RING 256                               // dwords of a stream's bit-window ring
#define TG_CH 64
template <int N>
__global__ void __launch_bounds__(64) k_dec_tans_gl(MicUnit *units) {
    __shared__ uint32_t s_gl[TD_RING + 4 + TG_CH / 2];
    MicUnit &u = units[blockIdx.x];
    if (u.status != MICD_OK) return;
    const uint32_t flav = u.flavour;
    if (flav == 1 || ((flav == 108) ? 8u : flav) != (uint32_t)N) return;
    if (u.ntok != 0) return;                                            // already decoded by an LDS class
    const uint32_t tl = u.table_log;
    if (u.bits_off >= u.comp_len) { if (threadIdx.x == 0) u.status = MICD_ERR_CORRUPT; return; }
    const uint32_t len = u.comp_len - u.bits_off;
    if (len >= (1u << 27)) return;                                      // bit positions are 32-bit here; the serial kernel takes it
    const uint32_t lane = threadIdx.x;
    uint32_t *ring = s_gl;
    uint32_t *stage = ring + TD_RING + 4;
    typedef const __attribute__((address_space(1))) uint16_t *gcu16;
    typedef const __attribute__((address_space(1))) uint32_t *gcu32;
    typedef __attribute__((address_space(1))) uint16_t *gu16;
    typedef __attribute__((address_space(1))) uint32_t *gu32;
    const gcu32 tabg = (gcu32)u.tt_nb;
    const gcu16 symg = (gcu16)u.tab_sym;
    const uint32_t count = mic_sym_ceiling(u, u.count);                 // (a ceiling is a multiple of 128: no tail behind it)
    const gu16 out = (gu16)u.tok;
    const uint8_t *bs = u.comp_in + u.bits_off;
    const uint32_t last = bs[len - 1];
    if (last == 0) { if (lane == 0) u.status = MICD_ERR_CORRUPT; return; }  // bitreader.go:36-38
    const uintptr_t addr = (uintptr_t)bs;
    const uint32_t sb = (uint32_t)(addr & 3);
    const gcu32 g = (gcu32)(addr - sb);
    const int32_t cur0 = (int32_t)(8u * (len - 1) + (uint32_t)(31 - __clz(last)) + 8u * sb);
    const int32_t top_dw = (cur0 - 1) >> 5;
    auto load_blk = [&](int32_t b) -> uint32_t {
        const int32_t idx = b * 64 + (int32_t)lane;
        return (b >= 0 && idx <= top_dw) ? __builtin_nontemporal_load(g + idx) : 0u;
    };
    auto store_blk = [&](int32_t b, uint32_t v) {
        const uint32_t slot = ((uint32_t)b & 3u) * 64u + lane;
        ring[slot] = v;
        if (slot == 0) ring[TD_RING] = v;
    };
    int32_t q = cur0 - 32;
    int32_t blk = (q >> 5) >> 6;
    store_blk(blk + 1, load_blk(blk + 1));
    store_blk(blk, load_blk(blk));
    store_blk(blk - 1, load_blk(blk - 1));
    uint32_t pf = load_blk(blk - 2);
    __syncthreads();
    auto window = [&](int32_t qq) -> uint32_t {
        const uint32_t *w = ring + (((uint32_t)qq >> 5) & (TD_RING - 1));
        return __builtin_amdgcn_alignbit(w[1], w[0], (uint32_t)qq);
    };
    auto take = [](uint32_t hi, uint32_t nb) -> uint32_t { return (uint32_t)(((uint64_t)hi << nb) >> 32); };   // top nb bits, nb = 0 .. 32
    uint32_t st[N];
#pragma unroll
    for (int p = 0; p < N; p++) { st[p] = window(q) >> (32u - tl); q -= (int32_t)tl; }
    auto group = [&](uint32_t *stage_w) {
        uint32_t e[N];
#pragma unroll
        for (int k = 0; k < N; k++) e[k] = tabg[st[k]];
#pragma unroll
        for (int p = 0; p < N; p += 2) {
            const uint32_t hi = window(q);
            stage_w[p >> 1] = st[p] | (st[p + 1] << 16);
            const uint32_t nb0 = e[p] >> 16, nb1 = e[p + 1] >> 16;           // <= 16 each
            st[p] = (e[p] & 0xFFFFu) + take(hi, nb0);
            st[p + 1] = (e[p + 1] & 0xFFFFu) + take(hi << nb0, nb1);
            q -= (int32_t)(nb0 + nb1);
        }
    };
    auto single = [&](int k, uint16_t *stage_h) {
        const uint32_t e = tabg[st[k]];
        const uint32_t hi = window(q);
        *stage_h = (uint16_t)st[k];
        const uint32_t nb = e >> 16;
        st[k] = (e & 0xFFFFu) + take(hi, nb);
        q -= (int32_t)nb;
    };
    // header walker (mic_rlewalk.h): a chunk's headers are read out of the registers that hold its tokens
    const bool frame = u.mode == 0 && u.seg != nullptr;
    MicRleWalk wk; wk.init(u, frame, count);
    auto walk = [&](uint32_t cend, auto get) {
        while (wk.on && wk.pos < cend) {
            const uint32_t h = get(wk.pos);
            if (wk.pos == 0) wk.first(h); else wk.step(h, lane);
        }
    };
    constexpr uint32_t G = TG_CH / N;
    const uint32_t chunks = count / TG_CH;
    uint32_t pend_lo = 0, pend_hi = 0; bool have_pend = false;
    uint32_t obase = 0;
    auto flush_pend = [&]() {
        if (!have_pend) return;
        const uint32_t pk = pend_lo | (pend_hi << 16);
        if (lane < TG_CH / 2) __builtin_nontemporal_store(pk, (gu32)out + obase + lane);
        const uint32_t cb = obase * 2;
        walk(cb + TG_CH, [&](uint32_t pos) -> uint32_t {
            const uint32_t rel = pos - cb;
            const uint32_t pair = __builtin_amdgcn_readlane(pk, rel >> 1);
            return (rel & 1) ? (pair >> 16) : (pair & 0xFFFFu);
        });
    };
    for (uint32_t ch = 0; ch < chunks; ch++) {
#pragma unroll 4
        for (uint32_t gi = 0; gi < G; gi++) group(stage + gi * (N / 2));
        store_blk(blk - 2, pf);
        flush_pend();
        blk = (q >> 5) >> 6;
        pf = load_blk(blk - 2);
        const uint32_t s2 = stage[lane & (TG_CH / 2 - 1)];
        pend_lo = symg[s2 & 0xFFFF]; pend_hi = symg[s2 >> 16];
        have_pend = true; obase = ch * (TG_CH / 2);
    }
    flush_pend();
    {
        const uint32_t done = chunks * TG_CH;
        const uint32_t rem = count - done;
        uint32_t k = 0;
        for (; k + N <= rem; k += N) group(stage + (k / 2));
        uint16_t *st16 = (uint16_t *)stage;
#pragma unroll
        for (int j = 0; j < N - 1; j++) if (k + (uint32_t)j < rem) single(j, st16 + k + j);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        uint32_t tv0 = 0;
        if (lane < rem) { tv0 = symg[st16[lane]]; out[done + lane] = (uint16_t)tv0; }
        walk(count, [&](uint32_t pos) -> uint32_t { return __builtin_amdgcn_readlane(tv0, pos - done); });
    }
    if (lane == 0) {
        u.dec_kernel = MIC_DEC_BY_GL;
        if (count == u.count && q + 32 - (int32_t)(8u * sb) < 0) u.status = MICD_ERR_CORRUPT;   // bitreader.go:113-120 (a prefix reads less)
        else {
            u.ntok = count;
            if (frame && !wk.err) wk.finish(u);
        }
    }
}

void mic_launch_decode(MicUnit *d_units, int n, hipStream_t stream, int variant, MicTimer *t, int *d_cls, uint32_t pred_mask, uint32_t cls_mask,
                       const MicSplitCfg *split) {
    const bool any_grad = (variant & MIC_VARIANT_GRAD) != 0, gap = (variant & MIC_VARIANT_GAP) != 0;
    if (gap) mic_launch_dec_gap_map(d_units, n, stream, t);
    if (t) t->mark("k_dec_tables_wg");
    // (classes 0-5: tableLog 13, 24-29: tableLog <= 12 -- what the compact table instance can take; a mask of all ones: unknown)
    mic_launch_dec_tables(d_units, n, stream, (cls_mask & (0x3F00003Fu | MIC_CLS_SPLIT)) != 0);
    if (gap) mic_launch_dec_gap_expand(d_units, n, stream, t);
    // lane-per-state kernels over compacted per-class lists (mic_decode_ls.hip): every table size has its class; what they leave
    // (a tableLog-16 table with 0-bit entries, 1-state streams) falls through to the kernels below, which skip decoded units
    mic_launch_dec_tans_ls(d_units, n, d_cls + MIC_CLS_HEAD, d_cls, stream, t, cls_mask, split);
    if (t) t->mark("k_dec_tans_gl<2>");
    hipLaunchKernelGGL(k_dec_tans_gl<2>, dim3(n), dim3(64), 0, stream, d_units);
    if (t) t->mark("k_dec_tans_gl<4,8>");
    hipLaunchKernelGGL(k_dec_tans_gl<4>, dim3(n), dim3(64), 0, stream, d_units);
    hipLaunchKernelGGL(k_dec_tans_gl<8>, dim3(n), dim3(64), 0, stream, d_units);
    if (gap) { if (t) t->mark("k_dec_gap_check"); hipLaunchKernelGGL(k_dec_gap_check, dim3(n), dim3(64), 0, stream, d_units); }
    if (t) t->mark("k_dec_tans_serial");
    hipLaunchKernelGGL(k_dec_tans_serial, dim3(n), dim3(64), 0, stream, d_units);
    mic_launch_decode_pixels(d_units, n, stream, t, any_grad, pred_mask);
    if (t) t->mark("end");
}
