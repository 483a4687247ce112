// mic_gap.hip -- gap removal around the unit codec: CompressSingleFrameGapRemoval / DecompressSingleFrameGapRemoval
// (gapremovalcompressu16.go:52-176, :178-282).
//
// The format is a container around the Delta+RLE tokens and the FSE stream the unit codec already writes:
//   mode 0x00            || CompressSingleFrame's bytes
//   mode 0x01 raw        || u16 numSymbols || numSymbols x u16 token value        || FSE of the compact indices
//   mode 0x02 bitmap     || u16 maxSym || bitmap (bit i of byte i / 8, LSB first) || ...   (read, never written: see k_enc_gap)
//   mode 0x03 delta      || u16 numSymbols || u16 e[0] || gap bytes (<= 254, else 0xFF + u16 LE) || ...
// Encode: the tokeniser has counted the histogram; k_enc_gap finds the used values, decides (:83-111), compacts the histogram in
// place and writes the map; k_enc_tables_wg and the tANS encoders then build and code the compact alphabet unchanged, after
// k_enc_gap_remap has rewritten the tokens; k_enc_gap_len puts the map's bytes into blob_len and k_enc_pack writes them first.
// Decode: k_dec_gap_map parses the map into an expand table and moves the unit past it, so that k_dec_parse and every kernel behind
// it see a plain FSE stream; k_dec_gap_expand rewrites tab_sym (symbol of each state) through the map once the tables stand, so the
// decoders emit the original tokens at no cost per symbol, in the class of the COMPACT table's log.
#include "mic_launch.h"
#include "mic_wave.h"

#define GAP_THREADS 256
#define GAP_WAVES (GAP_THREADS / 64)
#define GAP_CHUNK (GAP_THREADS * 4)          // histogram bins per step: four per thread (one 16-byte load)

// exclusive prefix sum over the work-group; *total = the sum of all.  (every thread calls it; it ends on a barrier)
__device__ __forceinline__ uint32_t gap_scan_add(uint32_t v, uint32_t *s_w, uint32_t *total) {
    const uint32_t ex = mic_group_excl_add<GAP_WAVES>(v, s_w, total);
    __syncthreads();
    return ex;
}
// exclusive prefix maximum (identity -1) and the maximum of all, of values >= -1: scanned as v + 1 on the unsigned maximum, whose
// identity is 0.  (it ends on a barrier too)
__device__ __forceinline__ int32_t gap_scan_max(int32_t v, int32_t *s_w, int32_t *total) {
    uint32_t all;
    const uint32_t ex = mic_group_excl_max<GAP_WAVES>((uint32_t)(v + 1), (uint32_t *)s_w, &all);
    __syncthreads();
    *total = (int32_t)all - 1;
    return (int32_t)ex - 1;
}

// One step of the walk over the histogram: the four bins of this thread at `base`, the used values among them, their compact
// indices, the gap of each to the value used before it and the delta map's escapes (gap >= 255) in front of it.  WRITE = the second
// walk, which compacts the histogram, fills the compact-index table and writes the map entries.
template <bool WRITE>
__device__ __forceinline__ void gap_step(MicUnit &u, uint32_t base, uint32_t hi, uint32_t mode, uint32_t *s_u, int32_t *s_i,
                                         uint32_t &c_used, int32_t &c_last, uint32_t &c_esc) {
    const uint32_t b0 = base + 4u * threadIdx.x;
    uint4 h4 = make_uint4(0u, 0u, 0u, 0u);
    if (b0 < hi) h4 = *(const uint4 *)(u.hist + b0);               // (hi <= tab_cap, a multiple of GAP_CHUNK: the load stays in the slab)
    uint32_t hv[4] = { h4.x, h4.y, h4.z, h4.w };
    uint32_t cnt = 0; int32_t first = -1, last = -1;
    for (int k = 0; k < 4; k++) {
        if (b0 + k >= hi) hv[k] = 0;
        if (hv[k]) { cnt++; if (first < 0) first = (int32_t)(b0 + k); last = (int32_t)(b0 + k); }
    }
    uint32_t used_all; int32_t last_all;
    const uint32_t idx0 = c_used + gap_scan_add(cnt, s_u, &used_all);
    int32_t prev = gap_scan_max(last, s_i, &last_all);
    if (prev < 0) prev = c_last;                                    // (the last value used by an earlier step)
    // within four bins no gap reaches 255: only a thread's first used value can be an escape
    const uint32_t esc = (first >= 0 && prev >= 0 && (uint32_t)(first - prev - 1) >= 255u) ? 1u : 0u;
    uint32_t esc_all;
    uint32_t esc0 = c_esc + gap_scan_add(esc, s_u, &esc_all);
    if (WRITE && cnt) {
        // every thread has read its bins (the scans end on barriers): bins that receive no compact count go to zero, then the counts
        // move down -- index <= value, and the indices written in this step, [c_used, c_used + used_all), are written, not zeroed
        mic_gp<uint32_t> hist = mic_g(u.hist);
        mic_gp<uint16_t> cidx = mic_g((uint16_t *)u.gap_buf);
        mic_gp<uint8_t> map = mic_g(u.gap_buf + mic_gap_map_off(u.tab_cap));
        uint32_t idx = idx0; int32_t p = prev;
        for (int k = 0; k < 4; k++) {
            if (!hv[k]) continue;
            const uint32_t v = b0 + k;
            if (v < c_used || v >= c_used + used_all) hist[v] = 0u;
            hist[idx] = hv[k];
            cidx[v] = (uint16_t)idx;
            if (mode == 1) { map[3 + 2 * idx] = (uint8_t)v; map[4 + 2 * idx] = (uint8_t)(v >> 8); }
            else if (idx == 0) { map[3] = (uint8_t)v; map[4] = (uint8_t)(v >> 8); }
            else {
                const uint32_t g = v - (uint32_t)p - 1u, at = 5u + (idx - 1u) + 2u * esc0;
                if (g >= 255u) { map[at] = 0xFF; map[at + 1] = (uint8_t)g; map[at + 2] = (uint8_t)(g >> 8); esc0++; }
                else map[at] = (uint8_t)g;
            }
            idx++; p = (int32_t)v;
        }
    }
    MIC_GROUP_HANDOFF();                                            // (the next step's zeroes may land where this step wrote counts)
    c_used += used_all; c_esc += esc_all;
    if (last_all >= 0) c_last = last_all;
}

// One work-group per unit, behind the tokeniser, in front of k_enc_tables_wg.  Units without the flag, or whose tokeniser failed,
// are left alone.
__global__ void __launch_bounds__(GAP_THREADS) k_enc_gap(MicUnit *units) {
    MicUnit &u = units[blockIdx.x];
    if (!u.gap || u.status != MICD_OK) return;
    __shared__ uint32_t s_u[GAP_WAVES];
    __shared__ int32_t s_i[GAP_WAVES];
    const uint32_t hi = min(u.tab_cap, (u.hist_hi >= 1 && u.hist_hi <= MIC_MAXSYM) ? u.hist_hi : MIC_MAXSYM + 1u);
    // walk 1: numUsed, maxSym, escapes of the delta map, and which steps hold used values (hi <= 65536: at most 64 steps)
    uint32_t used = 0, esc = 0; int32_t last = -1;
    uint64_t busy = 0;
    for (uint32_t base = 0; base < hi; base += GAP_CHUNK) {
        const uint32_t before = used;
        gap_step<false>(u, base, hi, 0, s_u, s_i, used, last, esc);
        if (used != before) busy |= 1ull << (base / GAP_CHUNK);
    }
    // :81-111, integer arithmetic as there
    const uint32_t max_sym = last < 0 ? 0u : (uint32_t)last, sym_len = max_sym + 1u;
    const uint32_t raw = 3u + 2u * used, bitmap = 3u + (max_sym + 8u) / 8u;
    const uint32_t delta = used == 0 ? 5u : 4u + (used - 1u) + 2u * esc + 1u;
    uint32_t best = raw, mode = 1;
    if (bitmap < best) { best = bitmap; mode = 2; }
    if (delta < best) { best = delta; mode = 3; }
    // A chosen bitmap never passes: bitmap * 8 = 24 + 8 * ((maxSym + 8) / 8) >= symLen + 24 > symLen - numUsed.
    const bool apply = used > 1 && used < sym_len / 2 && best * 8u < sym_len - used && mode != 2;
    mic_gp<uint8_t> map = mic_g(u.gap_buf + mic_gap_map_off(u.tab_cap));
    if (!apply) {
        if (threadIdx.x == 0) { map[0] = 0x00; u.gap_hdr_len = 1; }
        return;
    }
    used = 0; esc = 0; last = -1;
    // walk 2 visits only the steps with used values (a step without any has nothing to zero, move or write)
    for (uint32_t base = 0; base < hi; base += GAP_CHUNK)
        if ((busy >> (base / GAP_CHUNK)) & 1ull) gap_step<true>(u, base, hi, mode, s_u, s_i, used, last, esc);
    if (threadIdx.x == 0) {
        map[0] = (uint8_t)mode; map[1] = (uint8_t)used; map[2] = (uint8_t)(used >> 8);
        u.gap_hdr_len = best; u.hist_hi = used; u.gap = 2;
    }
}

// tokens -> compact indices (a gather from a table of at most 16 / 128 KiB: L2 hits).  grid = (chunks, units)
__global__ void __launch_bounds__(256) k_enc_gap_remap(MicUnit *units) {
    const MicUnit &u = units[blockIdx.y];
    if (u.gap != 2 || u.status != MICD_OK) return;
    mic_gp<uint16_t> tok = mic_g(u.tok);
    const mic_gp<const uint16_t> cidx = mic_g((const uint16_t *)u.gap_buf);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < u.ntok; i += gridDim.x * blockDim.x) tok[i] = cidx[tok[i]];
}

// behind the tANS encoders: the packed stream is mode || map || FSE
__global__ void __launch_bounds__(256) k_enc_gap_len(MicUnit *units, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    MicUnit &u = units[i];
    if (u.gap && u.status == MICD_OK) u.blob_len += u.gap_hdr_len;
}

// One wave per unit, in front of k_dec_parse: :178-256.  The unit is moved past mode || map; a map the reference refuses leaves an
// empty stream and gap = 3 (k_dec_gap_expand turns it into MIC_ERR_CORRUPT: k_dec_parse resets every unit's status).
__global__ void __launch_bounds__(64) k_dec_gap_map(MicUnit *units) {
    MicUnit &u = units[blockIdx.x];
    if (!u.gap || !u.comp_in) return;
    const uint32_t lane = threadIdx.x, len = u.comp_len;
    const uint8_t *c = u.comp_in;
    mic_gp<uint16_t> ex = mic_g((uint16_t *)u.gap_buf);
    const uint32_t cap = u.tab_cap;                                 // (the expand table keeps the map's first tab_cap entries: every
                                                                    //  symbol a table of this tier can hold)
    const uint32_t mode = len ? c[0] : 0xFFFFFFFFu;
    uint32_t hdr = 0, nsym = 0; bool ok = true;
    if (mode == 0x00) hdr = 1;
    else if (mode == 0x01) {
        ok = len >= 3;
        if (ok) { nsym = (uint32_t)c[1] | ((uint32_t)c[2] << 8); hdr = 3 + 2 * nsym; ok = len >= hdr; }
        if (ok) for (uint32_t i = lane; i < min(nsym, cap); i += 64) ex[i] = (uint16_t)((uint32_t)c[3 + 2 * i] | ((uint32_t)c[4 + 2 * i] << 8));
    } else if (mode == 0x02) {
        ok = len >= 3;
        if (ok) {
            const uint32_t max_sym = (uint32_t)c[1] | ((uint32_t)c[2] << 8), nbytes = (max_sym + 8) / 8;
            hdr = 3 + nbytes; ok = len >= hdr;
            if (ok) {
                // each lane a contiguous run of bytes; its first index = the popcounts of the lanes before it
                const uint32_t per = (nbytes + 63) / 64, lo = min(nbytes, lane * per), hi = min(nbytes, lo + per);
                // bits past maxSym in the last byte are not symbols (:228-232 reads sym = 0 .. maxSym)
                auto byte_at = [&](uint32_t b) -> uint32_t {
                    const uint32_t v = c[3 + b];
                    return 8 * b + 7 > max_sym ? v & ((1u << (max_sym - 8 * b + 1)) - 1u) : v;
                };
                uint32_t cnt = 0;
                for (uint32_t b = lo; b < hi; b++) cnt += __popc(byte_at(b));
                const uint32_t x = mic_wave_incl_add(cnt);
                uint32_t idx = x - cnt;
                nsym = __shfl(x, 63, 64);
                for (uint32_t b = lo; b < hi; b++)
                    for (uint32_t bits = byte_at(b); bits; bits &= bits - 1, idx++)
                        if (idx < cap) ex[idx] = (uint16_t)(8 * b + (uint32_t)__ffs(bits) - 1);
            }
        }
    } else if (mode == 0x03) {
        ok = len >= 5;
        if (ok) {
            nsym = (uint32_t)c[1] | ((uint32_t)c[2] << 8);
            hdr = 5;
            // the entries have variable length: one lane walks them (maps are short next to the stream); u16 arithmetic wraps as in Go
            // (staging the map in LDS first was measured: 0.34 against 0.36 ms for 256 CT maps, noise -- the walk's dependent steps dominate)
            auto at = [&](uint32_t q) -> uint32_t { return (uint32_t)c[q]; };
            if (lane == 0 && nsym) {
                uint16_t e = (uint16_t)(at(3) | (at(4) << 8));
                if (cap) ex[0] = e;
                uint32_t p = 5;
                for (uint32_t i = 1; i < nsym; i++) {
                    if (p >= len) { ok = false; break; }
                    const uint32_t b = at(p++);
                    uint32_t g = b;
                    if (b == 0xFF) {
                        if (p + 2 > len) { ok = false; break; }
                        g = at(p) | (at(p + 1) << 8);
                        p += 2;
                    }
                    e = (uint16_t)(e + g + 1u);
                    if (i < cap) ex[i] = e;
                }
                hdr = p;
            }
            ok = __shfl((int)ok, 0, 64) != 0;
            hdr = __shfl(hdr, 0, 64);
        }
    } else ok = false;
    if (lane == 0) {
        if (!ok) { u.gap = 3; u.comp_len = 0; return; }
        u.comp_in = c + hdr; u.comp_len = len - hdr; u.gap_hdr_len = hdr; u.gap_nsym = nsym;
        u.gap = mode == 0x00 ? 1u : 2u;
    }
}

// Behind k_dec_tables_wg: tab_sym[state] = expandMap[tab_sym[state]].  A table that gives weight to a compact symbol >= numSymbols
// (no encoder writes one -- FSE weights exactly the symbols that occur -- but a stream may) is left compact and parked in
// MICD_GAP_CHECK: no decoder but k_dec_gap_check (mic_decode.hip) takes it, which fails it only if such a symbol is emitted.
__global__ void __launch_bounds__(256) k_dec_gap_expand(MicUnit *units) {
    MicUnit &u = units[blockIdx.x];
    if (u.gap == 3) { if (threadIdx.x == 0) u.status = MICD_ERR_CORRUPT; return; }
    if (u.gap != 2 || u.status != MICD_OK) return;
    const uint32_t states = 1u << u.table_log, lim = min(u.gap_nsym, u.tab_cap);   // (symbols of a table are < tab_cap)
    mic_gp<uint16_t> ts = mic_g(u.tab_sym);
    const mic_gp<const uint16_t> ex = mic_g((const uint16_t *)u.gap_buf);
    int bad = 0;
    for (uint32_t s = threadIdx.x; s < states; s += 256) bad |= ts[s] >= lim;
    if (__syncthreads_or(bad)) { if (threadIdx.x == 0) u.status = MICD_GAP_CHECK; return; }
    for (uint32_t s = threadIdx.x; s < states; s += 256) ts[s] = ex[ts[s]];
}

void mic_launch_enc_gap(MicUnit *d_units, int n, hipStream_t stream, MicTimer *t) {
    if (t) t->mark("k_enc_gap");
    hipLaunchKernelGGL(k_enc_gap, dim3(n), dim3(GAP_THREADS), 0, stream, d_units);
}
void mic_launch_enc_gap_remap(MicUnit *d_units, int n, hipStream_t stream, MicTimer *t) {
    if (t) t->mark("k_enc_gap_remap");
    hipLaunchKernelGGL(k_enc_gap_remap, dim3(32, n), dim3(256), 0, stream, d_units);
}
void mic_launch_enc_gap_len(MicUnit *d_units, int n, hipStream_t stream) {
    hipLaunchKernelGGL(k_enc_gap_len, dim3((n + 255) / 256), dim3(256), 0, stream, d_units, n);
}
void mic_launch_dec_gap_map(MicUnit *d_units, int n, hipStream_t stream, MicTimer *t) {
    if (t) t->mark("k_dec_gap_map");
    hipLaunchKernelGGL(k_dec_gap_map, dim3(n), dim3(64), 0, stream, d_units);
}
void mic_launch_dec_gap_expand(MicUnit *d_units, int n, hipStream_t stream, MicTimer *t) {
    if (t) t->mark("k_dec_gap_expand");
    hipLaunchKernelGGL(k_dec_gap_expand, dim3(n), dim3(256), 0, stream, d_units);
}
