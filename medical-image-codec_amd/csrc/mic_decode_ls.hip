// mic_decode_ls.hip -- tANS decode with one LANE per (stream, state): nine streams per CU.
//
// The N states of an N-state stream (fse2state.go:203-308, fse4state.go:195-353, fse8state.go:230-380,
// rans8state.go:221-412) share one reverse bitstream, so a stream is a serial chain
//   state_k -> table entry -> (nbBits, nextState) -> bits at the running position -> state_k'
// and decode throughput = resident streams / latency of one round of N symbols.  Two things bound it on a
// CU: the LDS holds the 16-bit nextState tables of at most NINE streams (tableLog 13: 16 KiB each), and a wave issues one
// instruction per ~5 cycles whatever its lanes do.  The retired k_dec_tans_duo ran every lane of a
// wave through the same values -- two distinct streams per 64 lanes, N table look-ups issued one after the other -- so it
// was bound by instructions issued per symbol and got slower with more states.  Here lane g*N + k of a wave owns state k of
// the wave's stream g (three streams per wave, three waves per group, one group per CU; N = 4: lane 16 g + k, a DPP row a stream):
//   * a round = ONE table look-up instruction for all N states of all three streams, nbBits from v_ffbh, the offset of a
//     state's bits inside the round from a DPP prefix sum over the N lanes of its stream (quad_perm / row_shr: no LDS, no
//     readlane), the bits from a funnel shift of the stream's bit window, kept in a 256-dword LDS ring;
//   * N = 4: the round's 64-bit window is read at the round's start position together with the table look-ups, so a round costs
//     one LDS round trip (136 cycles for four symbols); N = 2: the 32-bit window is picked from three ring dwords read a round
//     EARLIER, so nothing but the look-up's own wait stands in the round (108 cycles for two symbols); N = 8: every lane reads its own window at
//     its own bit position once the prefix sum is known: two round trips for eight symbols.  More states decode FASTER;
//   * the lanes of a wave that own no state clone stream 0 (same addresses: LDS broadcasts); all 64 lanes share the
//     per-chunk work, which is small: ring refill (64 dwords per stream and 128 symbols, prefetched a chunk ahead) and one
//     coalesced 256-byte store of the chunk's 128 STATES per stream.
// The states are turned into symbols by k_dec_translate (below), not here: a symbol look-up is a 2-byte gather from a 16 KiB
// table per stream -- 9 tables x 32 CUs overflow an XCD's 4 MiB L2, every wave-instruction touches 64 cache lines, and with
// the gathers inside this kernel the chain waves spent 30 % of their time queueing on the CU's miss path (3200 of 11 000
// cycles per chunk; stamps: tools/time_dec.py on an LS_STAMP build).  k_dec_translate has the table in LDS, streams the
// states once, and walks the RLE headers (rledecompressu16.go:59-85) on tiles it already holds in LDS.
// Streams come from a compacted per-class list (k_dec_classify), so a launch only touches the units of its class.
// LDS per stream: ring 1024 B (2048 at tableLog 16) | 2 mirror dwords + pad, 16 B | stage 256 B (128 u16 states) | table 2 << tableLog B.
#include <type_traits>
#include "mic_dev.h"
#include "mic_launch.h"
#include "mic_wave.h"
#include "mic_rlewalk.h"

// Table-size classes: streams per wave x waves per group are what the LDS holds of 2 << tableLog byte tables.
//   tableLog 13: 3 x 3 = nine streams (159 120 bytes) | 14: 2 x 2 (136 256) | 15: 1 x 2 (134 736) | 16: 1 x 1 (133 392)
//   tableLog <= 12 (8 KiB tables: small units -- MIC3 planes, thin strips): 4 x 4 = sixteen streams (151 808)
// At tableLog 16 a nextState needs 17 bits when the table has 0-bit entries (zeroBits): those streams stay with k_dec_tans_gl.
#define LS_RING 0u
#define LS_CLASSES MIC_CLS_CLASSES                 // 5 table-size classes (tableLog 13, 14, 15, 16, <= 12) x (N in 2,4,8) x (zeroBits)
template <int TL> struct LsGeom {
    static constexpr int SPW = TL <= 12 ? 4 : TL == 13 ? 3 : TL == 14 ? 2 : 1;   // streams per wave
    static constexpr int WAVES = TL <= 12 ? 4 : TL == 13 ? 3 : TL == 16 ? 1 : 2;  // waves per group (one group per CU: the LDS is full)
    // The bit window's ring: blocks of 64 dwords.  A chunk of 128 symbols takes at most 4 * tableLog dwords off it (+ 2 the window
    // reads reach below the position): under a block up to tableLog 15, so three blocks stored (the position's, one above, one below)
    // and a fourth in flight do; at tableLog 16 a chunk can take a whole block, so the ring is twice as long and runs a block deeper.
    // The reads that reach furthest are those of N = 2 and N = 4, three dwords from the dword of p - 32 on for every position p of a
    // chunk, its last included: with D the dword of the chunk's first position, in block b, they span dwords D - 4 * tableLog - 1
    // ... D + 1.  tableLog 15: D - 61 >= 64 b - 61 = 64 (b - 1) + 3, inside block b - 1, and D + 1 inside b + 1 at the most: the
    // three stored blocks.  tableLog 16: D - 65 >= 64 (b - 2) + 63, inside block b - 2, the fourth of the four stored there (DEPTH 3).
    // The block stored at a chunk's end takes the slot of block b + 2 (b + 5), which no chunk from here on reads.
    static constexpr int RING_BLOCKS = TL == 16 ? 8 : 4;
    static constexpr int DEPTH = TL == 16 ? 3 : 2;                        // the block in flight is the position's block - DEPTH
    static constexpr int RING_BITS = TL == 16 ? 9 : 8;                    // dword index bits
    static constexpr uint32_t MIRROR = 256u * RING_BLOCKS;                // two mirror dwords (slots 0, 1) + two pad dwords
    static constexpr uint32_t STAGE = MIRROR + 16u;                       // 128 u16 states of a chunk
    static constexpr uint32_t TAB = STAGE + 256u;
    static constexpr uint32_t STREAM_BYTES = TAB + (2u << TL);
    static constexpr uint32_t LDS = WAVES * SPW * STREAM_BYTES;
    static_assert(LDS <= 160 * 1024, "one group must fit a CU's LDS");
};
#define LS_TL 13                                   // the nine-streams class

typedef __attribute__((address_space(3))) uint32_t *ls_l32;
typedef __attribute__((address_space(3))) uint16_t *ls_l16;
typedef const __attribute__((address_space(1))) uint16_t *ls_gcu16;
typedef const __attribute__((address_space(1))) uint32_t *ls_gcu32;
typedef __attribute__((address_space(1))) uint16_t *ls_gu16;
typedef __attribute__((address_space(1))) uint32_t *ls_gu32;
typedef uint32_t ls_v2 __attribute__((ext_vector_type(2)));

template <int CTRL> __device__ __forceinline__ uint32_t ls_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
#define LS_QP(a, b, c, d) ((a) | ((b) << 2) | ((c) << 4) | ((d) << 6))
#define LS_ROW_SHR(n) (0x110 + (n))
#define LS_ROW_HALF_MIRROR 0x141

__device__ __forceinline__ uint32_t ls_rl(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ uint64_t ls_rl64(uint64_t v, int lane) {
    return ((uint64_t)ls_rl((uint32_t)(v >> 32), lane) << 32) | ls_rl((uint32_t)v, lane);
}

// Per-class lists of unit indices, in unit order: list[c * n + i], count[c].  Class = 2 * log2(N / 2) + zeroBits for the
// N-state streams (rANS-8 decodes as 8-state), + 6 per table-size class (tableLog <= 13, 14, 15, 16); 1-state streams, very long
// streams and tableLog-16 tables with 0-bit entries are left to the kernels of mic_decode.hip.
// One group; the stream checks that need the blob (empty bitstream, zero end byte: bitreader.go:33-38) are made here.
// List LS_SPLIT_LIST holds the units of class 0 (two states, tableLog 13, no 0-bit entries) that k_dec_tans_ls_parts<2> takes when
// `split` is set (the launcher's: that kernel is launched) -- whole streams of at least min_tokens tokens and min_bits16 / 16 bits
// per token; list LS_RETRY_LIST is filled by that kernel with what it hands back, its count starts at zero here.
// List LS_SPLIT4_LIST holds those of them that have at least min_tokens4 tokens: k_dec_tans_ls_parts<4> takes them, and hands back
// to the same retry list.
// List LS_SPLIT8_LIST holds those of at least max(min_tokens8, min_tokens4) tokens: k_dec_tans_ls_parts<8> takes them, and appends
// what it hands back to the four-part list, which the four-part instance, launched behind it, judges afresh.
#define LS_SPLIT_LIST MIC_CLS_CLASSES
#define LS_RETRY_LIST (MIC_CLS_CLASSES + 1)
#define LS_SPLIT4_LIST (MIC_CLS_CLASSES + 2)
#define LS_SPLIT8_LIST (MIC_CLS_CLASSES + 3)
#define LS_LISTS MIC_CLS_LISTS                     // lists this kernel counts (the retry list takes no unit here)
__global__ void __launch_bounds__(1024) k_dec_classify(MicUnit *units, int n, int *list, int *count, int split, MicSplitCfg cfg) {
    __shared__ uint32_t s_w[16][LS_LISTS];
    __shared__ uint32_t s_base[LS_LISTS];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < LS_LISTS) s_base[tid] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + (int)tid;
        int cls = -1;
        if (i < n) {
            MicUnit &u = units[i];
            const uint32_t flav = u.flavour, tl = u.table_log;
            const uint32_t ns = (flav == 108) ? 8u : flav;
            if (u.status == MICD_OK && u.ntok == 0 && (ns == 2 || ns == 4 || ns == 8) && tl >= MIC_MIN_TABLELOG && tl <= MIC_MAX_TABLELOG &&
                !(tl == 16 && u.zero_bits)) {                               // (17-bit nextState: k_dec_tans_gl)
                if (u.bits_off >= u.comp_len) u.status = MICD_ERR_CORRUPT;
                else if (u.comp_len - u.bits_off < (1u << 27)) {            // 32-bit bit positions here; the serial kernel takes longer ones
                    if (u.comp_in[u.comp_len - 1] == 0) u.status = MICD_ERR_CORRUPT;
                    else {
                        cls = mic_dec_cls(flav, tl, u.zero_bits);
                        if (cls == 0 && split && mic_split_gate(u, cfg))
                            cls = u.count >= max(cfg.min_tokens8, cfg.min_tokens4) ? LS_SPLIT8_LIST : u.count >= cfg.min_tokens4 ? LS_SPLIT4_LIST : LS_SPLIT_LIST;
                    }
                }
            }
        }
        uint32_t rank = 0;
#pragma unroll
        for (int c = 0; c < LS_LISTS; c++) {
            const uint64_t m = __ballot(cls == c);
            if (cls == c) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) s_w[wave][c] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        if (cls >= 0) {
            uint32_t off = s_base[cls];
            for (uint32_t w = 0; w < wave; w++) off += s_w[w][cls];
            list[(size_t)cls * (size_t)n + off + rank] = i;
        }
        __syncthreads();
        if (tid < LS_LISTS) { uint32_t t = 0; for (int w = 0; w < 16; w++) t += s_w[w][tid]; s_base[tid] += t; }
        __syncthreads();
    }
    if (tid < LS_LISTS) count[tid] = (int)s_base[tid];
    if (tid == LS_RETRY_LIST) count[tid] = 0;
}

template <int N, bool ZB, int TL>
__global__ void __launch_bounds__(64 * LsGeom<TL>::WAVES) k_dec_tans_ls(MicUnit *units, const int *list, const int *count_p) {
    constexpr int LS_SPW = LsGeom<TL>::SPW, LS_WAVES = LsGeom<TL>::WAVES;
    constexpr uint32_t LS_STREAM_BYTES = LsGeom<TL>::STREAM_BYTES, LS_STAGE = LsGeom<TL>::STAGE, LS_TAB = LsGeom<TL>::TAB, LS_MIRROR = LsGeom<TL>::MIRROR;
    constexpr int LS_RB = LsGeom<TL>::RING_BLOCKS, LS_DEPTH = LsGeom<TL>::DEPTH, LS_RBITS = LsGeom<TL>::RING_BITS;
    extern __shared__ uint32_t s_mem[];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)s_mem != 0u) return;   // layout assumes dynamic LDS at 0
    const int n_cls = *count_p;
    const int slot0 = __builtin_amdgcn_readfirstlane(((int)blockIdx.x * LS_WAVES + (int)wv) * LS_SPW);   // (wave-uniform, provably so: descriptors below)
    if (slot0 >= n_cls) return;                                             // waves share nothing and never meet at a barrier
    // ---- roles ----------------------------------------------------------------------------------------------------
    // N = 4 gives every stream a DPP row of 16 lanes (states in lanes 0-3, the other twelve are clones that sit out the chunks):
    // row_shr then stops at the stream's first lane by itself, and the prefix sum of a round is two instructions
    constexpr int LS_LS = N == 4 ? 16 : N;                                  // lanes from one stream to the next
    const uint32_t k = (lane % LS_LS) % N;                                  // state of the chain this lane runs
    const bool real = lane % LS_LS < N && lane < LS_SPW * LS_LS;            // (not a clone inside a stream's row, nor a surplus lane)
    uint32_t g = lane / LS_LS; if (g >= LS_SPW) g = 0;                      // its stream; surplus lanes clone stream 0
    const bool have = slot0 + (int)g < n_cls;                               // the last wave of a class may hold fewer streams
    const uint32_t gs = have ? g : 0;                                       // absent streams run on stream 0's table (every access in range)
    const MicUnit &u = units[list[slot0 + (int)gs]];
    const uint32_t tl = u.table_log, size = 1u << tl;
    const uint32_t count = have ? mic_sym_ceiling(u, u.count) : 0u;          // (a ceiling is a multiple of 128: no tail behind it)
    const uint32_t bits_off = u.bits_off, len = u.comp_len - bits_off;
    const uint32_t sbase = (wv * LS_SPW + g) * LS_STREAM_BYTES;             // own ring / stage (also for an absent stream)
    const uint32_t tbase = (wv * LS_SPW + gs) * LS_STREAM_BYTES + LS_TAB;
    // ---- tables: u16 nextState = (newState + size) >> nbBits (fsedecompressu16.go:233-241), all 64 lanes per stream ----
#pragma unroll 1
    for (int j = 0; j < LS_SPW; j++) {
        if (slot0 + j >= n_cls) break;
        const int src = j * LS_LS;                                          // a lane that holds stream j's values
        const uint32_t sz = ls_rl(size, src);
        const uint32_t *dt = (const uint32_t *)(uintptr_t)ls_rl64((uint64_t)(uintptr_t)u.tt_nb, src);
        const uint32_t tb = (wv * LS_SPW + (uint32_t)j) * LS_STREAM_BYTES + LS_TAB;
        for (uint32_t p = lane * 4; p < sz; p += 256) {
            const uint4 e = *(const uint4 *)(dt + p);
            const uint32_t n0 = ((e.x & 0xFFFF) + sz) >> (e.x >> 16), n1 = ((e.y & 0xFFFF) + sz) >> (e.y >> 16);
            const uint32_t n2 = ((e.z & 0xFFFF) + sz) >> (e.z >> 16), n3 = ((e.w & 0xFFFF) + sz) >> (e.w >> 16);
            ls_v2 v; v.x = n0 | (n1 << 16); v.y = n2 | (n3 << 16);
            *(__attribute__((address_space(3))) ls_v2 *)(uintptr_t)(tb + p * 2) = v;
        }
    }
    // ---- bit reader (bitreader.go): grid of aligned dwords under the stream; unread bits = grid bits [8*sb, cur) ----
    const uint8_t *bs = u.comp_in + bits_off;
    const uint32_t last = bs[len - 1];                                      // non-zero: k_dec_classify
    const uintptr_t addr = (uintptr_t)bs;
    const uint32_t sb = (uint32_t)(addr & 3);
    const uint64_t gaddr = (uint64_t)(addr - sb);
    const int32_t cur0 = (int32_t)(8u * (len - 1) + (uint32_t)(31 - __clz(last)) + 8u * sb);
    const int32_t top_dw = have ? (cur0 - 1) >> 5 : -1;
    int32_t q = cur0 - 32;                                                  // window of a round = grid bits [q, q+32): its MSB is the next unread bit
    // wave-uniform per-stream values for the shared work.  The compressed stream and the output go through buffer descriptors:
    // a block of the stream that lies (partly) outside it reads as zeros and a store behind a stream's last whole chunk is
    // dropped by the range check, so the per-chunk upkeep below has no branch at all (a taken scalar branch costs a wave
    // 30-45 cycles, and the compiler-predicated form of this upkeep had fifteen of them: 1700 cycles per chunk, stamped).
    bool s_have[LS_SPW]; uint64_t s_out[LS_SPW]; int32_t s_blk[LS_SPW], s_pfb[LS_SPW]; uint32_t s_chunks[LS_SPW];
    __amdgpu_buffer_rsrc_t rs_in[LS_SPW], rs_out[LS_SPW];
#pragma unroll
    for (int j = 0; j < LS_SPW; j++) {
        const int src = j * LS_LS;
        s_have[j] = slot0 + j < n_cls;
        s_out[j] = ls_rl64((uint64_t)(uintptr_t)u.tok, src);
        s_chunks[j] = ls_rl(count, src) / 128u;
        s_blk[j] = ((int32_t)ls_rl((uint32_t)(q - (int32_t)(N * tl)), src) >> 5) >> 6;   // block of the position BEHIND the initial states (N * tableLog
                                                                            // bits at most: a chunk then never moves the position by more than one block)
        const uint32_t in_bytes = (uint32_t)__builtin_amdgcn_readfirstlane((int)(s_have[j] ? ((uint32_t)((int32_t)ls_rl((uint32_t)top_dw, src) + 1)) * 4u : 0u));
        const uint32_t out_bytes = (uint32_t)__builtin_amdgcn_readfirstlane((int)(s_have[j] ? s_chunks[j] * 256u : 0u));
        rs_in[j] = __builtin_amdgcn_make_buffer_rsrc((void *)(uintptr_t)ls_rl64(gaddr, src), 0, (int)in_bytes, 0x00020000);
        rs_out[j] = __builtin_amdgcn_make_buffer_rsrc((void *)(uintptr_t)s_out[j], 0, (int)out_bytes, 0x00020000);
    }
    auto load_blk = [&](int j, int32_t b) -> uint32_t {                    // dword `lane` of block b of stream j, zero outside the stream
        return __builtin_amdgcn_raw_buffer_load_b32(rs_in[j], (b * 64 + (int32_t)lane) * 4, 0, 2);   // (a negative offset is out of range too); nt: streamed once
    };
    auto store_blk = [&](int j, int32_t b, uint32_t v) {
        const uint32_t rb = (wv * LS_SPW + (uint32_t)j) * LS_STREAM_BYTES + LS_RING;
        const uint32_t slot = (uint32_t)b & (uint32_t)(LS_RB - 1);
        *(ls_l32)(uintptr_t)(rb + (slot * 64u + lane) * 4) = v;
        // mirror: a read of two or three dwords from the ring's last slots stays linear.  Lanes 0 and 1 write it when the block is
        // the ring's first, the pad dwords behind it otherwise (an address select, not a branch)
        if (lane < 2) *(ls_l32)(uintptr_t)(rb + LS_MIRROR + lane * 4 + (slot == 0u ? 0u : 8u)) = v;
    };
    uint32_t pf[LS_SPW];
#pragma unroll
    for (int j = 0; j < LS_SPW; j++) {
#pragma unroll
        for (int dd = -1; dd < LS_DEPTH; dd++) store_blk(j, s_blk[j] - dd, load_blk(j, s_blk[j] - dd));
        s_pfb[j] = s_blk[j] - LS_DEPTH;
        pf[j] = load_blk(j, s_pfb[j]);                                      // enters the ring at the end of the first chunk
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);                                     // wave-private LDS: the writes above are in before the reads below
    // ---- chain state ---------------------------------------------------------------------------------------------
    const uint32_t ringb = sbase + LS_RING;
    const uint32_t stgb = sbase + LS_STAGE + 2u * k;                        // stage16[r * N + k] = state k of round r
    const uint32_t cb = tbase - 2u * size;                                  // byte address of entry s = 2 * s + cb, s in [size, 2 * size)
    const uint32_t C = 31u - tl;
    auto window = [&](int32_t qq) -> uint32_t {
        const uint32_t a = (__builtin_amdgcn_ubfe((uint32_t)qq, 5, LS_RBITS) << 2) + ringb;
        const uint32_t w0 = *(ls_l32)(uintptr_t)a, w1 = *(ls_l32)(uintptr_t)(a + 4);
        return __builtin_amdgcn_alignbit(w1, w0, (uint32_t)qq);
    };
    auto entry = [&](uint32_t s) -> uint32_t { return *(ls_l16)(uintptr_t)(s * 2 + cb); };
    // initial states: state 0 first, tableLog bits each (fse2state.go:210-212); kept with the +size offset
    uint32_t st = size + (window(q - (int32_t)(k * tl)) >> (32u - tl));
    q -= (int32_t)(N * tl);
    const uint32_t kq = k & 3u;                                             // position inside the quad (N = 8: a stream spans two quads)
    const uint32_t mk1 = (kq >= 1) ? ~0u : 0u, mk2 = (kq >= 2) ? ~0u : 0u, mk4 = (k >= 4) ? ~0u : 0u;
    // bits of a round: nb = this state's nbBits, pre = bits the earlier states of the round take, ntot = MINUS the round's bits.
    // Minus, because `q - dpp(x)` must not reach the compiler: it folds the lane permutation into a v_subrev_u32_dpp, and on this
    // toolchain (ROCm 7.2, gfx950) that instruction computes dpp(src1) - src0 instead of src1 - dpp(src0) -- measured with
    // tools/dpp_subrev_repro.hip, v_sub_u32_dpp and v_add_u32_dpp are as documented -- so the sum is negated before it is permuted
    // and then ADDED to the bit position.
    auto prefix = [&](uint32_t nb, uint32_t &pre, uint32_t &ntot) {
        if (N == 2) {
            pre = ls_dpp<LS_QP(0, 0, 2, 2)>(nb) & mk1;
            ntot = 0u - (nb + ls_dpp<LS_QP(1, 0, 3, 2)>(nb));
        } else {
            uint32_t t = nb + (ls_dpp<LS_QP(0, 0, 1, 2)>(nb) & mk1);
            t = t + (ls_dpp<LS_QP(0, 0, 0, 1)>(t) & mk2);                    // inclusive prefix inside the quad
            const uint32_t ntq = ls_dpp<LS_QP(3, 3, 3, 3)>(0u - t);         // minus the quad's sum
            if (N == 4) { pre = t - nb; ntot = ntq; }
            else {
                t = t + ((0u - ls_dpp<LS_ROW_SHR(4)>(ntq)) & mk4);
                pre = t - nb;
                ntot = ntq + ls_dpp<LS_ROW_HALF_MIRROR>(ntq);
            }
        }
    };
    // one round = N symbols of every stream of the wave; stage slot at byte offset soff from stgb
    auto round = [&](uint32_t soff) {
        const uint32_t e = entry(st);
        if (N == 2) {
            const uint32_t hi = window(q);
            *(ls_l16)(uintptr_t)(stgb + soff) = (uint16_t)st;
            const uint32_t c = (uint32_t)__builtin_clz(e);
            const uint32_t nb = c - C, m = C - c;                           // m = -nbBits: a funnel shift right by m mod 32 = 32 - nbBits
            uint32_t pre, ntot; prefix(nb, pre, ntot);
            const uint32_t hi1 = hi << pre;
            if (ZB) st = (uint32_t)((((uint64_t)e << 32) | hi1) >> (32u - nb));   // nbBits may be 0: a 64-bit shift by 32 is well defined
            else st = __builtin_amdgcn_alignbit(e, hi1, m);
            q += (int32_t)ntot;
        } else {
            *(ls_l16)(uintptr_t)(stgb + soff) = (uint16_t)st;
            const uint32_t c = (uint32_t)__builtin_clz(e);
            const uint32_t nb = c - C, m = C - c;
            uint32_t pre, ntot; prefix(nb, pre, ntot);
            const uint32_t hi = window(q - (int32_t)pre);                   // this state's own window
            if (ZB) st = (uint32_t)((((uint64_t)e << 32) | hi) >> (32u - nb));
            else st = __builtin_amdgcn_alignbit(e, hi, m);
            q += (int32_t)ntot;
        }
    };
    // N = 2: the 64 rounds of a chunk as ONE hand-scheduled instruction stream.  A lone wave issues in order, one instruction per
    // ~4.3-6 cycles whether it depends on its predecessor or not (tools/ubench_ls.hip), and a round is the table look-up's LDS trip
    // (~64 cycles) plus every issue slot between the entry's arrival and the next look-up.  Seven sit there (ZB: nine):
    //   head  s_waitcnt (entry) | v_ffbh_u32_dpp: the PARTNER's leading zeros, from its entry (fresh from LDS, so the DPP read has no
    //         VALU-write hazard to pad) | v_ffbh | v_mad_i32_i24: the second state's offset C - c' = minus the first state's nbBits,
    //         0 * c' + 0 for the first state | v_sub: m = -nbBits | v_alignbit(window, window, offset): a ROTATE, so the first state
    //         (shift 0) keeps the window and the second sees it past the first one's bits (what wraps into the low bits is never
    //         read: the two states take <= 32 bits together) | v_alignbit(entry, window', m): the next state (ZB: + compare and
    //         select, m = 0 keeps the entry) | v_lshl_add: its table address | ds_read_u16
    //   tail  ds_write_b16: the state the NEXT round starts from, to the stage (the chunk's first by the prologue) | v_add_dpp: minus
    //         the round's bits | v_add: bit position | v_bfe + v_lshl_add: ring address | the next round's window (below) | ds_read2_b32
    //         + ds_read_b32: three ring dwords at the new position -- behind the look-up, in the shadow of its latency.
    // The window is NOT read at the round's position and waited for in the head (that was 115 cycles per round: the read could
    // leave only ~20 cycles behind the look-up and the head waited for it).  It is picked, in the tail, from the three dwords the
    // tail of the round BEFORE read at ITS position p: the chunk tracks q - 32, so they are the dwords of q - 32, q, q + 32 there and
    // hold grid bits [p - 32, p + 32) at least; two states take <= 2 * tableLog <= 32 bits, so the new position p' is in [p - 32, p]
    // and its window [p', p' + 32) is inside them: v_alignbit of the upper pair when the ring address of p' - 32 is still that of
    // p - 32, of the lower pair when it is the one below (they differ by one dword at most; a 0-bit round keeps the address) -- a
    // compare of the two addresses, two v_cndmask, one v_alignbit with the same shift operand (it uses the low five bits).  The
    // selects read the old dwords before the new read is issued, so one register set does; the two ring addresses alternate
    // between two registers: the .rept body is a double round.  108 cycles per round against 116 for the earlier order
    // (profiles/ubench_ls_early_window.txt; either change alone gains nothing: the early window with v_and_dpp of m and its two
    // pad slots 115-117, v_ffbh_dpp with the window read in the head 118-120).
    // Ring reach: dwords (p - 32) >> 5 ... + 2 for every position p of the chunk, its last included -- one dword below the
    // position's and one above, exactly what N = 4 reads (LsGeom); the two mirror dwords keep three dwords from slot 255 linear.
    // LDS queue, oldest first, at the entry's wait: entry, stage, dwords (2) -> lgkmcnt(3); at the tail's wait for the dwords of
    // the round before: dwords (2), entry, stage -> lgkmcnt(2).  The chunk's last round neither looks up nor reads: the next
    // chunk's prologue does both again, no window state crosses the statement.  v60-v62 take the three dwords (a 64-bit asm
    // operand cannot be split into its halves, fixed registers can).
#define LS2_LOOKUP \
        "v_lshl_add_u32 %[at], %[st], 1, %[cb]\n\t" \
        "ds_read_u16 %[e], %[at]\n\t"
#define LS2_DWORDS(A_) \
        "ds_read2_b32 v[60:61], " A_ " offset1:1\n\t" \
        "ds_read_b32 v62, " A_ " offset:8\n\t"
    // AN_ / AO_: the registers of the new and of the previous ring address
#define LS2_ROUND(AN_, AO_) \
        "s_waitcnt lgkmcnt(3)\n\t" \
        "v_ffbh_u32_dpp %[cp], %[e] quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_ffbh_u32 %[c], %[e]\n\t" \
        "v_mad_i32_i24 %[pre], %[cp], %[mk1], %[Ck]\n\t" \
        "v_sub_u32 %[m], %[C], %[c]\n\t" \
        "v_alignbit_b32 %[hi], %[hi], %[hi], %[pre]\n\t" \
        ".if %[ZBF]\n\t" \
        "v_alignbit_b32 %[hi], %[e], %[hi], %[m]\n\t" \
        "v_cmp_eq_u32 vcc, 0, %[m]\n\t" \
        "v_cndmask_b32 %[st], %[hi], %[e], vcc\n\t" \
        ".else\n\t" \
        "v_alignbit_b32 %[st], %[e], %[hi], %[m]\n\t" \
        ".endif\n\t" \
        ".if ls_off < ls_lim\n\t" \
        LS2_LOOKUP \
        "ds_write_b16 %[stg], %[st] offset:ls_off\n\t" \
        ".endif\n\t" \
        "v_add_u32_dpp %[pre], %[m], %[m] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
        "v_add_u32 %[q], %[q], %[pre]\n\t" \
        ".if ls_off < ls_lim\n\t" \
        "v_bfe_u32 " AN_ ", %[q], 5, %[RW]\n\t" \
        "v_lshl_add_u32 " AN_ ", " AN_ ", 2, %[ringb]\n\t" \
        "v_cmp_eq_u32 vcc, " AN_ ", " AO_ "\n\t" \
        "s_waitcnt lgkmcnt(2)\n\t" \
        "v_cndmask_b32 %[lo], v60, v61, vcc\n\t" \
        "v_cndmask_b32 %[hh], v61, v62, vcc\n\t" \
        "v_alignbit_b32 %[hi], %[hh], %[lo], %[q]\n\t" \
        LS2_DWORDS(AN_) \
        ".endif\n\t" \
        ".set ls_off, ls_off+4\n\t"
    // a whole chunk: 64 rounds.  The prologue looks up, stages the first state, reads the three dwords at the chunk's first position
    // and takes round 0's window from their upper pair; round 0's tail takes round 1's from the same three.
    // (a macro, not a lambda: clang does not capture through asm operands in a generic lambda)
    // DR_ double rounds, LIM_ = 4 * rounds: the stage offset behind which a round neither looks up nor reads (the split instances'
    // chunks are 32 and 16 rounds: LS_CHUNK2_N("16", "128"), LS_CHUNK2_N("8", "64"))
    // STG_: the stage of the chunk's states (the eight-part instance names one of two by the chunk's parity)
#define LS_CHUNK2() LS_CHUNK2_N("32", "256")
#define LS_CHUNK2_N(DR_, LIM_) LS_CHUNK2_AT(DR_, LIM_, stgb)
#define LS_CHUNK2_AT(DR_, LIM_, STG_) do { \
        uint32_t e, c, cp, m, hi, pre, at, a0, a1, lo, hh; \
        q -= 32; \
        asm volatile(".set ls_off, 4\n\t" \
                     ".set ls_lim, " LIM_ "\n\t" \
                     LS2_LOOKUP \
                     "ds_write_b16 %[stg], %[st]\n\t" \
                     "v_bfe_u32 %[a1], %[q], 5, %[RW]\n\t" \
                     "v_lshl_add_u32 %[a1], %[a1], 2, %[ringb]\n\t" \
                     LS2_DWORDS("%[a1]") \
                     "s_waitcnt lgkmcnt(0)\n\t" \
                     "v_alignbit_b32 %[hi], v62, v61, %[q]\n\t" \
                     ".rept " DR_ "\n\t" \
                     LS2_ROUND("%[a0]", "%[a1]") \
                     LS2_ROUND("%[a1]", "%[a0]") \
                     ".endr\n\t" \
                     "s_waitcnt lgkmcnt(0)" \
                     : [st] "+v"(st), [q] "+v"(q), [e] "=&v"(e), [c] "=&v"(c), [cp] "=&v"(cp), [m] "=&v"(m), [hi] "=&v"(hi), [pre] "=&v"(pre), \
                       [at] "=&v"(at), [a0] "=&v"(a0), [a1] "=&v"(a1), [lo] "=&v"(lo), [hh] "=&v"(hh) \
                     : [C] "v"(C), [mk1] "v"(mk1), [Ck] "v"(mk1 & C), [cb] "v"(cb), [ringb] "v"(ringb), [stg] "v"(STG_), [RW] "n"(LS_RBITS), \
                       [ZBF] "n"(ZB ? 1 : 0) \
                     : "memory", "vcc", "v60", "v61", "v62"); \
        q += 32; \
    } while (0)
    // N = 4: one LDS round trip per round as well (tools/ubench_ls.hip, k_cand4: 136 cycles per round of four symbols; with every
    // lane reading its own window behind the prefix sum -- two round trips -- it was 200).  The round's 64-bit window is read at
    // its start position with the table look-ups: three ring dwords from the dword of q - 32 on (q is moved down by 32 for the
    // chunk: the window's low half then starts at the tracked position) -> lo = bits [q-32, q), hi = bits [q, q+32) by two funnel
    // shifts; a state's bits are the top nbBits of (hi:lo) << pre, pre = the bits of the states in front of it: v_lshlrev_b64.
    // The prefix sum of m = -nbBits over the stream's four lanes runs in place on two v_add_u32_dpp, row_shr:1 and row_shr:2 without
    // bound_ctrl: a stream's lanes open a DPP row, so lane 0 (lanes 0, 1) has no source and keeps its value; the chunk runs with
    // EXEC = the states' lanes only.  The funnel shifts and a second v_sub for m fill the two wait states a DPP read of a fresh
    // VGPR needs.
    // The state a round ends with is staged in the tail, behind the window reads (the chunk's first one by the prologue).
    // LDS queue at the top of a round, oldest first: entry, window (2), stage.
#define LS_CHUNK4() do { \
        uint32_t e, c, a, m, p, at, tot; \
        const uint64_t ls_em = LS_SPW == 4 ? 0x000F000F000F000Full : LS_SPW == 3 ? 0x0000000F000F000Full : LS_SPW == 2 ? 0x00000000000F000Full : 0xFull; \
        q -= 32; \
        asm volatile(".set ls_off, 8\n\t" \
                     "s_mov_b64 exec, %[em]\n\t" \
                     "v_lshl_add_u32 %[at], %[st], 1, %[cb]\n\t" \
                     "ds_read_u16 %[e], %[at]\n\t" \
                     "v_bfe_u32 %[at], %[q], 5, %[RW]\n\t" \
                     "v_lshl_add_u32 %[at], %[at], 2, %[ringb]\n\t" \
                     "ds_read2_b32 v[60:61], %[at] offset1:1\n\t" \
                     "ds_read_b32 v62, %[at] offset:8\n\t" \
                     "ds_write_b16 %[stg], %[st]\n\t" \
                     ".rept 32\n\t" \
                     "s_waitcnt lgkmcnt(3)\n\t" \
                     "v_ffbh_u32 %[c], %[e]\n\t" \
                     "v_sub_u32 %[a], %[C], %[c]\n\t" \
                     "s_waitcnt lgkmcnt(1)\n\t" \
                     "v_alignbit_b32 v58, v61, v60, %[q]\n\t" \
                     "v_add_u32_dpp %[a], %[a], %[a] row_shr:1 row_mask:0xf bank_mask:0xf\n\t" \
                     "v_alignbit_b32 v59, v62, v61, %[q]\n\t" \
                     "v_sub_u32 %[m], %[C], %[c]\n\t" \
                     "v_add_u32_dpp %[a], %[a], %[a] row_shr:2 row_mask:0xf bank_mask:0xf\n\t" \
                     "v_sub_u32 %[p], %[m], %[a]\n\t" \
                     "v_lshlrev_b64 v[56:57], %[p], v[58:59]\n\t" \
                     ".if %[ZBF]\n\t" \
                     "v_alignbit_b32 %[p], %[e], v57, %[m]\n\t" \
                     "v_cmp_eq_u32 vcc, 0, %[m]\n\t" \
                     "v_cndmask_b32 %[st], %[p], %[e], vcc\n\t" \
                     ".else\n\t" \
                     "v_alignbit_b32 %[st], %[e], v57, %[m]\n\t" \
                     ".endif\n\t" \
                     "v_lshl_add_u32 %[at], %[st], 1, %[cb]\n\t" \
                     "ds_read_u16 %[e], %[at]\n\t" \
                     "v_mov_b32_dpp %[tot], %[a] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf\n\t" \
                     "v_add_u32 %[q], %[q], %[tot]\n\t" \
                     "v_bfe_u32 %[at], %[q], 5, %[RW]\n\t" \
                     "v_lshl_add_u32 %[at], %[at], 2, %[ringb]\n\t" \
                     "ds_read2_b32 v[60:61], %[at] offset1:1\n\t" \
                     "ds_read_b32 v62, %[at] offset:8\n\t" \
                     ".if ls_off < 256\n\t" \
                     "ds_write_b16 %[stg], %[st] offset:ls_off\n\t" \
                     ".endif\n\t" \
                     ".set ls_off, ls_off+8\n\t" \
                     ".endr\n\t" \
                     "s_waitcnt lgkmcnt(0)\n\t" \
                     "s_mov_b64 exec, -1" \
                     : [st] "+v"(st), [q] "+v"(q), [e] "=&v"(e), [c] "=&v"(c), [a] "=&v"(a), [m] "=&v"(m), [p] "=&v"(p), [at] "=&v"(at), [tot] "=&v"(tot) \
                     : [C] "v"(C), [cb] "v"(cb), [ringb] "v"(ringb), [stg] "v"(stgb), [RW] "n"(LS_RBITS), [ZBF] "n"(ZB ? 1 : 0), [em] "s"(ls_em) \
                     : "memory", "vcc", "v56", "v57", "v58", "v59", "v60", "v61", "v62"); \
        q += 32; \
    } while (0)
    // ---- chunks of 128 symbols per stream ---------------------------------------------------------------------------
    constexpr uint32_t R = 128 / N;                                         // rounds per chunk
    const uint32_t chunks = count / 128u, rem = count - chunks * 128u;
    uint32_t maxch = 0;
#pragma unroll
    for (int j = 0; j < LS_SPW; j++) if (s_have[j]) maxch = max(maxch, s_chunks[j]);
    maxch = (uint32_t)__builtin_amdgcn_readfirstlane((int)maxch);           // uniform by construction; keep the chunk loop scalar
    uint32_t sv_st = st; int32_t sv_q = q;                                  // a shorter stream's true state after its last whole chunk
#ifdef LS_STAMP
    uint64_t stamp[4] = { 0, 0, 0, 0 }, t_prev = __builtin_amdgcn_s_memtime();
#define LS_T(i) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xC07F); stamp[i] += t_ - t_prev; t_prev = t_; } while (0)
#else
#define LS_T(i) do { } while (0)
#endif
    for (uint32_t ch = 0; ch < maxch; ch++) {
        if (ch == chunks) { sv_st = st; sv_q = q; }                         // (per lane) this stream is done: it runs on, harmlessly, on its own table
        if (N == 2) LS_CHUNK2();
        else if (N == 4) LS_CHUNK4();
        else {
#pragma unroll
            for (uint32_t r = 0; r < R; r++) round(r * N * 2u);
        }
        LS_T(0);
        // the chunk's 128 states per stream are staged: out they go (lane l: states 2l, 2l+1), and the ring moves on.
        // Order: every consumer of last chunk's prefetch first -- the wait on the memory counter is then for operations that
        // have had a whole chunk to complete -- then the new loads, then the stores (vmcnt counts loads and stores together, in
        // order: a ring store behind a fresh global store would wait for that store's acknowledgement).
#pragma unroll
        for (int j = 0; j < LS_SPW; j++) store_blk(j, s_pfb[j], pf[j]);
        LS_T(1);
#pragma unroll
        for (int j = 0; j < LS_SPW; j++) {
            s_blk[j] = ((int32_t)ls_rl((uint32_t)q, j * LS_LS) >> 5) >> 6;
            s_pfb[j] = s_blk[j] - LS_DEPTH;
            pf[j] = load_blk(j, s_pfb[j]);
        }
        LS_T(2);
        {
            uint32_t s2[LS_SPW];
#pragma unroll
            for (int j = 0; j < LS_SPW; j++) s2[j] = *(ls_l32)(uintptr_t)((wv * LS_SPW + (uint32_t)j) * LS_STREAM_BYTES + LS_STAGE + lane * 4);
#pragma unroll
            for (int j = 0; j < LS_SPW; j++)                                // (a finished stream decodes garbage: its descriptor ends at its last whole chunk)
                __builtin_amdgcn_raw_buffer_store_b32(s2[j], rs_out[j], (int)(ch * 256u + lane * 4u), 0, 2);
        }
        LS_T(3);
    }
#ifdef LS_STAMP
    if (lane == 0) { MicUnit &ud = units[list[slot0]]; for (int i = 0; i < 4; i++) ud.dbg[i] = (uint32_t)(stamp[i] >> 4); ud.dbg[4] = maxch; }
#endif
    if (chunks < maxch) { st = sv_st; q = sv_q; }                           // (per lane) back to the true end-of-chunks state
    if (maxch) {   // ... and the rings back to where those states read (the run-off moved them on); harmless for the longest stream
#pragma unroll
        for (int j = 0; j < LS_SPW; j++) {
            if (!s_have[j]) continue;
            const int32_t b = ((int32_t)ls_rl((uint32_t)q, j * LS_LS) >> 5) >> 6;
#pragma unroll
            for (int dd = -1; dd <= 2; dd++) store_blk(j, b - dd, load_blk(j, b - dd));   // (a tail of 127 symbols can take 64 dwords at tableLog 16)
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
    }
    // ---- tails: rem < 128 tokens per stream; a state past the stream's last token neither moves nor takes bits ----------
    {
        uint32_t maxrem = 0;
#pragma unroll
        for (int j = 0; j < LS_SPW; j++) if (s_have[j]) maxrem = max(maxrem, ls_rl(rem, j * LS_LS));
#pragma unroll 1
        for (uint32_t r = 0; r * N < maxrem; r++) {
            const bool valid = r * N + k < rem;                             // fse2state.go:293-305 and siblings: the last states in lane order
            const uint32_t e = entry(st);
            if (real) *(ls_l16)(uintptr_t)(stgb + r * N * 2u) = (uint16_t)st;
            const uint32_t nbr = (uint32_t)__builtin_clz(e) - C;
            const uint32_t nb = valid ? nbr : 0u;
            uint32_t pre, ntot; prefix(nb, pre, ntot);
            const uint32_t hi = window(q - (int32_t)pre);
            const uint32_t nx = (uint32_t)((((uint64_t)e << 32) | hi) >> (32u - nb));
            st = valid ? nx : st;
            q += (int32_t)ntot;
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
#pragma unroll
        for (int j = 0; j < LS_SPW; j++) {
            if (!s_have[j]) continue;
            const uint32_t rj = ls_rl(rem, j * LS_LS), done = s_chunks[j] * 128u;
            const uint32_t s2 = *(ls_l32)(uintptr_t)((wv * LS_SPW + (uint32_t)j) * LS_STREAM_BYTES + LS_STAGE + lane * 4);
            const ls_gu16 o = (ls_gu16)(uintptr_t)s_out[j];
            if (2 * lane < rj) o[done + 2 * lane] = (uint16_t)s2;
            if (2 * lane + 1 < rj) o[done + 2 * lane + 1] = (uint16_t)(s2 >> 16);
        }
    }
    // ---- results: one lane per stream -------------------------------------------------------------------------------
    if (have && lane % LS_LS == 0 && lane < LS_SPW * LS_LS) {
        MicUnit &uo = units[list[slot0 + (int)g]];
        uo.dec_kernel = 1u + (uint32_t)((TL <= 12 ? 4 : TL - 13) * 6 + (N == 2 ? 0 : N == 4 ? 2 : 4) + (ZB ? 1 : 0));   // this instance's class, as mic_dec_cls numbers it
        // bitreader.go:113-120: more bits taken than the stream holds -- a prefix has read only the bits behind its own symbols
        if (count == uo.count && q + 32 - (int32_t)(8u * sb) < 0) uo.status = MICD_ERR_CORRUPT;
        else { uo.ntok = count; uo.dec_stage = MIC_STAGE_STATES; }   // tok holds STATES: k_dec_translate turns them into symbols
    }
}

// ==========================================================================================
// The split instances: two states, tableLog 13, no 0-bit entries, and every long stream decoded as PARTS (two, four or eight) parts by as
// many decoders that share the stream's table.  A tANS decoder that starts at a wrong bit position with wrong
// states falls in with the true one after a few thousand symbols when a symbol replaces most of a state's bits with stream bits
// (9.6 of 13 on the headline's strips).  So part 0 starts at the true start and writes true states to tok; part p >= 1 starts
// further down the stream with two states read from the bits there and writes to region p - 1 (R tokens each) of the unit's sym
// slab, idle between the table stage and k_dec_translate.  Part p >= 1 hands its position and states after W symbols to part
// p - 1, which runs until it has passed that position; once it reaches it with the same two states, role by role, everything
// part p decoded from there on is the stream's.
//   * lane 2 PARTS g + 2 part + k holds state k of part `part` of the wave's stream g (12, 24 or 48 state lanes a wave); the other
//     lanes clone lane k of stream 0's part 0 (same addresses, same values);
//   * a part has its own ring (4 blocks of B = 64 / PARTS dwords), mirror and stage: a chunk is 128 / PARTS symbols of the same
//     hand-scheduled round as the unsplit instance (LS_CHUNK2_N);
//   * the per-chunk upkeep serves the parts of a stream with one instruction each: lanes B p ... B p + B - 1 part p's block; one
//     ds_bpermute per stream brings every upkeep lane its part's position.
// Ring reach, as for LsGeom with blocks of B dwords: a chunk of 2 B symbols takes at most 2 B * 13 bits = 13 B / 16 < B dwords; the
// reads are three dwords from the dword of p - 32 on for every position p of the chunk, its last included: with D the dword of the
// chunk's first position, in block b, they span dwords D - 13 B / 16 - 1 ... D + 1 (B = 32: D - 27, B = 16: D - 14);
// D - 13 B / 16 - 1 >= B b - 13 B / 16 - 1 = B (b - 1) + 3 B / 16 - 1 (+ 5, + 2), inside block b - 1, and D + 1 inside block b + 1 at
// the most: the three stored blocks.  B = 8 has no dword to spare: a chunk of 16 symbols takes at most 208 bits = 6.5 dwords, the
// lowest read starts at the dword of p0 - 208 - 32 for a first position p0 >= 32 D, which is floor(D - 7.5) = D - 8 >= 8 (b - 1):
// exactly the first dword of block b - 1 when D is block b's first, and 6.5 < 8 keeps a chunk from crossing two blocks.  The block
// in flight (b - 2) takes the slot of block b + 2 at the chunk's end, which no chunk from here on reads.  The position behind the two initial states is at most 26 bits below the start, so the same three blocks
// hold what the initial states read.
// Where the parts start: Lb the stream's bits, Wb = W symbols' worth of bits at the mean rate, x = (Lb + (PARTS - 1) Wb) / PARTS;
// part p >= 1 starts at bit (PARTS - p) x - (PARTS - 1 - p) Wb, so that every part covers about x bits, W symbols of them under its
// upper neighbour (two parts: part 1 starts at x = (Lb + Wb) / 2).
// Joins: behind the chunk loop lane 0 of part p < PARTS - 1 steps part p symbol by symbol from its last chunk start above part
// p + 1's hand-over position q until its position is q, the PARTS - 1 joins of a stream side by side; the parts have met when its
// two states there are part p + 1's, role by role (part p's own step parity against part p + 1 at its step W, which is even: with
// an odd step index the lower part's lanes are role-swapped against the symbol parity, its output order is the symbol order all
// the same); e_p is part p's step index there (p >= 1: at least W).  One lane per stream turns them into token indices, I_1 = e_0,
// I_p+1 = I_p + e_p - W: token i of [I_p, I_p+1) is part p's step W + i - I_p (I_PARTS = count).  Checked there: I_1 inside part
// 0's whole chunks, every part's last step inside its region, and the last part's count by the over-read rule (bitreader.go:113-120:
// it must decode count - I_last + W steps without reading below bit 0).  The first boundary that fails names the outcome, and the
// whole unit -- no meeting, no room, a cut or damaged stream -- goes to the retry list, which the unsplit instance decodes and
// reports as it always has.
// Eight parts differ in three things (the third is the cache policy, LsParts::AUX).  A region holds a part's steps from W on (step j >= W at region offset j - W): the W steps in
// front are the overlap, which k_dec_translate never reads and the joins do not need, so seven regions of a seventh of the slab
// hold the parts of a full strip; the room checks are e_p - W <= R and j_end - W <= R, and tokens [I_p, I_p+1) lie at
// sym[(p - 1) R + i - I_p].  And what the instance hands back goes to the end of the four-part list, not to the retry list: a miss
// then costs a four-part chain instead of an unsplit one; the four-part instance, launched behind it, judges the unit afresh.
// LS_STAMP builds (tools/time_dec.py): shader-clock ticks per phase of the chunk loop, summed over the chunks, into dbg[] of the
// wave's first unit through ordinary stores -- 0 rounds, 1 ring stores, 2 loads, 3 state stores, 4 hand-over, snapshot and ballot;
// dbg[5] chunks, dbg[6] parts per stream.  The partner instance (eight parts): the chain wave's 0 rounds, 1 publish, 2 the wait for its
// partner, 4 as above (3 stays 0: the upkeep is not there; a pass has two of each phase and every slot keeps its per-chunk meaning), and
// the partner wave's own period in dbg[8 ..]: 8 waiting for the chunk, 9 positions, stage, ring fills, served and loads, 10 state stores,
// dbg[11] its chunks
#ifdef LS_STAMP
#define LS_ST_DECL uint64_t stamp[5] = { 0, 0, 0, 0, 0 }, t_prev = __builtin_amdgcn_s_memtime()
#define LS_ST_OUT(parts_) do { if (lane == 0) { MicUnit &ud = units[unit_i]; for (int i_ = 0; i_ < 5; i_++) ud.dbg[i_] = (uint32_t)(stamp[i_] >> 4); \
                                                ud.dbg[5] = ch_end; ud.dbg[6] = (parts_); } } while (0)
#else
#define LS_ST_DECL do { } while (0)
#define LS_ST_OUT(parts_) do { } while (0)
#endif
template <int PARTS> struct LsParts {
    static_assert(PARTS == 2 || PARTS == 4 || PARTS == 8, "a part needs a ring block of at least 8 dwords: a chunk of 128 / PARTS symbols must not cross two");
    static constexpr int TL = 13, SPW = 3, WAVES = 3;
    static constexpr int CHUNK = 128 / PARTS;                               // symbols of a chunk of one part: 64 | 32 | 16
    static constexpr int BLK = 64 / PARTS, BLK_SHIFT = PARTS == 2 ? 5 : PARTS == 4 ? 4 : 3;   // dwords of a ring block = upkeep lanes of a part: 32 | 16 | 8
    static constexpr int RING_BLOCKS = 4, DEPTH = 2, RING_BITS = BLK_SHIFT + 2;
    static constexpr uint32_t MIRROR = 4u * BLK * RING_BLOCKS;              // two mirror dwords + two pad dwords
    static constexpr uint32_t STAGE = MIRROR + 16u;                         // CHUNK u16 states of a chunk
    // Eight parts: the per-chunk upkeep (ring fills, state stores) is done by a PARTNER wave per chain wave (wave WAVES + w serves
    // chain wave w), which needs the chunk's stage twice, by chunk parity, and a mailbox per chain wave (protocol: above the kernel)
    static constexpr bool PARTNER = PARTS == 8;
    static constexpr int GROUP_WAVES = PARTNER ? 2 * WAVES : WAVES;
    static constexpr uint32_t STAGE_BYTES = 2u * CHUNK;
    static constexpr uint32_t PART_BYTES = STAGE + (PARTNER ? 2u : 1u) * STAGE_BYTES;   // 656 | 336 | 208
    static constexpr uint32_t TAB = (uint32_t)PARTS * PART_BYTES;           // the parts in front of the stream's table
    static constexpr uint32_t STREAM_BYTES = TAB + (2u << TL);              // 17 696 | 17 728 | 18 048
    static constexpr uint32_t MAILBOX = WAVES * SPW * STREAM_BYTES;         // behind the streams: MB_BYTES per chain wave
    static constexpr uint32_t MB_BYTES = PARTNER ? 256u : 0u;               // two halves (chunk parity) of 32 words: SPW * PARTS positions, then the words below
    static constexpr uint32_t MB_HALF = 128u;
    static constexpr uint32_t MB_DONE = 24u * 4u, MB_SERVED = 25u * 4u, MB_BAIL = 26u * 4u, MB_OWN = 27u * 4u;   // (in half 0; MB_OWN: SPW words)
    static constexpr uint32_t MB_FIN = 0x80000000u;                         // in the DONE word: the chain wave has left its loop
    static constexpr uint32_t LDS = MAILBOX + WAVES * MB_BYTES;             // 159 264 | 159 552 | 163 200
    static_assert(LDS <= 160 * 1024, "one group must fit a CU's LDS");
    static_assert(!PARTNER || SPW * PARTS <= 24, "the mailbox's words lie behind the positions");
    // Polls the partner waits for its chain wave's next chunk before it gives up: the chain wave's own bound (MicSplitCfg::partner_bound,
    // the longest it can stand still in front of a chunk) is added to it in the kernel.  Its own share covers the chain wave's start
    // (three tables, 48 KiB through one wave: some 10^4 cycles) and a chunk (some 10^3) 10^4 times over at 200 cycles a poll
    static constexpr uint32_t PARTNER_POLLS = 1u << 20;
    // Eight parts: a region holds a part's steps from W on only (step j at region offset j - W) -- the first W are the overlap, which
    // nothing reads: the joins are stepped from register snapshots.  Two and four parts keep the layout they were measured with
    static constexpr bool SKIP_W = PARTS == 8;
    // Cache policy of the chunk loop's buffer loads and state stores.  Two and four parts stream them (nt): a store instruction
    // writes segments of 128 and 64 bytes.  Eight parts write 32-byte segments, four chunks to a cache line about 2000 cycles apart:
    // streamed, the wait for the ring's loads stood behind those stores' acknowledgements for 800 cycles a chunk, 2400 in all (vmcnt
    // counts in order), and fetching two chunks ahead did not move it; left to the L2 to combine it is 310, 1940 in all, and
    // k_dec_translate finds part of the states there (profiles/tans2_split8_ab.json)
    static constexpr int AUX = PARTS == 8 ? 0 : 2;
    // R, the tokens of one of the PARTS - 1 scratch regions, in whole chunks.  Recorded, and every NO_ROOM outcome depends on it, so
    // each instance keeps its rule: two parts' one region is the slab, clamped by the stream's length (part 1 never has to hold
    // more); four parts' is a third of the slab whatever the stream's length (the sym slab is at least a tok slab), eight parts' a
    // seventh
    static __device__ __forceinline__ uint32_t region(uint32_t sym_cap, uint32_t tok_cap, uint32_t T) {
        const uint32_t slab = min(sym_cap, tok_cap);
        return (PARTS == 2 ? min(slab, T) : slab / (uint32_t)(PARTS - 1)) & ~(uint32_t)(CHUNK - 1);
    }
};

// a mailbox word (LsParts::PARTNER): every lane reads the same address, or one lane writes; volatile, and fenced against the compiler
// moving the ring and stage accesses across it -- the LDS itself serves a wave's operations in the order it issued them
__device__ __forceinline__ uint32_t ls_mb_get(uint32_t a) {
    asm volatile("" ::: "memory");
    const uint32_t v = *(volatile __attribute__((address_space(3))) uint32_t *)(uintptr_t)a;
    asm volatile("" ::: "memory");
    return v;
}
__device__ __forceinline__ void ls_mb_put(uint32_t a, uint32_t v) {
    asm volatile("" ::: "memory");
    *(volatile __attribute__((address_space(3))) uint32_t *)(uintptr_t)a = v;
    asm volatile("" ::: "memory");
}

// The partner protocol (eight parts).  The group has six waves: waves 0-2 are the chain waves with today's roles and lanes, wave 3 + w
// is the partner of chain wave w and does its per-chunk upkeep: it fills the parts' rings and sends the chunks' states out.  The two
// talk through chain wave w's mailbox in LDS, and through nothing else:
//   chain wave, behind chunk c:   the parts' positions into half c & 1 of the mailbox, then DONE = c + 1 (chunks run), then a read of
//                                 SERVED that nothing waits for: the loop test of the next chunk runs in its shadow;
//   chain wave, in front of c:    SERVED >= c - 1, by one compare on that read; else it polls (counted: MicUnit.partner[2]);
//   partner, for c = 0, 1, ...:   waits for DONE > c; reads the positions and the stage of half c & 1; where a part's position has reached a
//                                 new block b, puts block b - 2 into the ring from its register queue; SERVED = c + 1; then what goes to
//                                 memory: the queue's loads, and the states with the same two stores per stream as ever.
// A pass of either loop is two chunks, an even one and an odd one: the halves are immediates and fixed registers, and the chain wave has its
// wave-uniform exit test in front of the even chunk only.  It may so run one chunk behind the last that any part is on for: nothing is on in
// it, no snapshot moves, every record keeps its value; the chunk reads zeros below the stream, its states go where a shorter stream's go
// beside a longer neighbour (behind every token that is read, or nowhere: `fits`, tok's descriptor), and the partner serves it like any other
// (tests/tans_pairs_model.py).  The hand-over chunk is tested for in front of both chunks of a pass.
// Deadline (tests/tans_partner_model.py states it and tests/test_tans_partner_cpu.py checks it on the fastest consumers found): chunk c + 2
// starts in block b or b - 1 when b is the block of the position behind chunk c, and reads no lower than the block under its own, b - 2:
// the fill for chunk c.  That block takes the slot of b + 2, and chunk c + 1, which may be running, reads b + 1 .. b - 1.  Chunk c + 2 is
// also the next to write stage half c & 1 and mailbox half c & 1.  So SERVED >= c - 1 in front of chunk c is all a chain wave needs, and
// the partner has a whole chunk's time for work that touches LDS only: its loads run two blocks ahead of the ring.  The chain wave
// fills the four blocks b + 1 .. b - 2 of its first position itself, so chunks 0 and 1 wait for nobody.
// Ends: a chain wave that leaves its loop sets MB_FIN in DONE; the partner serves what is outstanding and leaves.  Every wait is a poll
// with s_sleep and a bound (the chain wave's: MicSplitCfg::partner_bound, some 400 cycles a poll: the default is 10^8 cycles, 10^4 times
// a partner's worst chunk -- three loads that miss to HBM, some 10^4 cycles; the partner's: LsParts::PARTNER_POLLS on top of that); a
// bound that runs out sets BAIL, the other side leaves at its next poll, and the wave's units are handed to the four-part list as
// MIC_SPLIT_STALLED.  The partner of a chain wave without units returns with it, before either touches the mailbox again.
template <int PARTS>
__global__ void __launch_bounds__(64 * LsParts<PARTS>::GROUP_WAVES) k_dec_tans_ls_parts(MicUnit *units, const int *list, const int *count_p, int *retry_list,
                                                                                      int *retry_count, uint32_t overlap, uint32_t wait_bound) {
    using G = LsParts<PARTS>;
    constexpr int LS_SPW = G::SPW, LS_RBITS = G::RING_BITS, LS_DEPTH = G::DEPTH;
    constexpr bool ZB = false;
    constexpr uint32_t tl = G::TL, size = 1u << tl, SB = G::STREAM_BYTES, PB = G::PART_BYTES, CH = G::CHUNK, BLK = G::BLK, LP = 2u * PARTS;
    extern __shared__ uint32_t s_mem[];
    const uint32_t lane = threadIdx.x & 63, wv_g = threadIdx.x >> 6;
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)s_mem != 0u) return;   // layout assumes dynamic LDS at 0
    const bool partner = G::PARTNER && wv_g >= (uint32_t)G::WAVES;         // (wave-uniform)
    const uint32_t wv = partner ? wv_g - (uint32_t)G::WAVES : wv_g;        // the chain wave: its own number, or the one this partner serves
    const uint32_t mb = G::MAILBOX + wv * G::MB_BYTES;
    if constexpr (G::PARTNER) {                                             // the one barrier: zeroed mailboxes, in front of every return
        if (!partner) *(ls_l32)(uintptr_t)(mb + lane * 4u) = 0u;
        __syncthreads();
    }
    const int n_cls = *count_p;
    const int slot0 = __builtin_amdgcn_readfirstlane(((int)blockIdx.x * G::WAVES + (int)wv) * LS_SPW);
    if (slot0 >= n_cls) return;                                             // waves share nothing and never meet at a barrier
    // ---- roles: lane LP g + 2 part + k; the lanes behind the last stream clone lane k of stream 0's part 0 ----
    const uint32_t k = lane & 1u;
    const bool real = lane < LP * LS_SPW;
    const uint32_t g = real ? lane / LP : 0u, part = real ? (lane >> 1) & (uint32_t)(PARTS - 1) : 0u;
    const bool last_part = part == (uint32_t)(PARTS - 1);                   // it has no lower neighbour: it stops at the stream's end
    const bool have = slot0 + (int)g < n_cls;
    const uint32_t gs = have ? g : 0u;                                      // absent streams run on stream 0's table, on rings of zeros
    const int unit_i = list[slot0 + (int)gs];
    const MicUnit &u = units[unit_i];
    const uint32_t T = have ? u.count : 0u;
    const uint32_t bits_off = u.bits_off, len = u.comp_len - bits_off;
    const uint32_t vbase = (wv * LS_SPW + g) * SB + part * PB;              // own ring / mirror / stage
    const uint32_t tbase = (wv * LS_SPW + gs) * SB + G::TAB;
    // ---- tables, as in k_dec_tans_ls: one per stream, all parts read it ----
#pragma unroll 1
    for (int j = 0; j < LS_SPW; j++) {
        if (slot0 + j >= n_cls || partner) break;
        const uint32_t *dt = (const uint32_t *)(uintptr_t)ls_rl64((uint64_t)(uintptr_t)u.tt_nb, (int)LP * j);
        const uint32_t tb = (wv * LS_SPW + (uint32_t)j) * SB + G::TAB;
        for (uint32_t p = lane * 4; p < size; p += 256) {
            const uint4 e = *(const uint4 *)(dt + p);
            const uint32_t n0 = ((e.x & 0xFFFF) + size) >> (e.x >> 16), n1 = ((e.y & 0xFFFF) + size) >> (e.y >> 16);
            const uint32_t n2 = ((e.z & 0xFFFF) + size) >> (e.z >> 16), n3 = ((e.w & 0xFFFF) + size) >> (e.w >> 16);
            ls_v2 v; v.x = n0 | (n1 << 16); v.y = n2 | (n3 << 16);
            *(__attribute__((address_space(3))) ls_v2 *)(uintptr_t)(tb + p * 2) = v;
        }
    }
    // ---- bit reader: grid of aligned dwords under the stream, as in k_dec_tans_ls ----
    const uint8_t *bs = u.comp_in + bits_off;
    const uint32_t last = bs[len - 1];                                      // non-zero: k_dec_classify
    const uintptr_t addr = (uintptr_t)bs;
    const uint32_t sb = (uint32_t)(addr & 3);
    const uint64_t gaddr = (uint64_t)(addr - sb);
    const uint32_t Lb = 8u * (len - 1) + (uint32_t)(31 - __clz(last));      // the stream's bits (below the end marker)
    const int32_t cur0 = (int32_t)(Lb + 8u * sb);
    const int32_t top_dw = have ? (cur0 - 1) >> 5 : -1;
    // part p >= 1 starts at bit (PARTS - p) x - (PARTS - 1 - p) Wb (Wb <= Lb, so Wb <= x <= Lb and the starts lie in [x, Lb], in falling order)
    const uint32_t Wb = T ? (uint32_t)min((uint64_t)overlap * (uint64_t)Lb / (uint64_t)T, (uint64_t)Lb) : 0u;
    const uint32_t x = (uint32_t)(((uint64_t)Lb + (uint64_t)(PARTS - 1) * (uint64_t)Wb) / (uint32_t)PARTS);
    const uint32_t pm = (uint32_t)((uint64_t)((uint32_t)PARTS - part) * (uint64_t)x - (uint64_t)((uint32_t)(PARTS - 1) - part) * (uint64_t)Wb);
    int32_t q = (part ? (int32_t)(pm + 8u * sb) : cur0) - 32;               // window of a round = grid bits [q, q+32)
    const int32_t qz = (int32_t)(8u * sb) - 32;                             // q of "no bits left"
    const uint32_t R = G::region(u.sym_cap, u.tok_cap, T);                  // tokens of a scratch region
    bool s_have[LS_SPW];
    __amdgpu_buffer_rsrc_t rs_in[LS_SPW], rs_tok[LS_SPW], rs_scr[LS_SPW];
    uint32_t s_R[LS_SPW];
#pragma unroll
    for (int j = 0; j < LS_SPW; j++) {
        const int src = (int)LP * j;
        s_have[j] = slot0 + j < n_cls;
        s_R[j] = (uint32_t)__builtin_amdgcn_readfirstlane((int)(s_have[j] ? ls_rl(R, src) : 0u));
        const uint32_t in_bytes = (uint32_t)__builtin_amdgcn_readfirstlane((int)(s_have[j] ? ((uint32_t)((int32_t)ls_rl((uint32_t)top_dw, src) + 1)) * 4u : 0u));
        const uint32_t tok_bytes = (uint32_t)__builtin_amdgcn_readfirstlane((int)(s_have[j] ? (ls_rl(T, src) / CH) * CH * 2u : 0u));
        const uint32_t scr_bytes = s_R[j] * 2u * (uint32_t)(PARTS - 1);     // PARTS - 1 regions of R states
        rs_in[j] = __builtin_amdgcn_make_buffer_rsrc((void *)(uintptr_t)ls_rl64(gaddr, src), 0, (int)in_bytes, 0x00020000);
        rs_tok[j] = __builtin_amdgcn_make_buffer_rsrc((void *)(uintptr_t)ls_rl64((uint64_t)(uintptr_t)u.tok, src), 0, (int)tok_bytes, 0x00020000);
        rs_scr[j] = __builtin_amdgcn_make_buffer_rsrc((void *)(uintptr_t)ls_rl64((uint64_t)(uintptr_t)u.sym, src), 0, (int)scr_bytes, 0x00020000);
    }
    const uint32_t up = lane >> G::BLK_SHIFT, lb = lane & (BLK - 1u);       // upkeep: lanes BLK p .. BLK p + BLK - 1 serve part p
    constexpr uint32_t LS_OOB = 0x7FFFFFF0u;                                // a byte offset no descriptor here reaches: the access is dropped
    auto blk_of = [&](int j, int32_t qq) -> int32_t {                      // block of the position of this lane's part of stream j (all lanes take part)
        return (__builtin_amdgcn_ds_bpermute((int)((LP * (uint32_t)j + 2u * up) << 2), qq) >> 5) >> G::BLK_SHIFT;
    };
    auto load_blk = [&](int j, int32_t b) -> uint32_t {                    // dword lb of block b of stream j, zero outside the stream
        return __builtin_amdgcn_raw_buffer_load_b32(rs_in[j], (b * (int32_t)BLK + (int32_t)lb) * 4, 0, G::AUX);
    };
    auto store_blk = [&](int j, int32_t b, uint32_t v) {
        const uint32_t rb = (wv * LS_SPW + (uint32_t)j) * SB + up * PB;
        const uint32_t slot = (uint32_t)b & (uint32_t)(G::RING_BLOCKS - 1);
        *(ls_l32)(uintptr_t)(rb + (slot * BLK + lb) * 4) = v;
        if (lb < 2) *(ls_l32)(uintptr_t)(rb + G::MIRROR + lb * 4 + (slot == 0u ? 0u : 8u)) = v;   // mirror | pad (an address select)
    };
    uint32_t pf[LS_SPW]; int32_t pfb[LS_SPW];
#pragma unroll
    for (int j = 0; j < LS_SPW; j++) {
        const int32_t b = blk_of(j, q - (int32_t)(2 * tl));                 // block of the position BEHIND the initial states
        if constexpr (G::PARTNER) {
            // the chain wave fills all four slots, b + 1 .. b - 2; the partner's queue starts with the block under them
            pfb[j] = b - LS_DEPTH - 1;
            if (!partner) {
#pragma unroll
                for (int dd = -1; dd <= LS_DEPTH; dd++) store_blk(j, b - dd, load_blk(j, b - dd));
            }
            continue;
        }
#pragma unroll
        for (int dd = -1; dd < LS_DEPTH; dd++) store_blk(j, b - dd, load_blk(j, b - dd));
        pfb[j] = b - LS_DEPTH;
        pf[j] = load_blk(j, pfb[j]);                                        // enters the rings at the end of the first chunk
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);                                     // wave-private LDS: the writes above are in before the reads below
    // ---- chain state ----
    const uint32_t ringb = vbase;
    uint32_t stgb = vbase + G::STAGE + 2u * k;                              // stage16[r * 2 + k] = state k of round r (eight parts: of stage half chunk & 1)
    const uint32_t cb = tbase - 2u * size;
    const uint32_t C = 31u - tl;
    auto window = [&](int32_t qq) -> uint32_t {
        const uint32_t a = (__builtin_amdgcn_ubfe((uint32_t)qq, 5, LS_RBITS) << 2) + ringb;
        const uint32_t w0 = *(ls_l32)(uintptr_t)a, w1 = *(ls_l32)(uintptr_t)(a + 4);
        return __builtin_amdgcn_alignbit(w1, w0, (uint32_t)qq);
    };
    auto entry = [&](uint32_t s) -> uint32_t { return *(ls_l16)(uintptr_t)(s * 2 + cb); };
    // initial states: part 0's are the stream's, the others' the same read at their starts -- valid table indices, but guesses
    uint32_t st = size + (window(q - (int32_t)(k * tl)) >> (32u - tl));
    q -= (int32_t)(2 * tl);
    const uint32_t mk1 = k ? ~0u : 0u;
    // ---- chunks of CH symbols per part ----
    const uint32_t Wc = (uint32_t)__builtin_amdgcn_readfirstlane((int)(overlap / CH));
    uint32_t maxT = 0;
#pragma unroll
    for (int j = 0; j < LS_SPW; j++) if (s_have[j]) maxT = max(maxT, ls_rl(T, (int)LP * j));
    const uint32_t ch_cap = (uint32_t)__builtin_amdgcn_readfirstlane((int)(maxT / CH + 2u));   // no part of the wave has anything to decode behind it
    // ... and no part of this stream behind its own T / CH + 2: what a part does is its stream's business alone.  c < T / CH + 2 is
    // (c - 1) CH <= T, a scalar product against a value the lane holds anyway (T < 2^31: a token takes a bit at least)
    auto own_chunk = [&](uint32_t c) -> bool { return (int32_t)((c - 1u) * CH) <= (int32_t)T; };
    const uint32_t nl = ((lane & ~1u) + 2u) & 63u;                          // the next part's first lane (the last part has none)
    // the scratch regions: byte offset of this lane's dword of chunk 0 (part 0's lanes aim out of range), and the same for tok
    uint32_t scr0[LS_SPW];
#pragma unroll
    for (int j = 0; j < LS_SPW; j++) scr0[j] = up ? (PARTS > 2 ? (up - 1u) * s_R[j] * 2u : 0u) + lb * 4u : LS_OOB;
    const uint32_t tok0 = up ? LS_OOB : lb * 4u;
    // (the partner instance) one chunk's states of this lane's part of every stream: out of the stage at byte offset `half` ...
    auto take_stage = [&](uint32_t half, uint32_t (&s2)[LS_SPW]) {
#pragma unroll
        for (int j = 0; j < LS_SPW; j++) s2[j] = *(ls_l32)(uintptr_t)((wv * LS_SPW + (uint32_t)j) * SB + up * PB + G::STAGE + half + lb * 4);
    };
    // ... and to tok and the scratch regions
    auto send_states = [&](uint32_t c, const uint32_t (&s2)[LS_SPW]) {
        const uint32_t off = c * 2u * CH;                                   // (part 0 runs on into a descriptor that ends at its last whole chunk)
        // eight parts: a region starts at step W, and the chunks in front of it are not stored (both terms below are wave-uniform)
        const uint32_t ch0 = G::SKIP_W ? Wc : 0u, soff = (c - ch0) * 2u * CH;
#pragma unroll
        for (int j = 0; j < LS_SPW; j++) {
            const bool fits = c >= ch0 && (c + 1u - ch0) * CH <= s_R[j];    // (a part that runs on past its region must not write into its neighbour's)
            __builtin_amdgcn_raw_buffer_store_b32(s2[j], rs_tok[j], (int)(tok0 + off), 0, G::AUX);   // (out of range + off < 2^32: still out of range)
            __builtin_amdgcn_raw_buffer_store_b32(s2[j], rs_scr[j], (int)(fits ? scr0[j] + soff : LS_OOB), 0, G::AUX);
        }
    };
    if constexpr (G::PARTNER) if (partner) {
        // ---- the partner wave: lanes BLK p .. BLK p + BLK - 1 serve part p of each of the chain wave's streams ----
        // Two blocks per part wait in registers, block pfb, what the ring takes next, and the one under it, each in the register of its
        // parity: pfe the even one, pfo the odd one.  A block enters the queue when the part reaches a new block and enters the ring two
        // such advances later, so its load has two chunks at the least to arrive, and no register is moved when the queue moves on: a
        // move would have to wait for the newest load.  Whether a part advances in a chunk is the stream's business (a chunk takes 0 to
        // 6.5 of a block's 8 dwords), so the roles are picked by a select on the block's parity and cannot be fixed per half of a pass.
        // Every chunk loads both blocks of the queue again, each lane its own two: a block that is there already arrives as the same
        // dwords, what is read meanwhile is right, and every load instruction has all its lanes, so the count below holds whatever the
        // parts do.  The loop's loads are asm: the value is not there when the statement is done, and the one wait that covers them, at
        // the top of a chunk's service, names what may still be out behind them (vmcnt counts in order)
        uint32_t pfe[LS_SPW], pfo[LS_SPW], touch = 0;
#pragma unroll
        for (int j = 0; j < LS_SPW; j++) {
            const uint32_t l0 = load_blk(j, pfb[j]), l1 = load_blk(j, pfb[j] - 1);
            const bool odd = (pfb[j] & 1) != 0;
            pfe[j] = odd ? l1 : l0; pfo[j] = odd ? l0 : l1;
        }
        const uint32_t polls = G::PARTNER_POLLS + min(wait_bound, 1u << 30);
        uint32_t c = 0, fin = 0;
        bool bail = false;
#ifdef LS_STAMP
        uint64_t pst[3] = { 0, 0, 0 }, pt = __builtin_amdgcn_s_memtime();
#define LS_PT(i) do { const uint64_t t_ = __builtin_amdgcn_s_memtime(); pst[i] += t_ - pt; pt = t_; } while (0)
#else
#define LS_PT(i) do { } while (0)
#endif
        // chunk c, of parity `half` (a literal at both calls: the mailbox half and the stage half are immediates) -> false: the chain
        // wave has left its loop and nothing is outstanding, or one side has given up
        auto serve = [&](const uint32_t half) __attribute__((always_inline)) -> bool {
            for (uint32_t tries = 0;; tries++) {                            // chunk c: run and published?
                const uint32_t dn = (uint32_t)__builtin_amdgcn_readfirstlane((int)ls_mb_get(mb + G::MB_DONE));
                fin = dn & G::MB_FIN;
                if ((dn & ~G::MB_FIN) > c) { fin = 0; break; }
                if (fin) break;                                             // the chain wave has left its loop, and nothing is outstanding
                if (__builtin_amdgcn_readfirstlane((int)ls_mb_get(mb + G::MB_BAIL)) != 0 || tries >= polls) { bail = true; break; }
                __builtin_amdgcn_s_sleep(2);
            }
            if (fin || bail) return false;
            LS_PT(0);
            int32_t qp[LS_SPW];
#pragma unroll
            for (int j = 0; j < LS_SPW; j++) qp[j] = (int32_t)ls_mb_get(mb + half * G::MB_HALF + ((uint32_t)j * (uint32_t)PARTS + up) * 4u);
            uint32_t s2[LS_SPW];
            take_stage(half * G::STAGE_BYTES, s2);                          // (issued here: they arrive while the rings are filled)
            // the loads of two chunks ago and everything older: a chunk is six loads, three touches and six stores, in this order, so what
            // may stay out is the chunk before (15) and the touches and stores of the one before that (9)
            asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
#pragma unroll
            for (int j = 0; j < LS_SPW; j++) {
                const bool adv = ((qp[j] >> 5) >> G::BLK_SHIFT) - LS_DEPTH <= pfb[j];   // the part has reached a new block: one at most per chunk
                if (adv) store_blk(j, pfb[j], (pfb[j] & 1) ? pfo[j] : pfe[j]);
                pfb[j] -= adv ? 1 : 0;
            }
            // SERVED, as soon as the chain wave may rely on it: behind the ring stores and the stage reads (the LDS keeps a wave's order),
            // in front of everything that goes to memory -- the chain wave looks at it once, right behind its next chunk
            if (lane == 0) ls_mb_put(mb + G::MB_SERVED, c + 1u);
#pragma unroll
            for (int j = 0; j < LS_SPW; j++) {                              // blocks pfb and pfb - 1: the even one of the two, and the odd one
                const int32_t off_e = ((pfb[j] & ~1) * (int32_t)BLK + (int32_t)lb) * 4, off_o = (((pfb[j] - 1) | 1) * (int32_t)BLK + (int32_t)lb) * 4;
                asm volatile("buffer_load_dword %[v], %[o], %[r], 0 offen" : [v] "+v"(pfe[j]) : [o] "v"(off_e), [r] "s"(rs_in[j]) : "memory");
                asm volatile("buffer_load_dword %[v], %[o], %[r], 0 offen" : [v] "+v"(pfo[j]) : [o] "v"(off_o), [r] "s"(rs_in[j]) : "memory");
            }
            // ... and a touch of the cache line under it (four blocks), behind the loads so that the wait above leaves it out: a block's
            // own load, a few chunks on, then finds the line in the L2 -- from HBM it took longer than a chunk, and the partner set the pace
#pragma unroll
            for (int j = 0; j < LS_SPW; j++) {
                const int32_t off = ((pfb[j] - 1 - 128 / 4 / (int32_t)BLK) * (int32_t)BLK + (int32_t)lb) * 4;
                asm volatile("buffer_load_dword %[v], %[o], %[r], 0 offen" : [v] "+v"(touch) : [o] "v"(off), [r] "s"(rs_in[j]) : "memory");
            }
            LS_PT(1);
            send_states(c, s2);
            LS_PT(2);
            c++;
            return true;
        };
        // a pass is two chunks, as the chain wave's: an even one out of the first halves, an odd one out of the second; FIN or BAIL ends
        // the loop in front of either
        while (serve(0u) && serve(1u)) { }
        if (bail) { if (lane == 0) ls_mb_put(mb + G::MB_BAIL, 1u); }
        // chunks served, per unit: what the chain wave says the unit's own parts ran (MB_OWN, in front of MB_FIN), or what was served of it
        if (lane < (uint32_t)LS_SPW && slot0 + (int)lane < n_cls) {
            const uint32_t own = fin ? ls_mb_get(mb + G::MB_OWN + lane * 4u) : ~0u;
            units[list[slot0 + (int)lane]].partner[1] = min(c, own);
        }
#ifdef LS_STAMP
        if (lane == 0) { MicUnit &ud = units[list[slot0]]; for (int i = 0; i < 3; i++) ud.dbg[8 + i] = (uint32_t)(pst[i] >> 4); ud.dbg[11] = c; }
#endif
        return;
    }
    bool handed = false;
    uint32_t m_ab = 0;                                                      // the next part's two states after Wc chunks, second << 16 (a state is below 2^14)
    int32_t qlim = last_part ? qz : INT32_MIN;                              // a part is on above it: nothing up to the hand-over, then the next part's
                                                                            // position after Wc chunks; the last part: bits left
    int32_t sn_q = q; uint32_t sn_st = st, sn_ch = 0;                       // snapshot: the last chunk start above qlim
    uint32_t ch = 0;
    // the partner instance: the lane's word of mailbox half 0, and the stage of the odd chunks (the halves of a chunk are immediates
    // and fixed registers: a pass of the loop is an even chunk and an odd one)
    [[maybe_unused]] const uint32_t mb_pos = mb + (g * (uint32_t)PARTS + part) * 4u, stgb1 = stgb + G::STAGE_BYTES;
    [[maybe_unused]] uint32_t mb_sv = 0, not_ready = 0;
    [[maybe_unused]] bool stalled = false;
    LS_ST_DECL;
    // in front of a chunk, per lane: the hand-over (uniform, once), and the snapshot -- the last chunk start above the limit
#define LS_PARTS_FRONT() \
        if (ch == Wc) {                                                     /* (uniform, once) */ \
            const int32_t qn = __builtin_amdgcn_ds_bpermute((int)(nl << 2), q); \
            m_ab = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(nl << 2), (int)st) | \
                   ((uint32_t)__builtin_amdgcn_ds_bpermute((int)((nl | 1u) << 2), (int)st) << 16); \
            qlim = last_part ? qz : qn; \
            handed = true; \
        } \
        const bool on = own_chunk(ch) & (q > qlim);                         /* (selects, no branch) */ \
        sn_q = on ? q : sn_q; sn_st = on ? st : sn_st; sn_ch = on ? ch : sn_ch; \
        asm volatile("" : "+v"(sn_q), "+v"(sn_st), "+v"(sn_ch))             /* (taken here: sunk behind the chunk, the selects keep the old q and st alive across it) */
    // The partner instance's chunk `ch` of parity HALF_ (a literal: stage, mailbox half and their offsets are immediates).  In front: SERVED
    // as it was behind the last chunk (the read was issued there; everything from there to here ran in its shadow); a partner that is
    // not ready is polled for (the slow path), and a bound that runs out leaves the loop (`break`: the macro stands in the loop's own
    // body).  Behind: the positions (lanes of role 0 of the 24 parts), then DONE, then the read of SERVED for the next chunk's test
#define LS_PARTNER_CHUNK(HALF_) \
        { \
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(mb_sv) :: "memory"); \
            uint32_t sv = (uint32_t)__builtin_amdgcn_readfirstlane((int)mb_sv); \
            if (__builtin_expect(sv + 1u < ch, 0)) { \
                not_ready++; \
                for (uint32_t tries = 0;; tries++) { \
                    sv = (uint32_t)__builtin_amdgcn_readfirstlane((int)ls_mb_get(mb + G::MB_SERVED)); \
                    if (sv + 1u >= ch) break; \
                    if (__builtin_amdgcn_readfirstlane((int)ls_mb_get(mb + G::MB_BAIL)) != 0 || tries + 1u >= wait_bound) { stalled = true; break; } \
                    __builtin_amdgcn_s_sleep(1); \
                } \
                if (stalled) break; \
            } \
            LS_T(2); \
            if constexpr ((HALF_) != 0) LS_CHUNK2_AT("4", "32", stgb1); else LS_CHUNK2_AT("4", "32", stgb); \
            LS_T(0); \
            const uint64_t em_pos = 0x0000555555555555ull, em_one = 1ull; \
            const uint32_t dn = ch + 1u; \
            asm volatile("s_mov_b64 exec, %[ep]\n\t" \
                         "ds_write_b32 %[pa], %[q] offset:%[HO]\n\t" \
                         "s_mov_b64 exec, %[e1]\n\t" \
                         "ds_write_b32 %[da], %[dn]\n\t" \
                         "ds_read_b32 %[sv], %[da] offset:%[SO]\n\t" \
                         "s_mov_b64 exec, -1" \
                         : [sv] "=&v"(mb_sv) \
                         : [pa] "v"(mb_pos), [q] "v"(q), [da] "v"(mb + G::MB_DONE), [dn] "v"(dn), [ep] "s"(em_pos), [e1] "s"(em_one), \
                           [SO] "n"(G::MB_SERVED - G::MB_DONE), [HO] "n"((HALF_) * G::MB_HALF) \
                         : "memory"); \
            LS_T(1); \
        }
    if constexpr (G::PARTNER) {
        // A pass is two chunks, an even one and an odd one, and the wave-uniform exit test stands in front of the even one only: the
        // wave runs at most one chunk more than its last part that is on needs.  In front of that chunk no lane is on (on only ever
        // goes off: q falls, the limit rises once, own_chunk ends), so the snapshots, and with them every record, keep their values;
        // its states go where a shorter stream's go beside a longer neighbour -- behind the tokens anything reads, or nowhere (`fits`,
        // tok's descriptor) --, its ring reads below the stream are zeros, and the partner serves it like any other.  ch <= ch_cap + 1
        for (;;) {
            {
                LS_PARTS_FRONT();
                if (ch >= ch_cap || !__any(on & real & have)) break;        // one wave-uniform test per pass
            }
            LS_T(4);
            LS_PARTNER_CHUNK(0)
            ch++;
            { LS_PARTS_FRONT(); }
            LS_T(4);
            LS_PARTNER_CHUNK(1)
            ch++;
        }
    } else {
        for (;; ch++) {
            LS_PARTS_FRONT();
            if (ch >= ch_cap || !__any(on & real & have)) break;            // one wave-uniform test per chunk
            LS_T(4);
            if constexpr (PARTS == 2) LS_CHUNK2_N("16", "128"); else LS_CHUNK2_N("8", "64");
            LS_T(0);
            // upkeep, in the order of k_dec_tans_ls: consumers of last chunk's prefetch, then the loads, then the stores
#pragma unroll
            for (int j = 0; j < LS_SPW; j++) store_blk(j, pfb[j], pf[j]);
            LS_T(1);
#pragma unroll
            for (int j = 0; j < LS_SPW; j++) pfb[j] = blk_of(j, q) - LS_DEPTH;
#pragma unroll
            for (int j = 0; j < LS_SPW; j++) pf[j] = load_blk(j, pfb[j]);
            LS_T(2);
            {
                uint32_t s2[LS_SPW];
#pragma unroll
                for (int j = 0; j < LS_SPW; j++) s2[j] = *(ls_l32)(uintptr_t)((wv * LS_SPW + (uint32_t)j) * SB + up * PB + G::STAGE + lb * 4);
                const uint32_t off = ch * 2u * CH;                          // (part 0 runs on into a descriptor that ends at its last whole chunk)
#pragma unroll
                for (int j = 0; j < LS_SPW; j++) {
                    const bool fits = (ch + 1u) * CH <= s_R[j];             // (a part that runs on past its region must not write into its neighbour's)
                    __builtin_amdgcn_raw_buffer_store_b32(s2[j], rs_tok[j], (int)(tok0 + off), 0, G::AUX);   // (out of range + off < 2^32: still out of range)
                    __builtin_amdgcn_raw_buffer_store_b32(s2[j], rs_scr[j], (int)(fits ? scr0[j] + off : LS_OOB), 0, G::AUX);
                }
            }
            LS_T(3);
        }
    }
    const uint32_t ch_end = ch;                                             // chunks every part ran and stored
    if constexpr (G::PARTNER) {
        // the unit's own chunks (its parts' last chunk that was on, + 1: a longer neighbour keeps the wave going), for the partner's
        // record, then MB_FIN beside the chunks run; a stalled wave sets BAIL instead.  Nothing below needs the partner, the rings or the stage
        uint32_t own = real && have ? sn_ch + 1u : 0u;
#pragma unroll
        for (uint32_t d = 1; d < LP; d <<= 1) own = max(own, (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane ^ d) << 2), (int)own));
        if (real && (lane & (LP - 1u)) == 0u) ls_mb_put(mb + G::MB_OWN + g * 4u, own);
        if (lane == 0) ls_mb_put(stalled ? mb + G::MB_BAIL : mb + G::MB_DONE, stalled ? 1u : ch_end | G::MB_FIN);
    }
    LS_ST_OUT((uint32_t)PARTS);
    // ---- the joins: boundary p | p + 1 by lane 0 of part p, those of a stream side by side ----
    const uint32_t sn_s1 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane | 1u) << 2), (int)sn_st);
    const uint32_t *grid = (const uint32_t *)(uintptr_t)gaddr;
    auto peek = [&](int32_t qq) -> uint32_t {                              // grid bits [qq, qq + 32), zeros outside the stream's dwords
        const int32_t d = qq >> 5;
        const uint32_t w0 = (d >= 0 && d <= top_dw) ? grid[d] : 0u, w1 = (d + 1 >= 0 && d + 1 <= top_dw) ? grid[d + 1] : 0u;
        return __builtin_amdgcn_alignbit(w1, w0, (uint32_t)qq);
    };
    auto step = [&](uint32_t &s, int32_t &pos) {                           // one symbol: nbBits >= 1 in this class
        const uint32_t e = entry(s), nb = (uint32_t)__builtin_clz(e) - C;
        s = (e << nb) | (peek(pos) >> (32u - nb));
        pos -= (int32_t)nb;
    };
    const uint32_t W = Wc * CH;
    uint32_t met = 0, e_p = 0;
    if (real && have && handed && own_chunk(Wc) && k == 0u && !last_part) { // (not its own chunk: a longer neighbour kept the loop going up to the hand-over)
        const int32_t qn = qlim;                                            // (handed, not the last part: the limit is the neighbour's hand-over position)
        uint32_t s0 = sn_st, s1 = sn_s1, i = sn_ch * CH; int32_t pos = sn_q;
        const uint32_t i_min = part ? W : 0u;                               // (a part's own first W steps are not its output)
        for (int n = 0; n <= (int)CH && pos >= qn; n++) {
            if (pos == qn) {
                const uint32_t nxt = (i & 1u) ? s1 : s0, oth = (i & 1u) ? s0 : s1;
                if (i >= i_min && (nxt | (oth << 16)) == m_ab) { met = 1u; e_p = i; }
                break;
            }
            if (i & 1u) step(s1, pos); else step(s0, pos);
            i++;
        }
    }
    // ---- one lane per stream: the other boundaries' results and the last part's snapshot (all lanes take part in the permutes) ----
    const uint32_t l0 = lane & ~(LP - 1u), ll = l0 + LP - 2u;               // the stream's first lane, its last part's first lane
    uint32_t mets[PARTS - 1] = { met }, es[PARTS - 1] = { e_p };
#pragma unroll
    for (int b = 1; b < PARTS - 1; b++) {
        mets[b] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((l0 + 2u * (uint32_t)b) << 2), (int)met);
        es[b] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((l0 + 2u * (uint32_t)b) << 2), (int)e_p);
    }
    const uint32_t pl_s0 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(ll << 2), (int)sn_st);
    const uint32_t pl_s1 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((ll + 1u) << 2), (int)sn_st);
    const int32_t pl_q = __builtin_amdgcn_ds_bpermute((int)(ll << 2), sn_q);
    const uint32_t pl_ch = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(ll << 2), (int)sn_ch);
    if (!(real && have && lane == l0)) return;
    // boundary b = 1 .. PARTS - 1: met, then room -- I_1 inside tok's whole chunks, part b - 1's last step e inside its region; then
    // the stream's end (PARTS): the last part's room and its count.  (Two parts: I_2 = I_3 = ~0, "no bound" to k_dec_translate)
    // Eight parts: a region holds steps from W on, so the room is e - W <= R and j_end - W <= R (e >= W: the join's i_min)
    constexpr int NI = PARTS > 4 ? PARTS - 1 : 3;
    uint32_t outcome = MIC_SPLIT_DONE, fail = 0, I[NI];
#pragma unroll
    for (int b = 0; b < NI; b++) I[b] = b && PARTS == 2 ? ~0u : 0u;
    const uint32_t dead = G::SKIP_W ? W : 0u;                               // a part's steps that its region does not hold
    {
        uint32_t at = 0;
#pragma unroll
        for (int b = 0; b < PARTS - 1; b++) {
            if (outcome != MIC_SPLIT_DONE) break;
            if (!mets[b]) { outcome = MIC_SPLIT_NOT_MET; fail = (uint32_t)b + 1u; break; }
            at = b ? at + es[b] - W : es[0];
            I[b] = at;
            if (b ? es[b] - dead > R : at > (T / CH) * CH) { outcome = MIC_SPLIT_NO_ROOM; fail = (uint32_t)b + 1u; }
        }
    }
    if (outcome == MIC_SPLIT_DONE) {
        fail = (uint32_t)PARTS;
        if (I[PARTS - 2] > T) outcome = MIC_SPLIT_BAD_COUNT;                 // (the parts in front hold more than the stream's symbols)
        else {
            const uint32_t j_end = T - I[PARTS - 2] + W, js = pl_ch * CH;   // the last part must hold steps [W, j_end)
            if (j_end - dead > R) outcome = MIC_SPLIT_NO_ROOM;
            else if (j_end > ch_end * CH) outcome = MIC_SPLIT_BAD_COUNT;    // (the loop ended: the last part was out of bits with symbols to go)
            else if (j_end > js) {
                // the over-read rule at the stream's last symbol: the last part's position behind step j_end - 1, from its last chunk start with bits left
                if (j_end - js > CH) outcome = MIC_SPLIT_BAD_COUNT;        // (the chunk behind the snapshot started without bits)
                else {
                    uint32_t s0 = pl_s0, s1 = pl_s1; int32_t pos = pl_q;
                    for (uint32_t j = js; j < j_end; j++) { if (j & 1u) step(s1, pos); else step(s0, pos); }
                    if (pos < qz) outcome = MIC_SPLIT_BAD_COUNT;
                }
            }
        }
        if (outcome == MIC_SPLIT_DONE) fail = 0u;
    }
    if constexpr (G::PARTNER) {
        if (stalled) { outcome = MIC_SPLIT_STALLED; fail = 0u; for (int b = 0; b < NI; b++) I[b] = 0u; }
    }
    MicUnit &uo = units[unit_i];
    if constexpr (G::PARTNER) { uo.partner[0] = 1u; uo.partner[2] = not_ready; uo.partner[3] = stalled ? 1u : 0u; }
    uo.split[0] = outcome; uo.split[1] = I[0]; uo.split[2] = W; uo.split[3] = I[1]; uo.split[4] = I[2];
    uo.split[5] = R; uo.split[6] = fail; uo.split[7] = (uint32_t)PARTS;
    if constexpr (PARTS == 8) { uo.split_hi[0] = I[3]; uo.split_hi[1] = I[4]; uo.split_hi[2] = I[5]; uo.split_hi[3] = I[6]; }
    if (outcome == MIC_SPLIT_DONE) {
        uo.dec_kernel = 1u;                                                 // class 0, as the unsplit instance reports it
        uo.ntok = T; uo.dec_stage = MIC_STAGE_STATES;                // tok and sym hold STATES: k_dec_translate joins and translates them
    } else retry_list[atomicAdd(retry_count, 1)] = unit_i;                  // (eight parts: the four-part list, behind what k_dec_classify put there)
}

// ==========================================================================================
// States -> symbols, and the RLE header walk.  One group of 256 threads per unit that k_dec_tans_ls decoded (MIC_STAGE_STATES):
// the unit's symbol table (tableSymbol of each state, <= 16 KiB) sits in LDS, waves 1-3 stream the states through it in tiles
// of 1536 (16 bytes in, eight LDS look-ups, 16 bytes out, in place) and leave each translated tile in LDS as well, where wave 0
// follows the linked list of RLE headers through it (rledecompressu16.go:59-85: a header <= midCount is a run of one value, a
// larger one a literal chunk) one tile behind -- no dependent HBM read per header.
// The walk is a serial chain (the next header's position is this one's value), but a self-synchronising one: a walk started at
// a wrong token lands on a true header within a few steps and is the true walk from there.  Where headers are dense (run-heavy
// streams: WaveletV2 coefficients, WSI planes) every lane therefore walks its 24 tokens of the tile from their first token on
// its own, noting the positions it visits in a bit mask; the true walk then hops from lane to lane -- "is the position I
// arrive at in your mask? then your exit is mine" (two v_readlane per 24 tokens instead of a loop trip per header; a lane whose
// mask misses the arrival walks again from there) -- and the headers from the arrival bit on are the true ones.  Segment
// records then leave from all lanes at once behind two DPP prefix sums (record index, first symbol).  Where headers are sparse
// (long literal chunks: noisy frames) the plain header-to-header loop is the cheaper one; the previous tile's count picks.
// Stop and error rules are MicRleWalk's (mic_rlewalk.h), which is the header-to-header loop: on an error the segments are dropped and the consumer
// (k_dec_pixels_wg) walks the stream itself and reports it.  Frames (mode 0) are walked, other units are translated only.
#define TR_THREADS 256                            // one walker wave + three translating waves: seven groups (walkers) per CU -- the walk is
                                                  // serial per unit, and on run-dense streams (WSI planes) it is what a unit waits for
#define TR_TILE ((TR_THREADS - 64) * 8)
#define TR_SEG (TR_TILE / 64)                     // tokens per walker lane
#define TR_DENSE 6                                // headers in a tile from which on the next one is walked by all lanes
static_assert(TR_SEG == 24 && TR_SEG * 64 == TR_TILE, "lane = position / 24 below is (position * 2731) >> 16");
template <int TRTL>   // 13: tables up to 2^13 states (two groups per CU) | 16: up to 2^16 (128 KiB of LDS: one group per CU)
__global__ void __launch_bounds__(TR_THREADS) k_dec_translate(MicUnit *units) {
    MicUnit &u = units[blockIdx.x];
    if (u.status != MICD_OK || u.dec_stage != MIC_STAGE_STATES) return;
    if ((TRTL == 13) != (u.table_log <= 13)) return;
    __shared__ uint16_t s_sym[1 << TRTL];
    __shared__ __attribute__((aligned(16))) uint16_t s_tile[2][TR_TILE + 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t size = 1u << u.table_log, ntok = u.ntok;
    {
        const uint32_t *src = (const uint32_t *)u.tab_sym;                  // 256 KiB-aligned slab
        for (uint32_t i = tid; i < size / 2; i += TR_THREADS) ((uint32_t *)s_sym)[i] = src[i];
    }
    uint16_t *tok = u.tok;
    // a split unit (k_dec_tans_ls_parts): the states of tokens [I_p, I_p+1) still lie in the scratch slab, sym[(p - 1) R + W + i - I_p];
    // they are read from there and written, translated, to tok -- everything behind this pass sees an ordinary tok.  Up to three
    // bounds b1 <= b2 <= b3 (none: ~0, which is what a two-part unit's record holds for I_2 and I_3) and, for the tokens from bound p
    // on, the offset o_p from token index to scratch index (modulo 2^32)
    // An eight-part unit (split[7] = 8) has four more bounds in split_hi, and its regions hold no steps in front of W:
    // sym[(p - 1) R + i - I_p].  All of this is uniform per unit
    const bool sp = TRTL == 13 && u.split[0] == MIC_SPLIT_DONE, sp8 = sp && u.split[7] == 8u;
    const uint32_t sp_R = u.split[5], sp_W = sp8 ? 0u : u.split[2];
    const uint32_t b1 = sp ? u.split[1] : ~0u, b2 = sp ? u.split[3] : ~0u, b3 = sp ? u.split[4] : ~0u;
    const uint32_t b4 = sp8 ? u.split_hi[0] : ~0u, b5 = sp8 ? u.split_hi[1] : ~0u, b6 = sp8 ? u.split_hi[2] : ~0u, b7 = sp8 ? u.split_hi[3] : ~0u;
    const uint32_t o1 = sp_W - b1, o2 = sp_R + sp_W - b2, o3 = 2u * sp_R + sp_W - b3;
    const uint32_t o4 = 3u * sp_R - b4, o5 = 4u * sp_R - b5, o6 = 5u * sp_R - b6, o7 = 6u * sp_R - b7;
    auto seg_of = [&](uint32_t i) -> uint32_t {
        return (uint32_t)(i >= b1) + (uint32_t)(i >= b2) + (uint32_t)(i >= b3) + (uint32_t)(i >= b4) + (uint32_t)(i >= b5) + (uint32_t)(i >= b6) +
               (uint32_t)(i >= b7);
    };
    auto scr_of = [&](uint32_t p, uint32_t i) -> uint32_t {
        return i + (p == 1u ? o1 : p == 2u ? o2 : p == 3u ? o3 : p == 4u ? o4 : p == 5u ? o5 : p == 6u ? o6 : o7);
    };
    const uint16_t *scr = u.sym;
    const bool frame = u.mode == 0 && u.seg != nullptr;
    // (a length-prefixed RLE stream, walk_mode 1 -- a whole WaveletV2 frame -- is one unit of millions of tokens: walking it here would
    //  be one wave's work per frame; it is marked MIC_STAGE_PARTS and walked in parts by k_rle_walk_parts, mic_wavelet.hip)
    const bool prefixed = u.mode == 1 && u.walk_mode == 1 && u.seg != nullptr;
    // walker (wave 0; uniform values: mic_rlewalk.h)
    MicRleWalk wk; wk.init(u, frame, ntok);
    bool w_dense = false;
    __syncthreads();
    typedef uint32_t tr_v4 __attribute__((ext_vector_type(4)));
    const uint32_t smask = size - 1;                                        // a state carries its +size offset: index = state - size
    for (uint32_t base = 0, it = 0; base < ntok; base += TR_TILE, it++) {
        const uint32_t tile_end = min(base + TR_TILE, ntok);
        uint16_t *tile = s_tile[it & 1];
        if (wave != 0) {
            const uint32_t l = (tid - 64) * 8, i0 = base + l;
            const uint32_t pseg = seg_of(i0);
            if (i0 + 8 <= tile_end && pseg == seg_of(i0 + 7u)) {
                tr_v4 v;
                if (pseg == 0u) v = __builtin_nontemporal_load((const tr_v4 *)(tok + i0));
                else {
                    // behind a join of a split unit: eight states from the scratch slab, 2-byte aligned only -- five aligned dwords and
                    // a funnel shift by the source's parity (the u16 in front of and behind the eight are inside the slab: W >= 32
                    // -- an eight-part unit's index is at least 0, and rounding it down to even stays there --, and the slab is 64
                    // tokens longer than what the parts may write)
                    const uint32_t sj = scr_of(pseg, i0);
                    const uint32_t *d = (const uint32_t *)(scr + (sj & ~1u));
                    const uint32_t sh = (sj & 1u) * 16u;
                    const uint32_t d0 = __builtin_nontemporal_load(d), d1 = __builtin_nontemporal_load(d + 1), d2 = __builtin_nontemporal_load(d + 2),
                                   d3 = __builtin_nontemporal_load(d + 3), d4 = __builtin_nontemporal_load(d + 4);
                    v.x = __builtin_amdgcn_alignbit(d1, d0, sh); v.y = __builtin_amdgcn_alignbit(d2, d1, sh);
                    v.z = __builtin_amdgcn_alignbit(d3, d2, sh); v.w = __builtin_amdgcn_alignbit(d4, d3, sh);
                }
                tr_v4 o;
                o.x = (uint32_t)s_sym[v.x & smask] | ((uint32_t)s_sym[(v.x >> 16) & smask] << 16);
                o.y = (uint32_t)s_sym[v.y & smask] | ((uint32_t)s_sym[(v.y >> 16) & smask] << 16);
                o.z = (uint32_t)s_sym[v.z & smask] | ((uint32_t)s_sym[(v.z >> 16) & smask] << 16);
                o.w = (uint32_t)s_sym[v.w & smask] | ((uint32_t)s_sym[(v.w >> 16) & smask] << 16);
                *(tr_v4 *)(tok + i0) = o;
                *(tr_v4 *)(tile + l) = o;
            } else {
                for (uint32_t i = i0; i < min(i0 + 8u, tile_end); i++) {   // the tile's tail, or the eight tokens that straddle a join (or two)
                    const uint32_t p = seg_of(i);
                    const uint16_t t = s_sym[(p ? scr[scr_of(p, i)] : tok[i]) & smask]; tok[i] = t; tile[i - base] = t;
                }
            }
        }
        __syncthreads();                                                    // tile `it` is in LDS; the walker is done with tile it - 1
        if (wave != 0 || !wk.on || wk.pos >= tile_end) continue;
        if (wk.pos == 0) {                                                  // token 0 fixes the run / literal split
            wk.first(tile[0]);
            if (!wk.on) continue;
        }
        const uint32_t nseg_in = wk.nseg;
        if (!w_dense) {
            // ---- header to header, from a 64-token window and v_readlane ----
            while (wk.on && wk.pos < tile_end) {
                const uint32_t rel = wk.pos - base;                         // (>= 0: a header inside an earlier tile was taken there)
                const uint32_t wv = (rel + lane < tile_end - base) ? (uint32_t)tile[rel + lane] : 0u;
                uint32_t j = 0;
                while (j < 64 && wk.on && wk.pos < tile_end) j += wk.step(ls_rl(wv, (int)j), lane);   // j >= 64: the next header is outside the window
            }
        } else {
            // ---- all lanes: lane l walks tokens [24 l, 24 l + 24) of the tile from the first one on; the true walk enters at rel0 ----
            // (the walker's stop and error rules in data-parallel form: only the header classifier is shared with it)
            const uint32_t tlen = tile_end - base, rel0 = wk.pos - base;
            const uint32_t s0 = lane * TR_SEG, s1 = min(s0 + TR_SEG, tlen);
            uint32_t mask = 0, ex = 0;
            auto lane_walk = [&](uint32_t p) {                              // mask: visited positions (bit = position - s0); ex: where the walk leaves
                mask = 0;                                                   // the lane's tokens, ~0 when it met a zero header (an error if true)
                while (p < s1) {
                    const uint32_t h = tile[p];
                    if (h == 0) { p = 0xFFFFFFFFu; break; }
                    mask |= 1u << (p - s0);
                    p += mic_rle_hdr(h, wk.mid).adv;
                }
                ex = p;
            };
            { const uint32_t p0 = max(s0, rel0); if (p0 < s1) lane_walk(p0); }
            uint32_t ent = 0xFFu;                                           // bit at which the true walk enters this lane's tokens (none: it jumps over them)
            uint32_t cur = rel0;
            while (cur < tlen) {
                const uint32_t s = (cur * 2731u) >> 16, bit = cur - s * TR_SEG;
                const uint32_t m = ls_rl(mask, (int)s);
                if (!((m >> bit) & 1u)) { if (lane == s) lane_walk(cur); }  // not where that lane's own walk went: it walks again from here
                if (lane == s) ent = bit;
                cur = ls_rl(ex, (int)s);
            }
            const uint32_t tm = (ent != 0xFFu) ? (mask & (0xFFFFFFFFu << ent)) : 0u;   // this lane's true headers
            uint32_t oc = 0;
            for (uint32_t t = tm; t; t &= t - 1) oc += mic_rle_hdr(tile[s0 + (uint32_t)__builtin_ctz(t)], wk.mid).len;
            const uint32_t hc = (uint32_t)__popc(tm);
            const uint32_t ihc = mic_wave_incl_add(hc), ioc = mic_wave_incl_add(oc);
            const uint32_t tot_h = ls_rl(ihc, 63), tot_o = ls_rl(ioc, 63);
            uint32_t idx = wk.nseg + ihc - hc, o = wk.out + ioc - oc, nval = 0;
            bool bad = ent != 0xFFu && ex == 0xFFFFFFFFu && wk.out + ioc < wk.symcap;   // the zero header is reached before the stream has its symbols
            for (uint32_t t = tm; t; t &= t - 1) {
                const uint32_t b = (uint32_t)__builtin_ctz(t), pos = base + s0 + b;
                const MicRleHdr hd = mic_rle_hdr(tile[s0 + b], wk.mid);
                if (o < wk.symcap) {
                    if (idx >= wk.segcap || (hd.run && pos + 1 >= ntok)) bad = true;
                    else {
                        MicRleWalk::v2 r; r.x = hd.rec(pos); r.y = o; wk.seg[idx] = r;
                    }
                    nval++;
                }
                idx++; o += hd.len;
            }
            if (__ballot(bad)) { wk.fail(); continue; }
            if (wk.out + tot_o >= wk.symcap) { wk.nseg += ls_rl(mic_wave_incl_add(nval), 63); wk.on = false; }   // the stream has its symbols: headers behind that are not read
            else wk.nseg += tot_h;
            wk.out += tot_o;
            wk.pos = base + cur;
        }
        w_dense = wk.nseg - nseg_in >= TR_DENSE;
    }
    if (tid == 0) {
        if (frame && !wk.err) wk.finish(u);
        else u.dec_stage = prefixed ? MIC_STAGE_PARTS : MIC_STAGE_NONE;
    }
}

// States -> symbols for the units k_dec_translate has no header walk to do for (a whole WaveletV2 frame: one unit of millions of
// tokens, its headers walked in parts by k_rle_walk_parts) and whose table is the 128 KiB one: the table takes a CU's LDS, so a unit has
// the CU to itself whatever the kernel -- and then three translating waves behind a barrier per 1536 tokens leave it idle (2.0 ms for
// 256 CR frames).  Here: sixteen waves, no tile, no barrier; a wave takes every sixteenth block of 512 tokens.
#define TRW_THREADS 1024
__global__ void __launch_bounds__(TRW_THREADS) k_dec_translate_wide(MicUnit *units) {
    MicUnit &u = units[blockIdx.x];
    if (u.status != MICD_OK || u.dec_stage != MIC_STAGE_STATES || u.table_log <= 13) return;
    if (!(u.mode == 1 && u.walk_mode == 1 && u.seg != nullptr)) return;     // (frames and bare streams: k_dec_translate<16>, which walks)
    __shared__ uint16_t s_sym[1 << 16];
    const uint32_t tid = threadIdx.x;
    const uint32_t size = 1u << u.table_log, ntok = u.ntok, smask = size - 1;
    {
        const uint32_t *src = (const uint32_t *)u.tab_sym;
        for (uint32_t i = tid; i < size / 2; i += TRW_THREADS) ((uint32_t *)s_sym)[i] = src[i];
    }
    __syncthreads();
    uint16_t *tok = u.tok;
    typedef uint32_t tr_v4 __attribute__((ext_vector_type(4)));
    const uint32_t nvec = ntok / 8;
    for (uint32_t i = tid; i < nvec; i += TRW_THREADS) {
        const tr_v4 v = __builtin_nontemporal_load((const tr_v4 *)(tok + 8 * i));
        tr_v4 o;
        o.x = (uint32_t)s_sym[v.x & smask] | ((uint32_t)s_sym[(v.x >> 16) & smask] << 16);
        o.y = (uint32_t)s_sym[v.y & smask] | ((uint32_t)s_sym[(v.y >> 16) & smask] << 16);
        o.z = (uint32_t)s_sym[v.z & smask] | ((uint32_t)s_sym[(v.z >> 16) & smask] << 16);
        o.w = (uint32_t)s_sym[v.w & smask] | ((uint32_t)s_sym[(v.w >> 16) & smask] << 16);
        *(tr_v4 *)(tok + 8 * i) = o;
    }
    for (uint32_t i = 8 * nvec + tid; i < ntok; i += TRW_THREADS) tok[i] = s_sym[tok[i] & smask];
    __syncthreads();                                                        // (every state of the unit has been read as a state)
    if (tid == 0) u.dec_stage = MIC_STAGE_PARTS;                            // translated; the headers are k_rle_walk_parts's
}

template <int N, bool ZB, int TL> static void launch_ls_list(MicUnit *d_units, int n, const int *list, const int *count, hipStream_t stream);
template <int N, bool ZB, int TL>
static void launch_ls_class(MicUnit *d_units, int n, const int *d_list, const int *d_count, hipStream_t stream, uint32_t cls_mask) {
    constexpr int cls = (TL <= 12 ? 4 : TL - 13) * 6 + (N == 2 ? 0 : N == 4 ? 2 : 4) + (ZB ? 1 : 0);
    if (!((cls_mask >> cls) & 1u)) return;                                  // (the session has not seen a stream of this class lately: mic_launch.h)
    launch_ls_list<N, ZB, TL>(d_units, n, d_list + (size_t)cls * (size_t)n, d_count + cls, stream);
}
template <int N, bool ZB, int TL>
static void launch_ls_list(MicUnit *d_units, int n, const int *list, const int *count, hipStream_t stream) {
    constexpr int per = LsGeom<TL>::WAVES * LsGeom<TL>::SPW;
    static MicPerDeviceOnce once;
    once.run([] { (void)hipFuncSetAttribute((const void *)k_dec_tans_ls<N, ZB, TL>, hipFuncAttributeMaxDynamicSharedMemorySize, LsGeom<TL>::LDS); });
    const unsigned groups = (unsigned)((n + per - 1) / per);
    hipLaunchKernelGGL((k_dec_tans_ls<N, ZB, TL>), dim3(groups), dim3(64 * LsGeom<TL>::WAVES), LsGeom<TL>::LDS, stream, d_units, list, count);
}
// a split instance on list `from`; what it hands back goes to the end of list `to` (the groups cover n units: an instance launched
// behind it on `to` sees them)
template <int PARTS>
static void launch_ls_parts(MicUnit *d_units, int n, int *d_list, int *d_count, int from, int to, hipStream_t stream, uint32_t overlap,
                            uint32_t wait_bound = 0) {
    using G = LsParts<PARTS>;
    constexpr int per = G::WAVES * G::SPW;
    static MicPerDeviceOnce once;
    once.run([] { (void)hipFuncSetAttribute((const void *)k_dec_tans_ls_parts<PARTS>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS); });
    const unsigned groups = (unsigned)((n + per - 1) / per);
    hipLaunchKernelGGL((k_dec_tans_ls_parts<PARTS>), dim3(groups), dim3(64 * G::GROUP_WAVES), G::LDS, stream, d_units, d_list + (size_t)from * (size_t)n,
                       d_count + from, d_list + (size_t)to * (size_t)n, d_count + to, overlap, wait_bound ? wait_bound : 1u);
}
template <int TL>
static void launch_ls_tl(MicUnit *d_units, int n, const int *d_list, const int *d_count, hipStream_t stream, bool skip_first, uint32_t m) {
    if (!skip_first) launch_ls_class<2, false, TL>(d_units, n, d_list, d_count, stream, m);
    if constexpr (TL < 16) launch_ls_class<2, true, TL>(d_units, n, d_list, d_count, stream, m);
    launch_ls_class<4, false, TL>(d_units, n, d_list, d_count, stream, m);
    if constexpr (TL < 16) launch_ls_class<4, true, TL>(d_units, n, d_list, d_count, stream, m);
    launch_ls_class<8, false, TL>(d_units, n, d_list, d_count, stream, m);
    if constexpr (TL < 16) launch_ls_class<8, true, TL>(d_units, n, d_list, d_count, stream, m);
}

// d_list: MIC_CLS_LISTS * n ints, d_count: MIC_CLS_LISTS ints (session workspace)
void mic_launch_dec_tans_ls(MicUnit *d_units, int n, int *d_list, int *d_count, hipStream_t stream, MicTimer *t, uint32_t cls_mask, const MicSplitCfg *cfg) {
    const MicSplitCfg sc = cfg ? *cfg : MicSplitCfg{};
    const bool split = (cls_mask & MIC_CLS_SPLIT) != 0;
    if (t) t->mark("k_dec_classify");
    hipLaunchKernelGGL(k_dec_classify, dim3(1), dim3(1024), 0, stream, d_units, n, d_list, d_count, split ? 1 : 0, sc);
    if (split) {
        // the split instances first (the longest kernels of the chain, the one with the longest units in front), then what
        // they hand back: an empty list in the normal case, and the unsplit instance's blocks leave at once.  (Without the retry
        // launch k_dec_tans_gl would take those units: slower, not wrong.)  The eight-part instance hands back to the four-part one.
        if (t) t->mark("k_dec_tans_ls_split8<13>");
        launch_ls_parts<8>(d_units, n, d_list, d_count, LS_SPLIT8_LIST, LS_SPLIT4_LIST, stream, sc.overlap & ~63u, sc.partner_bound);
        if (t) t->mark("k_dec_tans_ls_split4<13>");
        launch_ls_parts<4>(d_units, n, d_list, d_count, LS_SPLIT4_LIST, LS_RETRY_LIST, stream, sc.overlap & ~63u);
        if (t) t->mark("k_dec_tans_ls_split<13>");
        launch_ls_parts<2>(d_units, n, d_list, d_count, LS_SPLIT_LIST, LS_RETRY_LIST, stream, sc.overlap & ~63u);
        if (cls_mask & MIC_CLS_RETRY) {
            if (t) t->mark("k_dec_tans_ls<2,false,13> retry");
            launch_ls_list<2, false, 13>(d_units, n, d_list + (size_t)LS_RETRY_LIST * (size_t)n, d_count + LS_RETRY_LIST, stream);
        }
    }
    if (t) t->mark("k_dec_tans_ls<2,false,13>");
    launch_ls_class<2, false, 13>(d_units, n, d_list, d_count, stream, cls_mask);
    if (t) t->mark("k_dec_tans_ls<other,13>");
    launch_ls_tl<13>(d_units, n, d_list, d_count, stream, true, cls_mask);
    if (t) t->mark("k_dec_tans_ls<..12>");
    launch_ls_tl<12>(d_units, n, d_list, d_count, stream, false, cls_mask);
    if (t) t->mark("k_dec_tans_ls<14..16>");
    launch_ls_tl<14>(d_units, n, d_list, d_count, stream, false, cls_mask);
    launch_ls_tl<15>(d_units, n, d_list, d_count, stream, false, cls_mask);
    launch_ls_tl<16>(d_units, n, d_list, d_count, stream, false, cls_mask);
    if (t) t->mark("k_dec_translate");
    // classes 0-5: tableLog 13, 24-29: tableLog <= 12 -> the 16 KiB symbol table; 6-23: tableLog 14..16 -> the 128 KiB one
    if (cls_mask & (0x3F00003Fu | MIC_CLS_SPLIT)) hipLaunchKernelGGL(k_dec_translate<13>, dim3((unsigned)n), dim3(TR_THREADS), 0, stream, d_units);
    if (cls_mask & 0x00FFFFC0u) {
        hipLaunchKernelGGL(k_dec_translate_wide, dim3((unsigned)n), dim3(TRW_THREADS), 0, stream, d_units);   // (marks its units MIC_STAGE_PARTS: the next launch skips them)
        hipLaunchKernelGGL(k_dec_translate<16>, dim3((unsigned)n), dim3(TR_THREADS), 0, stream, d_units);
    }
}

// debug probe (not in the public header): streams per wave and waves per group of the kernels of a table-size class
// (table_log 12 stands for every smaller one), 0 for no class
extern "C" int mic_hip_debug_ls_geom(int table_log, int *spw, int *waves) {
    switch (table_log) {
    case 12: *spw = LsGeom<12>::SPW; *waves = LsGeom<12>::WAVES; return 1;
    case 13: *spw = LsGeom<13>::SPW; *waves = LsGeom<13>::WAVES; return 1;
    case 14: *spw = LsGeom<14>::SPW; *waves = LsGeom<14>::WAVES; return 1;
    case 15: *spw = LsGeom<15>::SPW; *waves = LsGeom<15>::WAVES; return 1;
    case 16: *spw = LsGeom<16>::SPW; *waves = LsGeom<16>::WAVES; return 1;
    }
    return 0;
}
