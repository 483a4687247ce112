// mic_wave.h -- the wave64 and work-group primitives every kernel file shares: lane permutations, scans, reductions.
// Device functions only; no kernel, and no state beyond the LDS scratch a caller passes.
//
// Every function here is called by ALL 64 lanes of a wave (the group functions: by every thread of the group): a lane that is
// switched off reads as the identity at best.
//
// Toolchain rule (tools/dpp_subrev_repro.hip): on this toolchain `v_subrev_u32_dpp` computes the wrong
// difference for gfx950 when LLVM folds a lane permutation into `x - dpp(y)`.  So nothing in this file subtracts a permuted value:
// the DPP scans only add and take maxima, and an exclusive value is formed as `incl - v` from the register a scan has finished
// with, never inside a DPP operand chain.  A caller that needs `x - dpp(y)` negates before the permutation and adds.  (Read in the
// disassembly of every object built with this header when it was introduced: no v_subrev_*_dpp.)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

// The one spelling of a DPP move: lanes the control gives no source, and rows RMASK leaves out, read `old`.
// Controls used here: 0x111/2/4/8 row_shr 1/2/4/8, 0x142 row_bcast 15, 0x143 row_bcast 31, 0x130 wave_shl 1, 0x138 wave_shr 1.
template <int CTRL, int RMASK = 0xF>
__device__ __forceinline__ uint32_t mic_dpp(uint32_t old, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, RMASK, 0xF, false);
}

// Wave-wide inclusive scans on the DPP network (row_shr 1/2/4/8, then row_bcast 15 and 31); lanes without a source read the
// identity 0, so the same shape serves add and max of unsigned values.
__device__ __forceinline__ uint32_t mic_wave_incl_add(uint32_t v) {
    v += mic_dpp<0x111>(0u, v); v += mic_dpp<0x112>(0u, v); v += mic_dpp<0x114>(0u, v); v += mic_dpp<0x118>(0u, v);
    v += mic_dpp<0x142, 0xA>(0u, v); v += mic_dpp<0x143, 0xC>(0u, v);
    return v;
}
__device__ __forceinline__ uint32_t mic_wave_incl_max(uint32_t v) {
    v = max(v, mic_dpp<0x111>(0u, v)); v = max(v, mic_dpp<0x112>(0u, v)); v = max(v, mic_dpp<0x114>(0u, v)); v = max(v, mic_dpp<0x118>(0u, v));
    v = max(v, mic_dpp<0x142, 0xA>(0u, v)); v = max(v, mic_dpp<0x143, 0xC>(0u, v));
    return v;
}

// A value that is the same in every lane, said so to the compiler: it moves to scalar registers.
__device__ __forceinline__ uint32_t mic_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t mic_uniform(uint64_t v) { return (uint64_t)mic_uniform((uint32_t)v) | ((uint64_t)mic_uniform((uint32_t)(v >> 32)) << 32); }

// The value of the lane d below (lanes 0 .. d-1: their own), 32 or 64 bits.
__device__ __forceinline__ uint32_t mic_lane_up(uint32_t v, int d) { return (uint32_t)__shfl_up((int)v, d); }
__device__ __forceinline__ uint64_t mic_lane_up(uint64_t v, int d) { return (uint64_t)__shfl_up((long long)v, d); }
// Wave-wide inclusive scan of any associative op(earlier, later) -- it need not commute -- over 32- or 64-bit values.
template <class T, class Op>
__device__ __forceinline__ T mic_wave_incl_scan(T v, uint32_t lane, Op op) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const T o = mic_lane_up(v, d); if (lane >= (uint32_t)d) v = op(o, v); }
    return v;
}
// What the lane below holds; lane 0 takes `first`.
__device__ __forceinline__ uint32_t mic_wave_prev(uint32_t v, uint32_t lane, uint32_t first) {
    const uint32_t p = mic_lane_up(v, 1);
    return lane == 0 ? first : p;
}

// Wave-wide reductions (xor butterfly): every lane returns the result.
__device__ __forceinline__ uint32_t mic_lane_xor(uint32_t v, int d) { return (uint32_t)__shfl_xor((int)v, d); }
__device__ __forceinline__ uint64_t mic_lane_xor(uint64_t v, int d) { return (uint64_t)__shfl_xor((long long)v, d); }
template <class T, class Op>
__device__ __forceinline__ T mic_wave_reduce(T v, Op op) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = op(v, mic_lane_xor(v, d));
    return v;
}
__device__ __forceinline__ uint32_t mic_wave_reduce_add(uint32_t v) { return mic_wave_reduce(v, [](uint32_t a, uint32_t b) { return a + b; }); }
__device__ __forceinline__ uint64_t mic_wave_reduce_add(uint64_t v) { return mic_wave_reduce(v, [](uint64_t a, uint64_t b) { return a + b; }); }
__device__ __forceinline__ uint32_t mic_wave_reduce_min(uint32_t v) { return mic_wave_reduce(v, [](uint32_t a, uint32_t b) { return min(a, b); }); }
__device__ __forceinline__ uint32_t mic_wave_reduce_max(uint32_t v) { return mic_wave_reduce(v, [](uint32_t a, uint32_t b) { return max(a, b); }); }
__device__ __forceinline__ uint64_t mic_wave_reduce_max(uint64_t v) { return mic_wave_reduce(v, [](uint64_t a, uint64_t b) { return a > b ? a : b; }); }

// Work-group exclusive scans of one value per thread, WAVES waves: lane 63 of every wave stores its inclusive value, a barrier,
// every thread combines the partials of the waves before its own.  Returns the exclusive prefix; *total = the whole group's.
// s_tmp: WAVES words of LDS.  ONE barrier inside, between the stores of the partials and their reads; the function neither
// begins nor ends on one, so a caller that uses s_tmp again (or has just read it) puts its own barrier in between.
template <int WAVES>
__device__ __forceinline__ uint32_t mic_group_excl_add(uint32_t v, uint32_t *s_tmp, uint32_t *total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = mic_wave_incl_add(v);
    if (lane == 63) s_tmp[wave] = incl;
    __syncthreads();
    uint32_t off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) { const uint32_t x = s_tmp[w]; if ((uint32_t)w < wave) off += x; tot += x; }
    *total = tot;
    return off + incl - v;
}
// (unsigned maximum, identity 0)
template <int WAVES>
__device__ __forceinline__ uint32_t mic_group_excl_max(uint32_t v, uint32_t *s_tmp, uint32_t *total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = mic_wave_incl_max(v);
    uint32_t ex = mic_dpp<0x138>(0u, incl);                              // the lane below; lane 0: the identity
    if (lane == 63) s_tmp[wave] = incl;
    __syncthreads();
    uint32_t tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) { const uint32_t x = s_tmp[w]; if ((uint32_t)w < wave) ex = max(ex, x); tot = max(tot, x); }
    *total = tot;
    return ex;
}

// The escape-marker recurrence of a symbol stream: a symbol equal to the delimiter is a marker unless it is itself the payload of
// one, marker[i] = isDelim[i] & !marker[i-1]; every symbol that is not a marker is a pixel.  A stretch of symbols is the function
// entry state (0 / 1: the symbol in front was a marker) -> (exit state, pixels in the stretch), packed into one word:
// bit 0 / 1 the exit state for entry 0 / 1, CB bits of pixel count for entry 0 from bit 2 and for entry 1 from bit 2 + CB.
// (k_dec_pixels_wg: CB = 14, counts at bits 2 and 16; k_dec_rows_tok: CB = 15, counts at bits 2 and 17.)
template <int CB>
struct MicMarkerFn {
    static constexpr uint32_t SH1 = 2 + CB, CMASK = (1u << CB) - 1u;
    static constexpr uint32_t identity = 2u;                             // state 0 -> 0, 1 -> 1, no pixels
    uint32_t s0 = 0, s1 = 1, c0 = 0, c1 = 0;
    // one symbol more: d = it equals the delimiter, in = it is part of the stream at all (d implies in; a position that is not
    // leaves state and count as they are)
    __device__ __forceinline__ void step(uint32_t d, uint32_t in) {
        const uint32_t m0 = d & (s0 ^ 1u), m1 = d & (s1 ^ 1u);
        c0 += in & (m0 ^ 1u); c1 += in & (m1 ^ 1u);
        s0 = in ? m0 : s0; s1 = in ? m1 : s1;
    }
    __device__ __forceinline__ uint32_t pack() const { return s0 | (s1 << 1) | (c0 << 2) | (c1 << SH1); }
    static __device__ __forceinline__ uint32_t state(uint32_t f, uint32_t entry) { return (f >> entry) & 1u; }
    static __device__ __forceinline__ uint32_t count(uint32_t f, uint32_t entry) { return entry ? f >> SH1 : (f >> 2) & CMASK; }
    static __device__ __forceinline__ uint32_t compose(uint32_t a, uint32_t b) {      // a then b
        const uint32_t a0 = a & 1u, a1 = (a >> 1) & 1u;
        const uint32_t c0 = count(a, 0) + count(b, a0), c1 = count(a, 1) + count(b, a1);
        return state(b, a0) | (state(b, a1) << 1) | (c0 << 2) | (c1 << SH1);
    }
};

// Row 0 of a frame under the inverse Delta(avg) predictor, by one wave: out[x] = raw ? sym : out[x-1] + sym - thr, out[-1] = 0.
// px: the row's W symbols; flags: bit x set = pixel x is stored raw; row16: the wave's LDS row buffer, `padded` >= W entries of
// which are written (pixels behind W as 0).  A lane takes (W + 63) / 64 consecutive columns: a first pass makes its (reset, sum)
// pair, an inclusive scan of the composition (a then b) = b.reset ? b : (a.reset, a.sum + b.sum) gives every lane its left
// neighbour, a second pass writes the pixels.  Wave-private LDS: no barrier, the waits order the lane's own reads and writes.
template <class PxPtr, class FlagPtr>
__device__ __forceinline__ void pr_row0_scan(uint16_t *row16, PxPtr px, FlagPtr flags, int W, int padded, uint32_t thr, uint32_t lane) {
    for (int x = (int)lane; x < padded; x += 64) row16[x] = (x < W) ? px[x] : (uint16_t)0;
    __builtin_amdgcn_s_waitcnt(0xC07F);                              // wave-private LDS: writes above land before the reads below
    const int cw = (W + 63) >> 6;
    const int x0 = min(W, (int)lane * cw), x1 = min(W, x0 + cw);
    uint32_t rs = 0, sum = 0;
    for (int x = x0; x < x1; x++) {
        const uint32_t raw = (flags[x >> 5] >> (x & 31)) & 1u, v = row16[x];
        if (raw) { rs = 1; sum = v; } else sum = (sum + v - thr) & 0xFFFFu;
    }
    // the pair as one word: the sum in bits 0..15, the reset in bit 16
    const uint32_t incl = mic_wave_incl_scan(sum | (rs << 16), lane, [](uint32_t a, uint32_t b) {
        return (b >> 16) ? b : ((a & 0x10000u) | ((a + b) & 0xFFFFu));
    });
    uint32_t cur = mic_wave_prev(incl, lane, 0u) & 0xFFFFu;
    for (int x = x0; x < x1; x++) {
        const uint32_t raw = (flags[x >> 5] >> (x & 31)) & 1u, v = row16[x];
        cur = raw ? v : ((cur + v - thr) & 0xFFFFu);
        row16[x] = (uint16_t)cur;
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);                              // wave-private LDS: writes above land before the reads below
}
