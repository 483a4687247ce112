// mic_verify.hip -- k_units_digest: the CRC-32 of every unit of a batch and, beside it, the compare of the unit's pixels with a second
// copy (the decode of the streams that were just packed), in ONE launch over fixed-size chunks of all units; k_units_digest_fold:
// one wave per unit joins the chunks' registers in order and takes the unit's last bytes.  No atomics touch the CRC: the result is
// the same call after call by construction.  The identities and the geometry: mic_verify.h.
#include "mic_verify.h"
#include "mic_launch.h"
#include "mic_wave.h"

namespace {

// Slicing-by-8: t[k][b] = the raw register of byte b followed by k zero bytes.  Computed by the compiler; a work-group copies the
// 8 KiB into LDS at its start (building them there would cost more than the chunk: ~2000 shift/xor steps a thread).
struct CrcTables { uint32_t t[8][256]; };
constexpr CrcTables make_crc_tables() {
    CrcTables T{};
    for (uint32_t b = 0; b < 256; b++) {
        uint32_t r = b;
        for (int k = 0; k < 8; k++) r = (r >> 1) ^ (MIC_CRC_POLY & (0u - (r & 1u)));
        T.t[0][b] = r;
    }
    for (int k = 1; k < 8; k++)
        for (uint32_t b = 0; b < 256; b++) T.t[k][b] = (T.t[k - 1][b] >> 8) ^ T.t[0][T.t[k - 1][b] & 0xFFu];
    return T;
}
__device__ const CrcTables g_crc_tables = make_crc_tables();

constexpr uint32_t kLaneWords = MIC_VFY_LANE_BYTES / 16;          // 16-byte words of a lane's run

// The pixel pointers come out of a record in memory, where the compiler no longer knows that they are global addresses and would
// use flat loads: these say so.
#define MIC_GLOBAL __attribute__((address_space(1)))
typedef uint32_t word_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 load_word(const void *p) {
    const word_t v = *(const MIC_GLOBAL word_t *)(uintptr_t)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint32_t load_px(const uint16_t *p) { return *(const MIC_GLOBAL uint16_t *)(uintptr_t)p; }

// eight more bytes (lo first) into a register
__device__ __forceinline__ uint32_t crc_step8(const uint32_t (*tab)[256], uint32_t reg, uint32_t lo, uint32_t hi) {
    lo ^= reg;
    return tab[7][lo & 0xFFu] ^ tab[6][(lo >> 8) & 0xFFu] ^ tab[5][(lo >> 16) & 0xFFu] ^ tab[4][lo >> 24] ^
           tab[3][hi & 0xFFu] ^ tab[2][(hi >> 8) & 0xFFu] ^ tab[1][(hi >> 16) & 0xFFu] ^ tab[0][hi >> 24];
}
__device__ __forceinline__ uint32_t crc_word(const uint32_t (*tab)[256], uint32_t reg, const uint4 &w) {
    return crc_step8(tab, crc_step8(tab, reg, w.x, w.y), w.z, w.w);
}
// the samples of a 16-byte word that differ, word at pixel index px0 of its unit (px0 may be negative for a unit's first word: those
// samples are zero in both copies)
__device__ __forceinline__ void diff_word(const uint4 &r, const uint4 &d, int64_t px0, uint32_t &count, uint32_t &first) {
    const uint32_t x[4] = { r.x ^ d.x, r.y ^ d.y, r.z ^ d.z, r.w ^ d.w };
    if ((x[0] | x[1] | x[2] | x[3]) == 0) return;
#pragma unroll
    for (int k = 3; k >= 0; k--) {                                  // (downwards: `first` ends as the smallest)
        if (x[k] >> 16) { count++; first = (uint32_t)(px0 + 2 * k + 1); }
        if (x[k] & 0xFFFFu) { count++; first = (uint32_t)(px0 + 2 * k); }
    }
}
// The word that holds a unit's first sample when the unit does not start on a 16-byte boundary: sample i of the word is pixel
// px0 + i, read one by one from pixel 0 on, zero in front of it.  Nothing outside the unit is touched.
__device__ __forceinline__ uint4 load_word_head(const uint16_t *base, int64_t px0) {
    uint32_t h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = (px0 + i >= 0) ? load_px(base + px0 + i) : 0u;
    return make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

template <bool COMPARE>
__global__ __launch_bounds__(MIC_VFY_THREADS) void k_units_digest(const MicVerifyUnit *__restrict__ units, const uint32_t *__restrict__ chunk_unit,
                                                                   MicVerifyConsts C, uint32_t *__restrict__ partial,
                                                                   unsigned long long *__restrict__ mism, unsigned long long *__restrict__ first_out) {
    __shared__ uint32_t s_tab[8][256];
    __shared__ uint32_t s_wave[MIC_VFY_THREADS / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    {
        const uint4 *src = (const uint4 *)&g_crc_tables.t[0][0];
        uint4 *dst = (uint4 *)&s_tab[0][0];
        for (uint32_t i = t; i < 8u * 256u / 4u; i += MIC_VFY_THREADS) dst[i] = src[i];
    }
    const uint32_t c = blockIdx.x, ui = chunk_unit[c];
    const MicVerifyUnit U = units[ui];
    // The body ends at the last 16-byte boundary inside the unit; chunk k of the unit's nchunks ends (nchunks - 1 - k) chunks in
    // front of it.  Everything below is in bytes from the unit's first one: off < 0 is in front of the unit.
    const uint64_t base = (uint64_t)(uintptr_t)U.ref;
    const int64_t body = (int64_t)(((base + 2 * U.npx) & ~(uint64_t)15) - base);
    const int64_t run0 = body - (int64_t)(U.nchunks - (c - U.chunk0)) * (int64_t)MIC_VFY_CHUNK_BYTES + (int64_t)t * (int64_t)MIC_VFY_LANE_BYTES;
    const bool compare = COMPARE && U.dec != nullptr;
    __syncthreads();

    uint32_t reg = 0, count = 0, first = ~0u;
    if (run0 >= 0) {                                               // the whole run lies inside the unit, on 16-byte boundaries
        const char *rp = (const char *)U.ref + run0;
        uint4 r[kLaneWords];
#pragma unroll
        for (uint32_t j = 0; j < kLaneWords; j++) r[j] = load_word(rp + 16 * j);
        if (compare) {
            const uint16_t *dp = U.dec + run0 / 2;
            uint4 d[kLaneWords];
#pragma unroll
            for (uint32_t j = 0; j < kLaneWords; j++) d[j] = load_word(dp + 8 * j);
#pragma unroll
            for (int j = (int)kLaneWords - 1; j >= 0; j--) diff_word(r[j], d[j], run0 / 2 + 8 * j, count, first);
        }
#pragma unroll
        for (uint32_t j = 0; j < kLaneWords; j++) reg = crc_word(s_tab, reg, r[j]);
    } else if (run0 + (int64_t)MIC_VFY_LANE_BYTES > 0) {           // the run that holds the unit's first byte (the head, peeled)
        for (int j = (int)kLaneWords - 1; j >= 0; j--) {           // (compare downwards, as above)
            const int64_t off = run0 + 16 * j;
            if (!compare || off + 16 <= 0) continue;
            const uint4 r = off >= 0 ? load_word((const char *)U.ref + off) : load_word_head(U.ref, off / 2);
            const uint4 d = off >= 0 ? load_word(U.dec + off / 2) : load_word_head(U.dec, off / 2);
            diff_word(r, d, off / 2, count, first);
        }
        for (uint32_t j = 0; j < kLaneWords; j++) {
            const int64_t off = run0 + 16 * (int64_t)j;
            if (off + 16 <= 0) continue;                           // (in front of the unit: zero bytes into a zero register)
            const uint4 r = off >= 0 ? load_word((const char *)U.ref + off) : load_word_head(U.ref, off / 2);
            reg = crc_word(s_tab, reg, r);
        }
    }                                                              // else: a run in front of the unit, register 0

    if (COMPARE && __ballot(count != 0)) {                         // only a wave that saw a difference touches the unit's record
        const uint32_t wc = mic_wave_reduce_add(count), wf = mic_wave_reduce_min(first);
        if (lane == 0) {
            atomicAdd(&mism[ui], (unsigned long long)wc);
            atomicMin(&first_out[ui], (unsigned long long)wf);
        }
    }
    // lanes to a wave: blocks of 2^k lanes join, the earlier block times x^(8 * bytes of the later one)
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const uint32_t other = mic_lane_xor(reg, 1 << k);
        const bool upper = (lane >> k) & 1u;
        reg = mic_crc_mul(upper ? other : reg, C.lane[k]) ^ (upper ? reg : other);
    }
    if (lane == 0) s_wave[wave] = reg;
    __syncthreads();
    if (t == 0) {
        uint32_t g = s_wave[0];
        for (uint32_t w = 1; w < MIC_VFY_THREADS / 64; w++) g = mic_crc_mul(g, C.wave) ^ s_wave[w];
        partial[c] = g;
    }
}

// One wave per unit: the chunks' registers in order, then the bytes behind the body's last 16-byte boundary (up to seven samples),
// hashed and compared one by one.  The records' atomics are complete (a kernel boundary lies in between).
__global__ __launch_bounds__(64) void k_units_digest_fold(const MicVerifyUnit *__restrict__ units, int n, MicVerifyConsts C, const uint32_t *__restrict__ partial,
                                                         int compare_all, uint32_t *__restrict__ reg_out, unsigned long long *__restrict__ mism,
                                                         unsigned long long *__restrict__ first_out) {
    const int ui = (int)blockIdx.x;
    if (ui >= n || threadIdx.x != 0) return;
    const MicVerifyUnit U = units[ui];
    uint32_t reg = 0;
    for (uint32_t k = 0; k < U.nchunks; k++) reg = mic_crc_mul(reg, C.chunk) ^ partial[U.chunk0 + k];
    const uint64_t base = (uint64_t)(uintptr_t)U.ref;
    const int64_t body = (int64_t)(((base + 2 * U.npx) & ~(uint64_t)15) - base);
    const bool compare = compare_all && U.dec != nullptr;
    unsigned long long cnt = 0, first = ~0ull;
    for (uint64_t p = body > 0 ? (uint64_t)body / 2 : 0; p < U.npx; p++) {
        const uint32_t v = load_px(U.ref + p);
        reg = mic_crc_byte(mic_crc_byte(reg, v & 0xFFu), v >> 8);
        if (compare && load_px(U.dec + p) != v) { cnt++; if (first == ~0ull) first = p; }
    }
    reg_out[ui] = reg;
    if (cnt) {
        mism[ui] += cnt;
        if (first_out[ui] == ~0ull) first_out[ui] = first;         // (every index of the body is smaller)
    }
}

}  // namespace

void mic_launch_units_digest(const MicVerifyUnit *d_units, int n, const uint32_t *d_chunk_unit, uint32_t nchunks, bool compare,
                             uint32_t *d_partial, uint32_t *d_reg, unsigned long long *d_mism, unsigned long long *d_first,
                             hipStream_t stream, MicTimer *t) {
    static const MicVerifyConsts C = [] {
        MicVerifyConsts c;
        for (int k = 0; k < 6; k++) c.lane[k] = mic_crc_xpow8((uint64_t)MIC_VFY_LANE_BYTES << k);
        c.wave = mic_crc_xpow8(MIC_VFY_WAVE_BYTES);
        c.chunk = mic_crc_xpow8(MIC_VFY_CHUNK_BYTES);
        return c;
    }();
    if (nchunks) {
        if (t) t->mark(compare ? "k_units_digest<compare>" : "k_units_digest");
        if (compare) hipLaunchKernelGGL(k_units_digest<true>, dim3(nchunks), dim3(MIC_VFY_THREADS), 0, stream, d_units, d_chunk_unit, C, d_partial, d_mism, d_first);
        else hipLaunchKernelGGL(k_units_digest<false>, dim3(nchunks), dim3(MIC_VFY_THREADS), 0, stream, d_units, d_chunk_unit, C, d_partial, d_mism, d_first);
    }
    if (t) t->mark("k_units_digest_fold");
    hipLaunchKernelGGL(k_units_digest_fold, dim3(n), dim3(64), 0, stream, d_units, n, C, d_partial, compare ? 1 : 0, d_reg, d_mism, d_first);
    if (t) t->mark("end");
}
