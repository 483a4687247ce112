// mic_verify.h -- CRC-32 digests and pixel compares of units on the device (mic_verify.hip), and the CRC arithmetic the host shares
// with the kernels.
//
// The CRC is the IEEE one (zlib's crc32, Go's hash/crc32.ChecksumIEEE): reflected polynomial 0xEDB88320, init and final xor
// 0xFFFFFFFF, over a unit's pixels as little-endian u16 bytes in row-major order.  In the reflected register bit 31 is x^0 and a
// multiplication by x is a shift to the right; "raw register" below is the register of a message hashed from a ZERO start without
// the final xor.  Two identities carry everything:
//   raw(A || B) = raw(A) * x^(8 |B|) mod P  xor  raw(B)           (so leading zero bytes change nothing)
//   crc(M)      = raw(M)  xor  0xFFFFFFFF * x^(8 |M|) mod P  xor  0xFFFFFFFF
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#define MIC_CRC_POLY 0xEDB88320u

// a * b mod P, both in the reflected representation (a's bits are walked from x^0 up)
__host__ __device__ inline uint32_t mic_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll
    for (int k = 31; k >= 0; k--) {
        p ^= b & (0u - ((a >> k) & 1u));
        b = (b >> 1) ^ (MIC_CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}
// x^(8 n) mod P: what n more bytes multiply a register by (square and multiply over the bits of n)
inline uint32_t mic_crc_xpow8(uint64_t nbytes) {
    uint32_t sq = 0x00800000u;                          // x^8
    uint32_t p = 0x80000000u;                           // x^0
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1) p = mic_crc_mul(sq, p);
        sq = mic_crc_mul(sq, sq);
    }
    return p;
}
// one byte into a register, bit by bit (tails of a few bytes; the kernels' bodies go through tables)
__host__ __device__ inline uint32_t mic_crc_byte(uint32_t reg, uint32_t byte) {
    reg ^= byte;
#pragma unroll
    for (int k = 0; k < 8; k++) reg = (reg >> 1) ^ (MIC_CRC_POLY & (0u - (reg & 1u)));
    return reg;
}

// ---- the digest kernels' geometry: a lane hashes a contiguous run of MIC_VFY_LANE_BYTES, a wave 64 of them, a work-group of
// MIC_VFY_THREADS threads one CHUNK.  A unit's body -- its bytes up to the last 16-byte boundary of the address space inside it --
// is cut into chunks from that END backwards, so every run starts on a 16-byte boundary and only a unit's first chunk is short; the
// up to 14 bytes behind the boundary are the fold kernel's.
#define MIC_VFY_LANE_BYTES 128u
#define MIC_VFY_THREADS 256u
#define MIC_VFY_WAVE_BYTES (64u * MIC_VFY_LANE_BYTES)
#define MIC_VFY_CHUNK_BYTES (MIC_VFY_THREADS * MIC_VFY_LANE_BYTES)

struct MicVerifyUnit {
    const uint16_t *ref;            // the pixels that are hashed
    const uint16_t *dec;            // the pixels they are compared with (null: this unit is hashed only); the same address as ref modulo 16:
                                    // the library lays the second copy out itself, and one set of 16-byte boundaries then serves both
    uint64_t npx;
    uint32_t chunk0, nchunks;       // the unit's chunks in the launch's flat grid: chunk0 .. chunk0 + nchunks - 1 (none: a body-less unit)
};
// multipliers of the folds, computed once on the host: lane[k] = x^(8 * LANE_BYTES * 2^k) joins blocks of 2^k lanes, wave joins
// waves, chunk joins chunks
struct MicVerifyConsts { uint32_t lane[6]; uint32_t wave, chunk; };

// d_chunk_unit[c]: the unit of chunk c; d_partial[c]: its raw register; per unit: d_reg (raw register of all its bytes), d_mism
// (differing samples), d_first (smallest differing pixel index, ~0: none).  d_mism is zero and d_first all ones on entry.
void mic_launch_units_digest(const MicVerifyUnit *d_units, int n, const uint32_t *d_chunk_unit, uint32_t nchunks, bool compare,
                             uint32_t *d_partial, uint32_t *d_reg, unsigned long long *d_mism, unsigned long long *d_first,
                             hipStream_t stream, struct MicTimer *t);
