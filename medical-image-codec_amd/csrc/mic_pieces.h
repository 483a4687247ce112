// mic_pieces.h -- helpers shared by the gather kernels (MIC3 patches, MIC2 crops, strip-file crops) and the MIC2 temporal pipeline.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

__device__ __forceinline__ uint32_t zigzag16(int32_t v) { const uint32_t x = (uint32_t)v & 0xFFFFu; return ((x << 1) ^ ((x & 0x8000u) ? 0xFFFFu : 0u)) & 0xFFFFu; }   // deltazigzagcompressu16.go:108-111
__device__ __forceinline__ uint32_t unzigzag16(uint32_t u) { return ((u >> 1) ^ ((u & 1u) ? 0xFFFFu : 0u)) & 0xFFFFu; }                                            // :113-116

// Lanes run along x of a piece row.  A piece narrower than a wave puts 64 / lw of its rows side by side in one (lw: the power of
// two >= w, at most 64), so a 17-pixel overlap keeps 32 + 17 lanes of 64 busy instead of 17.  grid = (pieces, row chunks).
struct PieceLanes { int col, lw, row, rstep; };
__device__ __forceinline__ PieceLanes piece_lanes(int w) {
    const int sh = min(6, 32 - __clz(w - 1));                                       // (w >= 1; __clz(0) = 32: one lane per row)
    return PieceLanes{ (int)threadIdx.x & ((1 << sh) - 1), 1 << sh, (int)(threadIdx.x >> sh) + (int)blockIdx.y * (256 >> sh), (256 >> sh) * (int)gridDim.y };
}
// rows of a piece per block pass = 256 / lanes per row; grid y cuts pieces of more than 16 passes (w, h: the largest piece of the launch)
inline unsigned row_chunks(int w, int h) {
    int lw = 1;
    while (lw < w && lw < 64) lw *= 2;
    const int passes = (h + 256 / lw - 1) / (256 / lw) * ((w + 63) / 64);
    return (unsigned)std::min(16, std::max(1, passes / 16));
}
