// mic_px_copy.h -- a row of nb bytes from s to d, both global and at ANY byte alignment, by the lanes of a piece (piece_lanes):
// what the native gathers out of the tile cache's pixel slots are made of (mic_gather.hip).  3-byte pixels and odd patch widths
// make every residue of source and destination occur.  Two forms, kept side by side so that tools/ubench_px_copy.hip can time
// one against the other on the same pieces:
//   px_row_dwords: bytes up to the destination's dword alignment, then whole dwords -- each assembled from two aligned source dwords
//                  when the source is skewed against the destination (v_alignbyte_b32) --, then the tail bytes;
//   px_row_plain:  a lane per pixel, its BPP bytes one by one: the plain loop, gather_rgb_native's three byte stores per lane.
// The second aligned dword a skewed lane reads holds a byte of the row's last dword, so it lies inside the allocation the row is in.
#pragma once
#include "mic_dev.h"
#include "mic_pieces.h"

// lanes of a row of nb bytes moved as dwords: four at least, one for each of the up to three bytes in front of and behind them
__device__ __forceinline__ PieceLanes px_row_lanes(int nb) { return piece_lanes(max(4, (nb + 3) >> 2)); }

__device__ __forceinline__ void px_row_dwords(mic_gp<const uint8_t> s, mic_gp<uint8_t> d, int nb, const PieceLanes &ln) {
    const int head = min(nb, (int)(-(intptr_t)(size_t)d & 3));
    const int nd = (nb - head) >> 2, tail = nb - head - 4 * nd;
    if (ln.col < head) d[ln.col] = s[ln.col];
    const mic_gp<uint32_t> d4 = (mic_gp<uint32_t>)(d + head);
    const size_t sa = (size_t)(s + head);
    const uint32_t skew = (uint32_t)(sa & 3);
    const mic_gp<const uint32_t> s4 = (mic_gp<const uint32_t>)(sa - skew);
    if (skew == 0)
        for (int x = ln.col; x < nd; x += ln.lw) d4[x] = s4[x];
    else
        for (int x = ln.col; x < nd; x += ln.lw) d4[x] = __builtin_amdgcn_alignbyte(s4[x + 1], s4[x], skew);
    const int t0 = head + 4 * nd;
    if (ln.col < tail) d[t0 + ln.col] = s[t0 + ln.col];
}

// (ln: piece_lanes(w), w the row's pixels)
template <int BPP>
__device__ __forceinline__ void px_row_plain(mic_gp<const uint8_t> s, mic_gp<uint8_t> d, int w, const PieceLanes &ln) {
    for (int x = ln.col; x < w; x += ln.lw) {
#pragma unroll
        for (int k = 0; k < BPP; k++) d[x * BPP + k] = s[x * BPP + k];
    }
}
