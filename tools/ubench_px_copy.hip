// ubench_px_copy.hip -- the two forms of the native RGB gather out of the tile cache's pixel slots (csrc/mic_px_copy.h), timed one
// against the other on the same pieces: 512 random 256 x 256 patches of an 8192 x 8192 slide whose 1024 tiles of 256 x 256 lie in
// slots of 3 bytes a pixel -- about 100 MB read and 100 MB written.  Every source residue meets every destination residue: tile
// columns and patch origins are arbitrary and a pixel is three bytes.  Also a 255-pixel patch width (odd rows in the tensor).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I medical-image-codec_amd/csrc tools/ubench_px_copy.hip -o tools/ubench_px_copy
//   tools/ubench_px_copy            -> one JSON line: min of 10 launches of each form, per patch width
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "mic_px_copy.h"

#define CHECK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(_e)); return 1; } } while (0)

template <bool DWORDS>
__global__ void __launch_bounds__(256) k_copy(const uint8_t *arena, const GatherPiece *pieces, uint8_t *out) {
    const GatherPiece pc = pieces[blockIdx.x];
    const int nb = pc.w * 3;
    const PieceLanes ln = DWORDS ? px_row_lanes(nb) : piece_lanes(pc.w);
    const uint8_t *src = arena + pc.src;
    uint8_t *dst = out + pc.dst * 3;
    for (int y = ln.row; y < pc.h; y += ln.rstep) {
        const mic_gp<const uint8_t> s = mic_g(src + (size_t)y * pc.sstride * 3);
        const mic_gp<uint8_t> d = mic_g(dst + (size_t)y * pc.dstride * 3);
        if (DWORDS) px_row_dwords(s, d, nb, ln); else px_row_plain<3>(s, d, pc.w, ln);
    }
}

int main() {
    const int T = 256, TX = 32, N = 512, RUNS = 10;
    const size_t slot = (size_t)T * T * 3, arena_bytes = slot * TX * TX;
    uint8_t *arena = nullptr, *out[2] = { nullptr, nullptr };
    CHECK(hipMalloc(&arena, arena_bytes));
    std::vector<uint8_t> h(arena_bytes);
    std::mt19937 rng(3);
    for (size_t i = 0; i < arena_bytes; i += 4) { const uint32_t v = rng(); memcpy(&h[i], &v, 4); }
    CHECK(hipMemcpy(arena, h.data(), arena_bytes, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    printf("{\"patches\": %d", N);
    for (int pw : { 256, 255 }) {
        const int ph = 256;
        std::vector<GatherPiece> pcs;
        int mw = 1, mh = 1;
        for (int i = 0; i < N; i++) {
            const int px = (int)(rng() % (unsigned)(T * TX - pw)), py = (int)(rng() % (unsigned)(T * TX - ph));
            for (int ty = py / T; ty <= (py + ph - 1) / T; ty++) for (int tx = px / T; tx <= (px + pw - 1) / T; tx++) {
                const int ax = std::max(px, tx * T), bx = std::min(px + pw, (tx + 1) * T), ay = std::max(py, ty * T), by = std::min(py + ph, (ty + 1) * T);
                pcs.push_back(GatherPiece{ (uint64_t)(ty * TX + tx) * slot + ((uint64_t)(ay - ty * T) * T + (uint64_t)(ax - tx * T)) * 3,
                                           ((uint64_t)i * ph + (uint64_t)(ay - py)) * pw + (uint64_t)(ax - px), T, pw, bx - ax, by - ay, 0, 0 });
                mw = std::max(mw, bx - ax); mh = std::max(mh, by - ay);
            }
        }
        const size_t out_bytes = (size_t)N * ph * pw * 3;
        for (int k = 0; k < 2; k++) { if (out[k]) CHECK(hipFree(out[k])); CHECK(hipMalloc(&out[k], out_bytes + 64)); CHECK(hipMemset(out[k], 0, out_bytes + 64)); }
        GatherPiece *d_pcs = nullptr;
        CHECK(hipMalloc(&d_pcs, pcs.size() * sizeof(GatherPiece)));
        CHECK(hipMemcpy(d_pcs, pcs.data(), pcs.size() * sizeof(GatherPiece), hipMemcpyHostToDevice));
        const dim3 grid((unsigned)pcs.size(), row_chunks(mw, mh)), block(256);
        float best[2] = { 1e30f, 1e30f };
        for (int r = 0; r < RUNS + 1; r++)
            for (int k = 0; k < 2; k++) {
                CHECK(hipEventRecord(e0, 0));
                if (k == 0) hipLaunchKernelGGL(k_copy<true>, grid, block, 0, 0, arena, d_pcs, out[0]);
                else hipLaunchKernelGGL(k_copy<false>, grid, block, 0, 0, arena, d_pcs, out[1]);
                CHECK(hipEventRecord(e1, 0));
                CHECK(hipEventSynchronize(e1));
                CHECK(hipGetLastError());
                float ms = 0;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                if (r > 0) best[k] = std::min(best[k], ms);
            }
        std::vector<uint8_t> a(out_bytes), b(out_bytes);
        CHECK(hipMemcpy(a.data(), out[0], out_bytes, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(b.data(), out[1], out_bytes, hipMemcpyDeviceToHost));
        const bool same = a == b;
        printf(", \"pw%d\": {\"pieces\": %zu, \"bytes\": %zu, \"dwords_ms\": %.4f, \"plain_ms\": %.4f, \"equal\": %s}", pw, pcs.size(), out_bytes, best[0], best[1], same ? "true" : "false");
        CHECK(hipFree(d_pcs));
        if (!same) { printf("}\n"); return 2; }
    }
    printf("}\n");
    return 0;
}
