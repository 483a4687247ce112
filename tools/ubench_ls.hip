// ubench_ls.hip -- where a round of the lane-per-state tANS decoder (csrc/mic_decode_ls.hip, N = 2) spends its cycles on gfx950.
// Build: hipcc --offload-arch=gfx950 -O3 -o ubench_ls ubench_ls.hip ; run on the GPU box.  Prints shader cycles per round
// (s_memtime, median over waves) for the shipped round and for ablations of it; the values decoded are meaningless.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

#define STREAM_BYTES 17680u
#define TAB 1296u
#define STAGE 1040u

// V: 0 shipped round | 1 no stage store | 2 plain VALU instead of DPP | 3 no window reads | 4 bare chain (entry -> state -> entry)
//    6 s_waitcnt only once per round (entry and window together)
template <int V>
__global__ void __launch_bounds__(192) k_round(const uint16_t *tab, uint32_t *out, int chunks, unsigned long long *cyc) {
    extern __shared__ uint32_t s_mem[];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t g = lane / 2; if (g >= 3) g = 0;
    const uint32_t k = lane & 1;
    const uint32_t sbase = (wv * 3 + g) * STREAM_BYTES;
    for (uint32_t j = 0; j < 3; j++) {
        const uint32_t tb = ((wv * 3 + j) * STREAM_BYTES + TAB) >> 2;
        for (uint32_t i = lane; i < 4096; i += 64) s_mem[tb + i] = ((const uint32_t *)tab)[i];
        const uint32_t rb = ((wv * 3 + j) * STREAM_BYTES) >> 2;
        for (uint32_t i = lane; i < 260; i += 64) s_mem[rb + i] = 0x9E3779B9u * (i + 1 + j);
    }
    __syncthreads();
    const uint32_t cb = sbase + TAB - 2u * 8192u, C = 31u - 13u, ringb = sbase, stgb = sbase + STAGE + 2u * k;
    const uint32_t mk1 = k ? ~0u : 0u;
    uint32_t st = 8192u + ((out[0] + 17u * lane) & 8191u), q = 1u << 20;
    uint32_t e, w0, w1, c, nb, m, hi, pre, at;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int ch = 0; ch < chunks; ch++) {
        asm volatile(
            ".set ls_off, 0\n\t"
            "v_lshl_add_u32 %[at], %[st], 1, %[cb]\n\tds_read_u16 %[e], %[at]\n\t"
            "v_bfe_u32 %[at], %[q], 5, 8\n\tv_lshl_add_u32 %[at], %[at], 2, %[ringb]\n\t"
            ".if %[V] != 3 && %[V] != 4\n\tds_read_b32 %[w0], %[at]\n\tds_read_b32 %[w1], %[at] offset:4\n\t.endif\n\t"
            ".rept 64\n\t"
            ".if %[V] == 3 || %[V] == 4\n\ts_waitcnt lgkmcnt(0)\n\t.elseif %[V] == 6\n\ts_waitcnt lgkmcnt(0)\n\t.else\n\ts_waitcnt lgkmcnt(2)\n\t.endif\n\t"
            ".if %[V] != 1 && %[V] != 4\n\tds_write_b16 %[stg], %[st] offset:ls_off\n\t.endif\n\t"
            ".set ls_off, ls_off+4\n\t"
            "v_ffbh_u32 %[c], %[e]\n\t"
            "v_sub_u32 %[nb], %[c], %[C]\n\t"
            "v_sub_u32 %[m], %[C], %[c]\n\t"
            ".if %[V] == 4\n\t"
            "v_alignbit_b32 %[st], %[e], %[q], %[m]\n\t"
            "v_lshl_add_u32 %[at], %[st], 1, %[cb]\n\tds_read_u16 %[e], %[at]\n\t"
            ".else\n\t"
            ".if %[V] == 3 || %[V] == 6\n\tv_alignbit_b32 %[hi], %[w1], %[w0], %[q]\n\t"
            ".else\n\ts_waitcnt lgkmcnt(1)\n\tv_alignbit_b32 %[hi], %[w1], %[w0], %[q]\n\t.endif\n\t"
            ".if %[V] == 2\n\tv_and_b32 %[pre], %[nb], %[mk1]\n\t"
            ".else\n\tv_and_b32_dpp %[pre], %[nb], %[mk1] quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t.endif\n\t"
            "v_lshlrev_b32 %[hi], %[pre], %[hi]\n\t"
            "v_alignbit_b32 %[st], %[e], %[hi], %[m]\n\t"
            "v_lshl_add_u32 %[at], %[st], 1, %[cb]\n\tds_read_u16 %[e], %[at]\n\t"
            ".if %[V] == 2\n\tv_add_u32 %[pre], %[nb], %[nb]\n\t"
            ".else\n\tv_add_u32_dpp %[pre], %[nb], %[nb] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t.endif\n\t"
            "v_sub_u32 %[q], %[q], %[pre]\n\t"
            "v_bfe_u32 %[at], %[q], 5, 8\n\tv_lshl_add_u32 %[at], %[at], 2, %[ringb]\n\t"
            ".if %[V] != 3\n\tds_read_b32 %[w0], %[at]\n\tds_read_b32 %[w1], %[at] offset:4\n\t.endif\n\t"
            ".endif\n\t"
            ".endr\n\t"
            "s_waitcnt lgkmcnt(0)"
            : [st] "+v"(st), [q] "+v"(q), [e] "=&v"(e), [w0] "=&v"(w0), [w1] "=&v"(w1), [c] "=&v"(c), [nb] "=&v"(nb), [m] "=&v"(m),
              [hi] "=&v"(hi), [pre] "=&v"(pre), [at] "=&v"(at)
            : [C] "v"(C), [mk1] "v"(mk1), [cb] "v"(cb), [ringb] "v"(ringb), [stg] "v"(stgb), [V] "n"(V)
            : "memory");
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (lane == 0) cyc[blockIdx.x * 3 + wv] = t1 - t0;
    if (st == 0xFFFFFFFFu) out[1] = st + q;
}

// Bare chain (entry -> ffbh -> sub -> alignbit -> lshl_add -> entry) plus X extra DEPENDENT instructions of one kind in the chain:
// K: 0 none | 1 v_alignbit_b32 | 2 v_and_b32_dpp quad_perm | 3 v_lshlrev_b32 | 4 s_waitcnt (satisfied) | 5 v_add_u32 | 6 v_mov_b32_dpp |
//    7 v_mov + v_lshlrev_b64 + v_mov (the 64-bit shift between two moves)
template <int K, int X>
__global__ void __launch_bounds__(64) k_cost(const uint16_t *tab, uint32_t *out, int chunks, unsigned long long *cyc) {
    extern __shared__ uint32_t s_mem[];
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t i = lane; i < 4096; i += 64) s_mem[(TAB >> 2) + i] = ((const uint32_t *)tab)[i];
    __syncthreads();
    const uint32_t cb = TAB - 2u * 8192u, C = 31u - 13u, ones = ~0u, zero = 0;
    uint32_t st = 8192u + ((out[0] + 17u * lane) & 8191u), q = 0x12345678u, e, c, m, at;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int ch = 0; ch < chunks; ch++) {
        asm volatile(
            "v_lshl_add_u32 %[at], %[st], 1, %[cb]\n\tds_read_u16 %[e], %[at]\n\t"
            ".rept 64\n\t"
            "s_waitcnt lgkmcnt(0)\n\t"
            "v_ffbh_u32 %[c], %[e]\n\t"
            "v_sub_u32 %[m], %[C], %[c]\n\t"
            ".rept %[X]\n\t"
            ".if %[K] == 1\n\tv_alignbit_b32 %[m], %[zero], %[m], %[zero]\n\t"
            ".elseif %[K] == 2\n\tv_and_b32_dpp %[m], %[m], %[ones] quad_perm:[0,1,2,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            ".elseif %[K] == 3\n\tv_lshlrev_b32 %[m], %[zero], %[m]\n\t"
            ".elseif %[K] == 4\n\ts_waitcnt lgkmcnt(0)\n\t"
            ".elseif %[K] == 5\n\tv_add_u32 %[m], %[m], %[zero]\n\t"
            ".elseif %[K] == 6\n\tv_mov_b32_dpp %[m], %[m] quad_perm:[0,1,2,3] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            ".elseif %[K] == 7\n\tv_mov_b32 v61, %[m]\n\tv_lshlrev_b64 v[62:63], %[zero], v[60:61]\n\tv_mov_b32 %[m], v63\n\t"
            ".endif\n\t"
            ".endr\n\t"
            "v_alignbit_b32 %[st], %[e], %[q], %[m]\n\t"
            "v_lshl_add_u32 %[at], %[st], 1, %[cb]\n\tds_read_u16 %[e], %[at]\n\t"
            ".endr\n\t"
            "s_waitcnt lgkmcnt(0)"
            : [st] "+v"(st), [e] "=&v"(e), [c] "=&v"(c), [m] "=&v"(m), [at] "=&v"(at)
            : [C] "v"(C), [cb] "v"(cb), [q] "v"(q), [ones] "v"(ones), [zero] "v"(zero), [K] "n"(K), [X] "n"(X) : "memory");
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (lane == 0) cyc[blockIdx.x] = t1 - t0;
    if (st == 0xFFFFFFFFu) out[1] = st;
}
template <int K, int X> int cost(const char *name, const uint16_t *d_tab, uint32_t *d_out, unsigned long long *d_cyc, int chunks) {
    hipLaunchKernelGGL((k_cost<K, X>), dim3(1), dim3(64), 20 * 1024, 0, d_tab, d_out, chunks, d_cyc);
    CK(hipDeviceSynchronize());
    unsigned long long c = 0;
    CK(hipMemcpy(&c, d_cyc, 8, hipMemcpyDeviceToHost));
    printf("chain + %d x %-28s %6.1f cycles/round\n", X, name, (double)c / ((double)chunks * 64.0));
    return 0;
}

// Candidate rounds of the m-only form (v_sub m = -nbBits; rotate instead of shift).  W: 0 ds_read2_b32 window | 1 two ds_read_b32.
// P: where the stage store sits: 0 tail (stores the new state) | 1 head, behind v_sub (stores the round's start state) |
//    2 as 1, and v_and_dpp moved in front of the window wait (s_nop for the DPP hazard).
template <int W, int P>
__global__ void __launch_bounds__(192) k_cand(const uint16_t *tab, uint32_t *out, int chunks, unsigned long long *cyc) {
    extern __shared__ uint32_t s_mem[];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t g = lane / 2; if (g >= 3) g = 0;
    const uint32_t k = lane & 1;
    const uint32_t sbase = (wv * 3 + g) * STREAM_BYTES;
    for (uint32_t j = 0; j < 3; j++) {
        const uint32_t tb = ((wv * 3 + j) * STREAM_BYTES + TAB) >> 2;
        for (uint32_t i = lane; i < 4096; i += 64) s_mem[tb + i] = ((const uint32_t *)tab)[i];
        const uint32_t rb = ((wv * 3 + j) * STREAM_BYTES) >> 2;
        for (uint32_t i = lane; i < 260; i += 64) s_mem[rb + i] = 0x9E3779B9u * (i + 1 + j);
    }
    __syncthreads();
    const uint32_t cb = sbase + TAB - 2u * 8192u, C = 31u - 13u, ringb = sbase, stgb = sbase + STAGE + 2u * k;
    const uint32_t mk1 = k ? ~0u : 0u;
    uint32_t st = 8192u + ((out[0] + 17u * lane) & 8191u), q = 1u << 20;
    uint32_t e, c, m, hi, pre, at;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int ch = 0; ch < chunks; ch++) {
        asm volatile(
            ".set ls_off, 0\n\t"
            "v_lshl_add_u32 %[at], %[st], 1, %[cb]\n\tds_read_u16 %[e], %[at]\n\t"
            ".if %[P] == 0\n\tds_write_b16 %[stg], %[st] offset:ls_off\n\t.set ls_off, ls_off+4\n\t.endif\n\t"
            "v_bfe_u32 %[at], %[q], 5, 8\n\tv_lshl_add_u32 %[at], %[at], 2, %[ringb]\n\t"
            ".if %[W] == 0\n\tds_read2_b32 v[62:63], %[at] offset1:1\n\t.else\n\tds_read_b32 v62, %[at]\n\tds_read_b32 v63, %[at] offset:4\n\t.endif\n\t"
            ".rept 64\n\t"
            // wait for the entry: queue (oldest first) P0: e, stage, window(1 or 2) ; P1/P2: e, window(1 or 2)
            ".if %[P] == 0\n\t.if %[W] == 0\n\ts_waitcnt lgkmcnt(2)\n\t.else\n\ts_waitcnt lgkmcnt(3)\n\t.endif\n\t"
            ".else\n\t.if %[W] == 0\n\ts_waitcnt lgkmcnt(1)\n\t.else\n\ts_waitcnt lgkmcnt(2)\n\t.endif\n\t.endif\n\t"
            "v_ffbh_u32 %[c], %[e]\n\t"
            "v_sub_u32 %[m], %[C], %[c]\n\t"
            ".if %[P] != 0\n\tds_write_b16 %[stg], %[st] offset:ls_off\n\t.set ls_off, ls_off+4\n\t.endif\n\t"
            ".if %[P] == 2\n\ts_nop 0\n\tv_and_b32_dpp %[pre], %[m], %[mk1] quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t.endif\n\t"
            // wait for the window: P0: only older ops matter -> 0 ; P1/P2: the stage store is younger than the window
            ".if %[P] == 0\n\ts_waitcnt lgkmcnt(0)\n\t.else\n\ts_waitcnt lgkmcnt(1)\n\t.endif\n\t"
            "v_alignbit_b32 %[hi], v63, v62, %[q]\n\t"
            ".if %[P] != 2\n\tv_and_b32_dpp %[pre], %[m], %[mk1] quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t.endif\n\t"
            "v_alignbit_b32 %[hi], %[hi], %[hi], %[pre]\n\t"
            "v_alignbit_b32 %[st], %[e], %[hi], %[m]\n\t"
            "v_lshl_add_u32 %[at], %[st], 1, %[cb]\n\tds_read_u16 %[e], %[at]\n\t"
            ".if %[P] == 0\n\t.if ls_off < 256\n\tds_write_b16 %[stg], %[st] offset:ls_off\n\t.endif\n\t.set ls_off, ls_off+4\n\t.endif\n\t"
            "v_add_u32_dpp %[pre], %[m], %[m] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
            "v_add_u32 %[q], %[q], %[pre]\n\t"
            "v_bfe_u32 %[at], %[q], 5, 8\n\tv_lshl_add_u32 %[at], %[at], 2, %[ringb]\n\t"
            ".if %[W] == 0\n\tds_read2_b32 v[62:63], %[at] offset1:1\n\t.else\n\tds_read_b32 v62, %[at]\n\tds_read_b32 v63, %[at] offset:4\n\t.endif\n\t"
            ".endr\n\t"
            "s_waitcnt lgkmcnt(0)"
            : [st] "+v"(st), [q] "+v"(q), [e] "=&v"(e), [c] "=&v"(c), [m] "=&v"(m), [hi] "=&v"(hi), [pre] "=&v"(pre), [at] "=&v"(at)
            : [C] "v"(C), [mk1] "v"(mk1), [cb] "v"(cb), [ringb] "v"(ringb), [stg] "v"(stgb), [W] "n"(W), [P] "n"(P)
            : "memory", "v62", "v63");
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (lane == 0) cyc[blockIdx.x * 3 + wv] = t1 - t0;
    if (st == 0xFFFFFFFFu) out[1] = st + q;
}
template <int W, int P> int cand(const char *name, const uint16_t *d_tab, uint32_t *d_out, unsigned long long *d_cyc, int chunks) {
    CK(hipFuncSetAttribute((const void *)k_cand<W, P>, hipFuncAttributeMaxDynamicSharedMemorySize, 9 * STREAM_BYTES));
    hipLaunchKernelGGL((k_cand<W, P>), dim3(1), dim3(192), 9 * STREAM_BYTES, 0, d_tab, d_out, chunks, d_cyc);
    CK(hipDeviceSynchronize());
    unsigned long long c[3];
    CK(hipMemcpy(c, d_cyc, 24, hipMemcpyDeviceToHost));
    printf("%-70s %6.1f cycles/round\n", name, (double)c[1] / ((double)chunks * 64.0));
    return 0;
}

// Candidate rounds that take the window read off the round's dependent path (measured against k_cand<0, 1>, the shipped order).
// E1: 1 = the window a round early.  The tail of a round, where the next position q' is known, picks the next round's window from
//     three ring dwords read a round before (the dwords of q - 32, q, q + 32 for the position q of that time: two states take
//     <= 32 bits, so q' is in the first or the second of them -- the same ring address as then, or the one below) with a compare
//     of the two ring addresses, two v_cndmask and one v_alignbit, and then reads the three dwords at q'.  All of it sits in the
//     shadow of the look-up; behind the entry's s_waitcnt the head holds no LDS wait.  One register set does: the selects read
//     the old dwords before the new read is issued.  The ring addresses alternate between two registers: a double round.
// E2: where the second state's offset (the first state's nbBits) comes from.  0 = v_and_b32_dpp of m (shipped; m is fresh from a
//     VALU write, so two slots must separate them) | 1 = v_ffbh_u32_dpp of the partner's ENTRY (fresh from LDS: no hazard), then one
//     v_mad_i32_i24 per lane (state 1: C - c', state 0: 0 * c' + 0), lanes as shipped | 2 = the same on N = 4's lane layout (a DPP
//     row per stream, EXEC = lanes 0 and 1 of a row): row_shr:1 without bound_ctrl leaves lane 0's register at its preset C, v_sub.
//     With E1 the stage store moves to the tail (it stores the state the NEXT round starts from); E1 alone keeps it in the head,
//     beside an s_nop, as the two slots the DPP read of m needs.
// LDS queue, oldest first, at the entry's wait | at the tail's wait for the three dwords (E1):
//     E1 = 0: entry, window                                   (as shipped)
//     E1 = 1, E2 = 0: entry, dwords (2)                       | dwords (2), stage, entry
//     E1 = 1, E2 > 0: entry, stage, dwords (2)                | dwords (2), entry, stage
#define UE_LOOKUP "v_lshl_add_u32 %[at], %[st], 1, %[cb]\n\tds_read_u16 %[e], %[at]\n\t"
#define UE_ROUND(AN_, AO_) \
            ".if %[E1] == 0\n\ts_waitcnt lgkmcnt(1)\n\t.elseif %[E2] == 0\n\ts_waitcnt lgkmcnt(2)\n\t.else\n\ts_waitcnt lgkmcnt(3)\n\t.endif\n\t" \
            ".if %[E2] == 0\n\t" \
            "v_ffbh_u32 %[c], %[e]\n\t" \
            "v_sub_u32 %[m], %[C], %[c]\n\t" \
            "ds_write_b16 %[stg], %[st] offset:ls_off\n\t.set ls_off, ls_off+4\n\t" \
            ".if %[E1] == 0\n\ts_waitcnt lgkmcnt(1)\n\tv_alignbit_b32 %[hi], v63, v62, %[q]\n\t.else\n\ts_nop 0\n\t.endif\n\t" \
            "v_and_b32_dpp %[pre], %[m], %[mk1] quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
            ".else\n\t" \
            ".if %[E2] == 1\n\tv_ffbh_u32_dpp %[cp], %[e] quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
            ".else\n\tv_ffbh_u32_dpp %[cp], %[e] row_shr:1 row_mask:0xf bank_mask:0xf\n\t.endif\n\t" \
            "v_ffbh_u32 %[c], %[e]\n\t" \
            ".if %[E2] == 1\n\tv_mad_i32_i24 %[pre], %[cp], %[mk1], %[Ck]\n\t.else\n\tv_sub_u32 %[pre], %[C], %[cp]\n\t.endif\n\t" \
            "v_sub_u32 %[m], %[C], %[c]\n\t" \
            ".if %[E1] == 0\n\t" \
            "ds_write_b16 %[stg], %[st] offset:ls_off\n\t.set ls_off, ls_off+4\n\t" \
            "s_waitcnt lgkmcnt(1)\n\tv_alignbit_b32 %[hi], v63, v62, %[q]\n\t" \
            ".endif\n\t" \
            ".endif\n\t" \
            "v_alignbit_b32 %[hi], %[hi], %[hi], %[pre]\n\t" \
            "v_alignbit_b32 %[st], %[e], %[hi], %[m]\n\t" \
            UE_LOOKUP \
            ".if %[E1] != 0 && %[E2] != 0\n\t.if ls_off < 256\n\tds_write_b16 %[stg], %[st] offset:ls_off\n\t.endif\n\t.set ls_off, ls_off+4\n\t.endif\n\t" \
            "v_add_u32_dpp %[pre], %[m], %[m] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
            "v_add_u32 %[q], %[q], %[pre]\n\t" \
            "v_bfe_u32 " AN_ ", %[q], 5, 8\n\tv_lshl_add_u32 " AN_ ", " AN_ ", 2, %[ringb]\n\t" \
            ".if %[E1] == 0\n\t" \
            "ds_read2_b32 v[62:63], " AN_ " offset1:1\n\t" \
            ".else\n\t" \
            "v_cmp_eq_u32 vcc, " AN_ ", " AO_ "\n\t" \
            "s_waitcnt lgkmcnt(2)\n\t" \
            "v_cndmask_b32 %[lo], v56, v57, vcc\n\t" \
            "v_cndmask_b32 %[hh], v57, v58, vcc\n\t" \
            "v_alignbit_b32 %[hi], %[hh], %[lo], %[q]\n\t" \
            "ds_read2_b32 v[56:57], " AN_ " offset1:1\n\t" \
            "ds_read_b32 v58, " AN_ " offset:8\n\t" \
            ".endif\n\t"
template <int E1, int E2>
__global__ void __launch_bounds__(192) k_early(const uint16_t *tab, uint32_t *out, int chunks, unsigned long long *cyc) {
    extern __shared__ uint32_t s_mem[];
    constexpr uint32_t LS = E2 == 2 ? 16 : 2;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t g = lane / LS; if (g >= 3) g = 0;
    const uint32_t k = lane & 1;
    const uint32_t sbase = (wv * 3 + g) * STREAM_BYTES;
    for (uint32_t j = 0; j < 3; j++) {
        const uint32_t tb = ((wv * 3 + j) * STREAM_BYTES + TAB) >> 2;
        for (uint32_t i = lane; i < 4096; i += 64) s_mem[tb + i] = ((const uint32_t *)tab)[i];
        const uint32_t rb = ((wv * 3 + j) * STREAM_BYTES) >> 2;
        for (uint32_t i = lane; i < 260; i += 64) s_mem[rb + i] = 0x9E3779B9u * (i + 1 + j);
    }
    __syncthreads();
    const uint32_t cb = sbase + TAB - 2u * 8192u, C = 31u - 13u, ringb = sbase, stgb = sbase + STAGE + 2u * k;
    const uint32_t mk1 = k ? ~0u : 0u, Ck = k ? C : 0u;
    const uint64_t em = E2 == 2 ? 0x0000000300030003ull : ~0ull;
    uint32_t st = 8192u + ((out[0] + 17u * lane) & 8191u), q = 1u << 20, cp = C;
    uint32_t e, c, m, hi, pre, at, a0, a1, lo, hh;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int ch = 0; ch < chunks; ch++) {
        asm volatile(
            ".set ls_off, 0\n\t"
            "s_mov_b64 exec, %[em]\n\t"
            UE_LOOKUP
            ".if %[E1] != 0 && %[E2] != 0\n\tds_write_b16 %[stg], %[st]\n\t.set ls_off, 4\n\t.endif\n\t"
            "v_bfe_u32 %[a1], %[q], 5, 8\n\tv_lshl_add_u32 %[a1], %[a1], 2, %[ringb]\n\t"
            ".if %[E1] == 0\n\t"
            "ds_read2_b32 v[62:63], %[a1] offset1:1\n\t"
            ".else\n\t"                                                      // round 0's window from the upper pair; round 0's tail picks round 1's from the same three
            "ds_read2_b32 v[56:57], %[a1] offset1:1\n\t"
            "ds_read_b32 v58, %[a1] offset:8\n\t"
            "s_waitcnt lgkmcnt(0)\n\t"
            "v_alignbit_b32 %[hi], v58, v57, %[q]\n\t"
            ".endif\n\t"
            ".rept 32\n\t"
            UE_ROUND("%[a0]", "%[a1]")
            UE_ROUND("%[a1]", "%[a0]")
            ".endr\n\t"
            "s_waitcnt lgkmcnt(0)\n\t"
            "s_mov_b64 exec, -1"
            : [st] "+v"(st), [q] "+v"(q), [cp] "+v"(cp), [e] "=&v"(e), [c] "=&v"(c), [m] "=&v"(m), [hi] "=&v"(hi), [pre] "=&v"(pre), [at] "=&v"(at),
              [a0] "=&v"(a0), [a1] "=&v"(a1), [lo] "=&v"(lo), [hh] "=&v"(hh)
            : [C] "v"(C), [mk1] "v"(mk1), [Ck] "v"(Ck), [cb] "v"(cb), [ringb] "v"(ringb), [stg] "v"(stgb), [em] "s"(em), [E1] "n"(E1), [E2] "n"(E2)
            : "memory", "vcc", "v56", "v57", "v58", "v62", "v63");
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (lane == 0) cyc[blockIdx.x * 3 + wv] = t1 - t0;
    if (st == 0xFFFFFFFFu) out[1] = st + q + cp;
}
template <int E1, int E2> int early(const char *name, const uint16_t *d_tab, uint32_t *d_out, unsigned long long *d_cyc, int chunks) {
    CK(hipFuncSetAttribute((const void *)k_early<E1, E2>, hipFuncAttributeMaxDynamicSharedMemorySize, 9 * STREAM_BYTES));
    hipLaunchKernelGGL((k_early<E1, E2>), dim3(1), dim3(192), 9 * STREAM_BYTES, 0, d_tab, d_out, chunks, d_cyc);
    CK(hipDeviceSynchronize());
    unsigned long long c[3];
    CK(hipMemcpy(c, d_cyc, 24, hipMemcpyDeviceToHost));
    printf("%-70s %6.1f cycles/round (waves %.1f %.1f %.1f)\n", name, (double)c[1] / ((double)chunks * 64.0), (double)c[0] / ((double)chunks * 64.0),
           (double)c[1] / ((double)chunks * 64.0), (double)c[2] / ((double)chunks * 64.0));
    return 0;
}

// N = 4 in ONE LDS round trip: the round's 64-bit window (three ring dwords at the round's start position) is read with the table
// look-ups; a state's bits are the top nbBits of window << (bits of the earlier states), a v_lshlrev_b64.  The prefix sum of
// m = -nbBits over a stream's four lanes runs in place on two v_add_u32_dpp (row_shr:1, row_shr:2, no bound_ctrl): a stream's lanes
// open a DPP row of 16, so its first lane (first two) has no source and keeps its value; EXEC = the states' lanes.
// (A DPP bank_mask selects groups of four CONSECUTIVE lanes, not lane % 4: it cannot do this inside a quad.)
// V: 0 as described | 1 without the 64-bit shift (two funnel shifts, compare, select: exact only for the first state's zero offset
//    through a lane mask)
template <int V>
__global__ void __launch_bounds__(192) k_cand4(const uint16_t *tab, uint32_t *out, int chunks, unsigned long long *cyc) {
    extern __shared__ uint32_t s_mem[];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t g = lane / 16; if (g >= 3) g = 0;
    const uint32_t k = lane & 3;
    const uint32_t sbase = (wv * 3 + g) * STREAM_BYTES;
    for (uint32_t j = 0; j < 3; j++) {
        const uint32_t tb = ((wv * 3 + j) * STREAM_BYTES + TAB) >> 2;
        for (uint32_t i = lane; i < 4096; i += 64) s_mem[tb + i] = ((const uint32_t *)tab)[i];
        const uint32_t rb = ((wv * 3 + j) * STREAM_BYTES) >> 2;
        for (uint32_t i = lane; i < 260; i += 64) s_mem[rb + i] = 0x9E3779B9u * (i + 1 + j);
    }
    __syncthreads();
    const uint32_t cb = sbase + TAB - 2u * 8192u, C = 31u - 13u, ringb = sbase, stgb = sbase + STAGE + 2u * k;
    const uint32_t K31 = (uint32_t)-31;
    const uint64_t em = 0x0000000F000F000Full;
    const uint64_t mk0 = 0x1111111111111111ull;
    uint32_t st = 8192u + ((out[0] + 17u * lane) & 8191u), qm = 1u << 20;
    uint32_t e, c, a, m, p, at, tot, xa, xb;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int ch = 0; ch < chunks; ch++) {
        asm volatile(
            ".set ls_off, 8\n\t"
            "s_mov_b64 exec, %[em]\n\t"
            "v_lshl_add_u32 %[at], %[st], 1, %[cb]\n\tds_read_u16 %[e], %[at]\n\t"
            "v_bfe_u32 %[at], %[qm], 5, 8\n\tv_lshl_add_u32 %[at], %[at], 2, %[ringb]\n\t"
            "ds_read2_b32 v[60:61], %[at] offset1:1\n\tds_read_b32 v62, %[at] offset:8\n\t"
            "ds_write_b16 %[stg], %[st]\n\t"
            ".rept 32\n\t"
            "s_waitcnt lgkmcnt(3)\n\t"
            "v_ffbh_u32 %[c], %[e]\n\t"
            "v_sub_u32 %[a], %[C], %[c]\n\t"
            "s_waitcnt lgkmcnt(1)\n\t"
            "v_alignbit_b32 v58, v61, v60, %[qm]\n\t"
            "v_add_u32_dpp %[a], %[a], %[a] row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
            "v_alignbit_b32 v59, v62, v61, %[qm]\n\t"
            "v_sub_u32 %[m], %[C], %[c]\n\t"
            "v_add_u32_dpp %[a], %[a], %[a] row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
            ".if %[V] == 0\n\t"
            "v_sub_u32 %[p], %[m], %[a]\n\t"
            "v_lshlrev_b64 v[56:57], %[p], v[58:59]\n\t"
            "v_alignbit_b32 %[st], %[e], v57, %[m]\n\t"
            ".else\n\t"
            "v_sub_u32 %[p], %[a], %[m]\n\t"
            "v_alignbit_b32 %[xa], v59, v58, %[p]\n\t"
            "v_alignbit_b32 %[xb], v58, v58, %[p]\n\t"
            "v_cmp_lt_i32 vcc, %[p], %[K31]\n\t"
            "v_cndmask_b32 %[xa], %[xa], %[xb], vcc\n\t"
            "v_cndmask_b32 %[xa], %[xa], v59, %[mk0]\n\t"
            "v_alignbit_b32 %[st], %[e], %[xa], %[m]\n\t"
            ".endif\n\t"
            "v_lshl_add_u32 %[at], %[st], 1, %[cb]\n\tds_read_u16 %[e], %[at]\n\t"
            "v_mov_b32_dpp %[tot], %[a] quad_perm:[3,3,3,3] row_mask:0xf bank_mask:0xf\n\t"
            "v_add_u32 %[qm], %[qm], %[tot]\n\t"
            "v_bfe_u32 %[at], %[qm], 5, 8\n\tv_lshl_add_u32 %[at], %[at], 2, %[ringb]\n\t"
            "ds_read2_b32 v[60:61], %[at] offset1:1\n\tds_read_b32 v62, %[at] offset:8\n\t"
            ".if ls_off < 256\n\tds_write_b16 %[stg], %[st] offset:ls_off\n\t.endif\n\t"
            ".set ls_off, ls_off+8\n\t"
            ".endr\n\t"
            "s_waitcnt lgkmcnt(0)\n\t"
            "s_mov_b64 exec, -1"
            : [st] "+v"(st), [qm] "+v"(qm), [e] "=&v"(e), [c] "=&v"(c), [a] "=&v"(a), [m] "=&v"(m), [p] "=&v"(p), [at] "=&v"(at), [tot] "=&v"(tot),
              [xa] "=&v"(xa), [xb] "=&v"(xb)
            : [C] "v"(C), [cb] "v"(cb), [ringb] "v"(ringb), [stg] "v"(stgb), [K31] "v"(K31), [mk0] "s"(mk0), [em] "s"(em), [V] "n"(V)
            : "memory", "vcc", "v56", "v57", "v58", "v59", "v60", "v61", "v62");
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (lane == 0) cyc[blockIdx.x * 3 + wv] = t1 - t0;
    if (st == 0xFFFFFFFFu) out[1] = st + qm;
}
template <int V> int cand4(const char *name, const uint16_t *d_tab, uint32_t *d_out, unsigned long long *d_cyc, int chunks) {
    CK(hipFuncSetAttribute((const void *)k_cand4<V>, hipFuncAttributeMaxDynamicSharedMemorySize, 9 * STREAM_BYTES));
    hipLaunchKernelGGL((k_cand4<V>), dim3(1), dim3(192), 9 * STREAM_BYTES, 0, d_tab, d_out, chunks, d_cyc);
    CK(hipDeviceSynchronize());
    unsigned long long c[3];
    CK(hipMemcpy(c, d_cyc, 24, hipMemcpyDeviceToHost));
    printf("%-70s %6.1f cycles/round of FOUR symbols\n", name, (double)c[1] / ((double)chunks * 32.0));
    return 0;
}

template <int V> int run(const char *name, const uint16_t *d_tab, uint32_t *d_out, unsigned long long *d_cyc, int blocks, int waves, int chunks) {
    CK(hipFuncSetAttribute((const void *)k_round<V>, hipFuncAttributeMaxDynamicSharedMemorySize, 9 * STREAM_BYTES));
    hipLaunchKernelGGL(k_round<V>, dim3(blocks), dim3(64 * waves), 9 * STREAM_BYTES, 0, d_tab, d_out, chunks, d_cyc);
    CK(hipDeviceSynchronize());
    std::vector<unsigned long long> c((size_t)blocks * 3);
    CK(hipMemcpy(c.data(), d_cyc, c.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> v;
    for (int b = 0; b < blocks; b++) for (int w = 0; w < waves; w++) v.push_back((double)c[(size_t)b * 3 + w] / ((double)chunks * 64.0));
    std::sort(v.begin(), v.end());
    printf("%-46s blocks %3d waves %d: %6.1f cycles/round (min %.1f max %.1f)\n", name, blocks, waves, v[v.size() / 2], v.front(), v.back());
    return 0;
}

int main() {
    // table: nextState values whose nbBits (13 - highbit) average ~5.5, like 12-bit noise at ratio ~2
    std::vector<uint16_t> tab(8192);
    uint32_t x = 12345;
    for (auto &t : tab) { x = x * 1664525u + 1013904223u; const uint32_t nb = 3 + (x >> 28) % 6; t = (uint16_t)((1u << (13 - nb)) + ((x >> 8) & ((1u << (13 - nb)) - 1))); }
    uint16_t *d_tab; uint32_t *d_out; unsigned long long *d_cyc;
    CK(hipMalloc(&d_tab, 16384)); CK(hipMalloc(&d_out, 64)); CK(hipMalloc(&d_cyc, 8 * 3 * 1024));
    CK(hipMemcpy(d_tab, tab.data(), 16384, hipMemcpyHostToDevice)); CK(hipMemset(d_out, 0, 64));
    const int chunks = 400;
    cand<0, 0>("m-only round, ds_read2 window, stage store in the tail", d_tab, d_out, d_cyc, chunks);
    cand<1, 0>("m-only round, two ds_read_b32, stage store in the tail", d_tab, d_out, d_cyc, chunks);
    cand<0, 1>("m-only round, ds_read2 window, stage store in the head (shipped)", d_tab, d_out, d_cyc, chunks);
    cand<1, 1>("m-only round, two ds_read_b32, stage store in the head", d_tab, d_out, d_cyc, chunks);
    cand<0, 2>("... and v_and_dpp in front of the window wait", d_tab, d_out, d_cyc, chunks);
    cand<1, 2>("... the same with two ds_read_b32", d_tab, d_out, d_cyc, chunks);
    early<0, 0>("double round, shipped order (= k_cand<0,1>)", d_tab, d_out, d_cyc, chunks);
    early<1, 0>("E1: window a round early", d_tab, d_out, d_cyc, chunks);
    early<0, 1>("E2: partner's nbBits by v_ffbh_dpp of its entry + v_mad, lanes as shipped", d_tab, d_out, d_cyc, chunks);
    early<0, 2>("E2: ... row per stream, row_shr:1 + v_sub", d_tab, d_out, d_cyc, chunks);
    early<1, 1>("E1 + E2, lanes as shipped (v_mad)", d_tab, d_out, d_cyc, chunks);
    early<1, 2>("E1 + E2, row per stream (v_sub)", d_tab, d_out, d_cyc, chunks);
    cand<0, 1>("shipped order again", d_tab, d_out, d_cyc, chunks);
    cand4<0>("N = 4, one LDS round trip, v_lshlrev_b64", d_tab, d_out, d_cyc, chunks);
    cand4<1>("N = 4, one LDS round trip, funnel shifts + selects", d_tab, d_out, d_cyc, chunks);
    cost<7, 1>("v_mov, v_lshlrev_b64, v_mov", d_tab, d_out, d_cyc, chunks); cost<7, 4>("v_mov, v_lshlrev_b64, v_mov", d_tab, d_out, d_cyc, chunks);
    cost<0, 0>("(nothing)", d_tab, d_out, d_cyc, chunks);
    cost<1, 1>("v_alignbit_b32", d_tab, d_out, d_cyc, chunks); cost<1, 4>("v_alignbit_b32", d_tab, d_out, d_cyc, chunks);
    cost<2, 1>("v_and_b32_dpp", d_tab, d_out, d_cyc, chunks); cost<2, 4>("v_and_b32_dpp", d_tab, d_out, d_cyc, chunks);
    cost<3, 1>("v_lshlrev_b32", d_tab, d_out, d_cyc, chunks); cost<3, 4>("v_lshlrev_b32", d_tab, d_out, d_cyc, chunks);
    cost<4, 1>("s_waitcnt (satisfied)", d_tab, d_out, d_cyc, chunks); cost<4, 4>("s_waitcnt (satisfied)", d_tab, d_out, d_cyc, chunks);
    cost<5, 1>("v_add_u32", d_tab, d_out, d_cyc, chunks); cost<5, 4>("v_add_u32", d_tab, d_out, d_cyc, chunks);
    cost<6, 1>("v_mov_b32_dpp", d_tab, d_out, d_cyc, chunks); cost<6, 4>("v_mov_b32_dpp", d_tab, d_out, d_cyc, chunks);
    for (int blocks : {1}) {
        run<0>("shipped round", d_tab, d_out, d_cyc, blocks, 3, chunks);
        run<0>("shipped round, one wave per CU", d_tab, d_out, d_cyc, blocks, 1, chunks);
        run<1>("no stage store", d_tab, d_out, d_cyc, blocks, 3, chunks);
        run<2>("plain VALU instead of DPP", d_tab, d_out, d_cyc, blocks, 3, chunks);
        run<3>("no window reads", d_tab, d_out, d_cyc, blocks, 3, chunks);
        run<6>("one wait per round (entry + window)", d_tab, d_out, d_cyc, blocks, 3, chunks);
        run<4>("bare chain: entry, ffbh, 2 sub, alignbit, lshl_add", d_tab, d_out, d_cyc, blocks, 3, chunks);
    }
    return 0;
}
