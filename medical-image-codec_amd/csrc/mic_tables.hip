// mic_tables.hip -- per-unit FSE table kernels (encode and decode side), one work-group of 1024
// threads per unit.
//
//   k_enc_tables_wg  histogram scan -> gates -> tableLog -> normalise -> NCount header -> CTable
//                    (fse2state.go:22-52; fsecompressu16.go:465-571, :191-289, :329-431)
//   k_dec_tables_wg  prefix / flavour -> NCount parse -> decode table
//                    (fse2state.go:102-116; fsedecompressu16.go:48-263; ransu16.go:77-135)
//
// What runs where: normalisation, the symbol prefix sums, the symbol spread and the slot
// numbering are data-parallel (mic_tables_par.h); the NCount header is a variable-width bit
// packing whose 32-bit accumulator wraps exactly like the reference's (fsecompressu16.go:260-262)
// and stays on one lane, reading norm[] from LDS.  "Small" units (alphabet <= 8192 symbols,
// tableLog <= 13: every 8..12-bit image) keep all scratch in LDS as 16-bit values; anything
// larger (16-bit CT: 65536 symbols, tableLog 16) uses the unit's HBM scratch slabs through the
// same code.
//
// Each kernel comes in two instances (TbLds below).  The compact one takes the small tANS units of
// at most 4096 symbols -- the tokens of every frame of up to 12 bits -- with a carve-up of 68.5 KiB
// and at most 64 VGPRs: two work-groups per CU, which cover each other's barrier and LDS stalls.
// The standard one (96.4 KiB, one work-group per CU) takes everything else: larger alphabets,
// tableLog above 13, rANS, the HBM scratch path -- and every unit the compact one did not take.
// The compact one is launched first, over the whole batch, when the launch masks say the batch may
// hold such a unit (mic_launch.h: what the host knows and what the session remembers; a wrong
// guess costs time, never correctness); a group returns at once for a unit that is not its own,
// and MicUnit.tb_inst says which instance built a unit's tables.
#include "mic_dev.h"
#include "mic_fse_tables.h"
#include "mic_tables_par.h"
#include "mic_launch.h"
#include "mic_wave.h"

#define TB_SMALL_SYMS 8192
#define TB_SMALL_TL 13
#define TB_C4K_SYMS 4096                     // the compact instance's alphabet

// LDS carve-up shared by both kernels (bytes), per instance.  The small path of tp_build ranks its big symbols by waves: wave w
// owns words [256 w, 256 w + 256) from BITMAP on (16 KiB, running on into WPREF) and 256 16-bit prefixes from word 1024 of BIG
// on (8 KiB behind a list of at most 2^13 / 17 symbols) -- all the compact instance keeps of the three areas.
template <bool C4K> struct TbLds {
    static constexpr uint32_t SYMS   = C4K ? TB_C4K_SYMS : TB_SMALL_SYMS;
    static constexpr uint32_t NORM   = 0;                                 // int16[SYMS]
    static constexpr uint32_t FIRST  = 2 * SYMS;                          // uint16[SYMS]
    static constexpr uint32_t CUM    = 4 * SYMS;                          // uint16[SYMS]
    static constexpr uint32_t VISIT  = 6 * SYMS;                          // uint16[8192]: 2^13 table positions  (small units only)
    static constexpr uint32_t BITMAP = VISIT + 16 * 1024;                 // uint32[2048 + 1]
    static constexpr uint32_t WPREF  = BITMAP + 8256;                     // uint32[2048 + 1]
    static constexpr uint32_t BIG    = BITMAP + 16512;                    // uint32[4096 + 2]; compact: uint32[1024] + uint16[16 * 256]
    static constexpr uint32_t TMP    = BIG + (C4K ? 12288 : 16448);       // uint32[128]
    static constexpr uint32_t BYTES  = TMP + 512;                         // standard ~96.4 KiB: 1 group / CU; compact 68.5 KiB: 2
    static_assert(WPREF - BITMAP >= 4 * (2048 + 1) && BIG - WPREF >= 4 * (2048 + 1) && BIG - BITMAP >= 4 * 256 * TP_WAVES, "bitmap, prefixes; a wave's 256 words");
    static_assert(TMP - BIG >= (C4K ? 4 * 1024 + 2 * 256 * TP_WAVES : 4 * (4096 + 2)) && (1 << TB_SMALL_TL) / (TP_SMALLV + 1) < 1024, "big list (and the waves' prefixes behind it)");
    static_assert((((SYMS * TB_SMALL_TL) >> 3) + 3 + 8 + 3) / 4 * 4 <= BITMAP - VISIT, "the NCount bit buffer of a small unit fits the visit area");
    static_assert(BYTES % 16 == 0, "");
};
#define TB_STATIC_LDS 512                    // bound on what a kernel declares beside the carve-up (s_misc, the vote words)
static_assert(TbLds<false>::BYTES == 64 * 1024 + 32960 + 512 && TbLds<false>::BYTES + TB_STATIC_LDS <= 160 * 1024, "the standard instance: one group per CU");
static_assert(TbLds<true>::BYTES <= 80 * 1024 && 2 * (TbLds<true>::BYTES + TB_STATIC_LDS) <= 160 * 1024, "the compact instance: two groups per CU");
__host__ __device__ inline bool tb_is_c4k(uint32_t symbol_len, uint32_t tl, uint32_t flavour) {
    return symbol_len <= TB_C4K_SYMS && tl <= TB_SMALL_TL && flavour != 108;
}

// ------------------------------------------------------------------------------------------
// writeCount (fsecompressu16.go:191-289) on the whole group, for tableLog <= 14 (a field is at most
// 15 bits there, so the reference's 32-bit accumulator never drops any; above that the serial
// writer reproduces its wrap-around).  The header is a concatenation of bit fields, LSB first:
//   [4: tableLog-5] then, per written symbol s,  [run code][count field]
// * written symbols: every non-zero count and the first zero of a zero-run; the other zeros of a
//   run (R of them) become the run code in front of the next written symbol: 16 one-bits per 24,
//   then 2 one-bits per 3, then R % 24 % 3 in 2 bits;
// * count field: remaining = 2^tl + 1 - sum of |count| before s (a prefix sum), threshold = the
//   largest power of two <= remaining (at most 2^tl), nbBits = log2(threshold) + 1,
//   max = 2*threshold - 1 - remaining, v = count + 1 (+ max when v >= threshold), nbBits - 1 bits when v < max.
// Bit offsets are a second prefix sum; fields are OR-ed into an LDS bit buffer and copied out.
// rem16 / s016: symbol_len entries each; bitbuf: zero-initialised here, bit_base + 8 * (((symbol_len * tl) >> 3) + 8) bits.
// Small alphabets: everything in LDS, the finished header is copied to `out`.  Large ones (HBM scratch): bitbuf is
// the output itself, addressed from the aligned word 2 bytes in front of it (bit_base = 16, to_out = false).
// For tableLog 16 a count field can be 17 bits; the reference's 32-bit accumulator holds 16 pending bits at
// most when a field arrives, so a field that would not fit (pending + length > 32) makes this return
// MICD_ERR_UNSUPPORTED and the caller runs the serial writer, which reproduces the wrap (fsecompressu16.go:260-262).
template <typename NormT, typename ScrT>
__device__ int tb_write_ncount_par(const NormT *norm, uint32_t symbol_len, uint32_t tl, ScrT *rem16, ScrT *s016,
                                   uint32_t *bitbuf, uint32_t bit_base, bool to_out, uint32_t *s_tmp, uint8_t *out, uint32_t cap,
                                   uint32_t *hdr_len) {
    const uint32_t tid = threadIdx.x;
    const uint32_t size = 1u << tl;
    const uint32_t max_header = ((symbol_len * tl) >> 3) + 3;
    if (cap < max_header + 2) return MICD_ERR_CAPACITY;
    const uint32_t nwords = (bit_base / 8 + max_header + 8 + 3) / 4;
    for (uint32_t i = tid; i < nwords; i += TP_THREADS) bitbuf[i] = 0;
    // pass A: remaining in front of every symbol, first zero of the run a symbol closes
    uint32_t carry_sum = 0, carry_fz = 0;
    for (uint32_t base = 0; base < symbol_len; base += TP_THREADS) {
        const uint32_t s2 = base + tid;
        const int32_t v = (s2 < symbol_len) ? (int32_t)norm[s2] : 0;
        const int32_t vp = (s2 > 0 && s2 < symbol_len) ? (int32_t)norm[s2 - 1] : 1;
        uint32_t tot;
        const uint32_t ex = tp_block_excl((uint32_t)(v < 0 ? -v : v), s_tmp, &tot);
        // exclusive max-scan of (index + 1) of first zeros
        const uint32_t fz = (s2 < symbol_len && v == 0 && vp != 0) ? s2 + 1 : 0u;
        __syncthreads();
        uint32_t mtot;
        const uint32_t me = max(mic_group_excl_max<TP_WAVES>(fz, s_tmp + 32, &mtot), carry_fz);
        mtot = max(mtot, carry_fz);
        if (s2 < symbol_len) { rem16[s2] = (ScrT)(size + 1 - (carry_sum + ex)); s016[s2] = (ScrT)me; }
        carry_sum += tot; carry_fz = mtot;
    }
    if (carry_sum != size) return MICD_ERR_INTERNAL;          // (the serial writer ends with remaining != 1)
    __syncthreads();
    // field of symbol s: ones (run code body), then `lo` = [2-bit run remainder][count field] in lo_len bits
    auto field = [&](uint32_t s2, uint32_t &ones, uint64_t &lo, uint32_t &lo_len, uint32_t &flen_out) {
        ones = 0; lo = 0; lo_len = 0; flen_out = 0;
        const int32_t v = (int32_t)norm[s2];
        const int32_t vp = s2 > 0 ? (int32_t)norm[s2 - 1] : 1;
        if (v == 0 && vp == 0) return;                                    // inside a zero run: part of the run code
        if (vp == 0) {                                                    // closes a run of R + 1 zeros
            const uint32_t R = s2 - (uint32_t)s016[s2];
            const uint32_t r24 = R % 24;
            ones = 16 * (R / 24) + 2 * (r24 / 3);
            lo = r24 % 3; lo_len = 2;
        }
        const int32_t remaining = (int32_t)rem16[s2];
        const uint32_t hb = min(tl, (uint32_t)(31 - __clz((uint32_t)remaining)));
        const int32_t threshold = 1 << hb;
        const uint32_t nbb = hb + 1;
        const int32_t mx = (2 * threshold - 1) - remaining;
        int32_t cnt = v + 1;
        if (cnt >= threshold) cnt += mx;
        const uint32_t flen = nbb - ((cnt < mx) ? 1u : 0u);
        lo |= (uint64_t)(uint32_t)cnt << lo_len; lo_len += flen; flen_out = flen;
    };
    // pass B: offsets and packing
    uint32_t carry_bits = bit_base + 4;
    uint32_t wraps = 0;
    if (tid == 0) atomicOr(&bitbuf[bit_base >> 5], (tl - MIC_MIN_TABLELOG) << (bit_base & 31));
    for (uint32_t base = 0; base < symbol_len; base += TP_THREADS) {
        const uint32_t s2 = base + tid;
        uint32_t ones = 0, lo_len = 0, flen = 0; uint64_t lo = 0;
        if (s2 < symbol_len) field(s2, ones, lo, lo_len, flen);
        uint32_t tot;
        const uint32_t ex = tp_block_excl(ones + lo_len, s_tmp, &tot);
        uint32_t pos = carry_bits + ex;
        if (tl > 15 && flen) {                                            // pending bits when the count field arrives: 1 .. 16
            const uint32_t tb = pos - bit_base + ones + (lo_len - flen);
            if (((tb - 1) & 15u) + 1 + flen > 32) wraps = 1;
        }
        if (ones) {                                                       // bits [pos, pos + ones) set
            uint32_t left = ones;
            while (left) {
                const uint32_t sh = pos & 31, take = min(left, 32u - sh);
                const uint32_t m = (take == 32 ? 0xFFFFFFFFu : ((1u << take) - 1u)) << sh;
                atomicOr(&bitbuf[pos >> 5], m);
                pos += take; left -= take;
            }
        }
        if (lo_len) {                                                     // <= 19 bits
            const uint32_t sh = pos & 31;
            const uint64_t v = lo << sh;
            atomicOr(&bitbuf[pos >> 5], (uint32_t)v);
            if (sh + lo_len > 32) atomicOr(&bitbuf[(pos >> 5) + 1], (uint32_t)(v >> 32));
        }
        carry_bits += tot;
    }
    if (__syncthreads_or((int)wraps)) return MICD_ERR_UNSUPPORTED;
    const uint32_t nbytes = (carry_bits - bit_base + 7) >> 3;
    if (nbytes > max_header) return MICD_ERR_INTERNAL;
    if (to_out) {
        const uint8_t *bb = (const uint8_t *)bitbuf + bit_base / 8;
        for (uint32_t i = tid; i < nbytes + 8; i += TP_THREADS) out[i] = (i < nbytes) ? bb[i] : (uint8_t)0;   // + the 8 bytes k_enc_tans_wg ORs into
    }
    __threadfence_block();
    *hdr_len = nbytes;
    return MICD_OK;
}

// ------------------------------------------------------------------------------------------
template <typename NormT, typename IdxT, bool RANS>   // RANS: the instance takes rANS units (nstates 108)
__device__ void enc_tables_body(MicUnit &u, NormT *norm, IdxT *first_visit, IdxT *cum_all, uint16_t *visit_pos,
                                uint32_t *bitmap, uint32_t *wprefix, uint32_t *big_list, uint32_t *s_tmp,
                                uint32_t *s_misc, uint32_t n, uint32_t symbol_len, uint32_t tl) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t size = 1u << tl;
    const uint32_t *hist = u.hist;
    uint32_t route = sizeof(NormT) == 2 ? MIC_TBR_SMALL : MIC_TBR_HBM;  // group-uniform; lane 0 stores it with zero_bits
    MIC_STAMP_BEGIN();
    // ---- normalise, primary method (fsecompressu16.go:524-571), one symbol per thread -----------
    {
        const uint64_t scale = 62 - (uint64_t)tl;
        const uint64_t step = (1ull << 62) / (uint64_t)n;
        const uint64_t v_step = 1ull << (scale - 20);
        const uint32_t low_threshold = n >> tl;
        uint32_t used = 0;                        // sum of proba (and 1 per low-prob symbol)
        uint32_t best_p = 0, best_s = 0;          // first symbol with the largest proba
        for (uint32_t s = tid; s < symbol_len; s += TP_THREADS) {
            const uint32_t cnt = hist[s];
            int32_t nv;
            if (cnt == 0) nv = 0;
            else if (cnt <= low_threshold) { nv = -1; used += 1; }
            else {
                int32_t proba = (int32_t)(((uint64_t)cnt * step) >> scale);
                if (proba < 8) {
                    const uint64_t rest_to_beat = v_step * (uint64_t)mic_rtb_table[proba];
                    const uint64_t v = (uint64_t)cnt * step - ((uint64_t)proba << scale);
                    if (v > rest_to_beat) proba++;
                }
                nv = proba; used += (uint32_t)proba;
                if ((uint32_t)proba > best_p) { best_p = (uint32_t)proba; best_s = s; }   // s grows: first max kept
            }
            norm[s] = (NormT)nv;
        }
        // reduce: sum(used); argmax(best_p) with the smallest symbol index on ties
        const uint32_t sum = mic_wave_reduce_add(used);
        // key = proba << 17 | (65536 - s)  -> larger proba wins, then smaller s   (proba <= 65536 -> use 64 bit)
        const unsigned long long key = mic_wave_reduce_max((uint64_t)(((unsigned long long)best_p << 20) | (unsigned long long)(0xFFFFF - best_s)));
        __syncthreads();
        if (lane == 0) { s_tmp[wave] = sum; ((unsigned long long *)(s_tmp + 32))[wave] = key; }
        __syncthreads();
        if (tid == 0) {
            uint32_t tot = 0; unsigned long long k = 0;
            for (int w = 0; w < TP_WAVES; w++) { tot += s_tmp[w]; const unsigned long long o = ((unsigned long long *)(s_tmp + 32))[w]; k = k > o ? k : o; }
            const int32_t still = (int32_t)size - (int32_t)tot;
            const uint32_t largest_p = (uint32_t)(k >> 20);
            const uint32_t largest = largest_p ? (0xFFFFF - (uint32_t)(k & 0xFFFFF)) : 0u;   // no proba > 0: largest stays 0
            int rc = MICD_OK; uint32_t second = 0;
            if (-still >= ((int32_t)norm[largest] >> 1)) second = 1;                           // corner case -> normalizeCount2
            else norm[largest] = (NormT)((int32_t)norm[largest] + still);
            s_misc[2] = second; s_misc[3] = (uint32_t)rc;
        }
        __syncthreads();
        if (!s_misc[2]) route |= MIC_TBR_PRIMARY;
        else {
            // normalizeCount2 (fsecompressu16.go:573-651).  Common for alphabets close to the table size
            // (12-bit frames at tableLog 13), so it runs on the whole group: two classification passes with
            // block reductions, then the weights  (end >> v) - (start >> v)  where `end` is a running sum of
            // count * rStep over the undecided symbols -- an exclusive 64-bit prefix sum.  The two corner
            // cases that turn on a serial loop in the reference stay serial (tid 0, HBM arrays).
            const int32_t not_yet = -2;
            uint64_t *s_t64 = (uint64_t *)(s_tmp + 32);                  // 16 wave partials + spare, 8-byte aligned
            auto reduce2 = [&](uint32_t a, uint64_t b, uint32_t &ra, uint64_t &rb) {
                a = mic_wave_reduce_add(a); b = mic_wave_reduce_add(b);
                __syncthreads();
                if (lane == 0) { s_tmp[wave] = a; s_t64[wave] = b; }
                __syncthreads();
                uint32_t ta = 0; uint64_t tb = 0;
#pragma unroll 4                                                    // (sixteen partials read at once are 48 vector registers)
                for (int w = 0; w < TP_WAVES; w++) { ta += s_tmp[w]; tb += s_t64[w]; }
                ra = mic_uniform(ta); rb = mic_uniform(tb);                    // (scalar: the compact instance lives on 64 vector registers)
            };
            uint32_t total = n;
            const uint32_t low_threshold2 = total >> tl;
            uint32_t low_one = (total * 3) >> (tl + 1);
            uint32_t d1 = 0; uint64_t sub1 = 0;
            for (uint32_t s2 = tid; s2 < symbol_len; s2 += TP_THREADS) {
                const uint32_t cnt = hist[s2];
                int32_t nv;
                if (cnt == 0) nv = 0;
                else if (cnt <= low_threshold2) { nv = -1; d1++; sub1 += cnt; }
                else if (cnt <= low_one) { nv = 1; d1++; sub1 += cnt; }
                else nv = not_yet;
                norm[s2] = (NormT)nv;
            }
            uint32_t distributed; uint64_t subs;
            reduce2(d1, sub1, distributed, subs);
            total -= (uint32_t)subs;
            int rc2 = MICD_OK;
            bool serial = false;
            uint32_t to_distribute = 0;
            if (distributed >= size) rc2 = MICD_ERR_INTERNAL;            // the reference divides by zero or spins (see mic_normalize_count2)
            else {
                to_distribute = size - distributed;
                if ((total / to_distribute) > low_one) {                 // uniform
                    route |= MIC_TBR_N2_UNIFORM;
                    low_one = (total * 3) / (to_distribute * 2);
                    uint32_t d2 = 0; uint64_t sub2 = 0;
                    for (uint32_t s2 = tid; s2 < symbol_len; s2 += TP_THREADS) {
                        const uint32_t cnt = hist[s2];
                        if ((int32_t)norm[s2] == not_yet && cnt <= low_one) { norm[s2] = (NormT)1; d2++; sub2 += cnt; }
                    }
                    uint32_t dd; uint64_t ss;
                    reduce2(d2, sub2, dd, ss);
                    distributed += dd; total -= (uint32_t)ss;
                    if (distributed >= size) rc2 = MICD_ERR_INTERNAL;
                    else to_distribute = size - distributed;
                }
                if (rc2 == MICD_OK && (distributed == symbol_len + 1 || total == 0)) serial = true;
            }
            if (rc2 == MICD_OK && !serial) {
                const uint64_t v_step_log = 62 - (uint64_t)tl;
                const uint64_t midv = (1ull << (v_step_log - 1)) - 1;
                const uint64_t r_step = mic_uniform((uint64_t)((((1ull << v_step_log) * (uint64_t)to_distribute) + midv) / (uint64_t)total));
                uint64_t carry = midv;
                uint32_t badw = 0;
                for (uint32_t base = 0; base < symbol_len; base += TP_THREADS) {
                    const uint32_t s2 = base + tid;
                    const bool ny = s2 < symbol_len && (int32_t)norm[s2] == not_yet;
                    const uint64_t val = ny ? (uint64_t)hist[s2] * r_step : 0ull;
                    const uint64_t incl = mic_wave_incl_scan(val, lane, [](uint64_t a, uint64_t b) { return a + b; });
                    __syncthreads();
                    if (lane == 63) s_t64[wave] = incl;
                    __syncthreads();
                    uint64_t off = 0, tot = 0;
#pragma unroll 4
                    for (int w = 0; w < TP_WAVES; w++) { const uint64_t x = s_t64[w]; if ((uint32_t)w < wave) off += x; tot += x; }
                    if (ny) {
                        const uint64_t start = carry + off + incl - val, end = start + val;
                        const uint32_t weight = (uint32_t)(end >> v_step_log) - (uint32_t)(start >> v_step_log);
                        if (weight < 1) badw = 1;
                        norm[s2] = (NormT)(int32_t)weight;
                    }
                    carry += mic_uniform(tot);
                }
                if (__syncthreads_or((int)badw)) rc2 = MICD_ERR_INTERNAL;
            }
            if (rc2 == MICD_OK && serial) {
                __syncthreads();
                if (tid == 0) s_misc[3] = (uint32_t)mic_normalize_count2(u.hist, u.norm, symbol_len, n, tl);
                __threadfence_block();
                __syncthreads();
                rc2 = (int)s_misc[3];
                if (rc2 == MICD_OK && (void *)norm != (void *)u.norm)
                    for (uint32_t s2 = tid; s2 < symbol_len; s2 += TP_THREADS) norm[s2] = (NormT)u.norm[s2];
            }
            if (rc2 != MICD_OK) { if (tid == 0) u.status = rc2; return; }
            route |= serial ? MIC_TBR_N2_SERIAL : MIC_TBR_N2_PAR;
        }
    }
    __threadfence_block();
    __syncthreads();
    MIC_STAMP_AT(u, 5);
    // ---- NCount header (one lane; fsecompressu16.go:191-289) ----------------------------------------
    int rc_par = MICD_ERR_UNSUPPORTED;
    if (u.blob_cap >= 6 + 16 && ((uintptr_t)u.blob & 3) == 0) {
        // scratch that tp_build only needs later: first_visit / cum_all hold the two per-symbol arrays; small alphabets
        // pack into visit_pos (LDS) and copy out, large ones pack straight into the blob (word-aligned 2 bytes ahead)
        uint32_t hdr = 0;
        if (sizeof(NormT) == 2)
            rc_par = tb_write_ncount_par(norm, symbol_len, tl, first_visit, cum_all, (uint32_t *)visit_pos, 0u, true, s_tmp,
                                         u.blob + 6, u.blob_cap - 6 - 8, &hdr);
        else
            rc_par = tb_write_ncount_par(norm, symbol_len, tl, first_visit, cum_all, (uint32_t *)(u.blob + 4), 16u, false, s_tmp,
                                         u.blob + 6, u.blob_cap - 6 - 8, &hdr);
        if (rc_par != MICD_ERR_UNSUPPORTED && tid == 0) { if (rc_par == MICD_OK) u.hdr_len = hdr; s_misc[3] = (uint32_t)rc_par; }
        __syncthreads();
    }
    route |= rc_par != MICD_ERR_UNSUPPORTED ? MIC_TBR_W_PAR : MIC_TBR_W_SERIAL;
    if (rc_par != MICD_ERR_UNSUPPORTED) {
    } else if (tid == 0) {
        int rc = MICD_OK;
        uint32_t hdr = 0;
        if (u.blob_cap < 6 + 8) rc = MICD_ERR_CAPACITY;
        else rc = mic_write_ncount(norm, symbol_len, tl, u.blob + 6, u.blob_cap - 6, &hdr);
        if (rc == MICD_OK) {
            u.hdr_len = hdr;
            for (int k = 0; k < 8; k++) u.blob[6 + hdr + k] = 0;      // k_enc_tans_wg ORs into the first stream word
        }
        s_misc[3] = (uint32_t)rc;
    }
    __threadfence_block();
    __syncthreads();
    if ((int)s_misc[3] != MICD_OK) { if (tid == 0) u.status = (int)s_misc[3]; return; }
    MIC_STAMP_AT(u, 6);
    if (RANS && u.nstates == 108) {
        // buildRansEncTable (ransu16.go:139-180): bias = cumulative frequency, positives in symbol order, then the
        // low-probability symbols; record = freq | k0 << 20 in tt_nb, bias in tt_find.  No state table.
        uint32_t carry_pos = 0, carry_low = 0;
        for (uint32_t base = 0; base < symbol_len; base += TP_THREADS) {
            const uint32_t s2 = base + tid;
            const int32_t v = (s2 < symbol_len) ? (int32_t)norm[s2] : 0;
            uint32_t tot;
            const uint32_t ex = tp_block_excl((v > 0 ? (uint32_t)v : 0u) | ((v == -1 ? 1u : 0u) << 20), s_tmp, &tot);
            if (s2 < symbol_len) first_visit[s2] = (IdxT)(v == -1 ? carry_low + (ex >> 20) : carry_pos + (ex & 0xFFFFF));
            carry_pos += tot & 0xFFFFF; carry_low += tot >> 20;
        }
        __syncthreads();
        if (carry_pos + carry_low != size) { if (tid == 0) u.status = MICD_ERR_INTERNAL; return; }
        for (uint32_t s2 = tid; s2 < symbol_len; s2 += TP_THREADS) {
            const int32_t v = (int32_t)norm[s2];
            if (v == 0) continue;
            const uint32_t freq = v > 0 ? (uint32_t)v : 1u;
            const uint32_t k0 = tl - mic_high_bits(freq);
            u.tt_nb[s2] = freq | (k0 << 20);
            u.tt_find[s2] = (int32_t)(v > 0 ? (uint32_t)first_visit[s2] : carry_pos + (uint32_t)first_visit[s2]);
        }
        if (tid == 0) { u.zero_bits = 0; u.tb_route = route | MIC_TBR_RANS; }
        return;
    }
    // ---- CTable: stateTable via the parallel spread, symbolTT per symbol ------------------------------
    TpScratch<NormT, IdxT> S;
    S.norm = norm; S.first_visit = first_visit; S.cum_all = cum_all; S.visit_pos = visit_pos;
    S.bitmap = bitmap; S.wprefix = wprefix; S.big_list = big_list; S.s_tmp = s_tmp;
    uint32_t *state_tab = u.state_tab;
    const int rc = tp_build(S, symbol_len, tl, [&](uint32_t p, uint32_t s, uint32_t r, uint32_t) {
        state_tab[(uint32_t)cum_all[s] + r] = size + p;                  // fsecompressu16.go:398-402
    });
    if (rc != MICD_OK) { if (tid == 0) u.status = rc; return; }
    uint32_t zb = 0;
    const uint32_t tlv = (tl << 16) - size;
    const int32_t large_limit = (int32_t)(size >> 1);
    for (uint32_t s = tid; s < symbol_len; s += TP_THREADS) {           // fsecompressu16.go:411-424
        const int32_t v = (int32_t)norm[s];
        if (v == 0) continue;
        const int32_t total = (int32_t)(uint32_t)cum_all[s];
        if (v > large_limit) zb = 1;
        if (v == -1 || v == 1) { u.tt_nb[s] = tlv; u.tt_find[s] = total - 1; }
        else {
            const uint32_t max_bits_out = tl - mic_high_bits((uint32_t)(v - 1));
            u.tt_nb[s] = (max_bits_out << 16) - ((uint32_t)v << max_bits_out);
            u.tt_find[s] = total - v;
        }
    }
    const int anyzb = __syncthreads_or((int)zb);
    if (tid == 0) { u.zero_bits = anyzb ? 1u : 0u; u.tb_route = route | (s_tmp[TP_WAVES] << 16); }   // (tp_build's nbig is still there)
    MIC_STAMP_AT(u, 7);
}

// C4K: the compact instance (two groups per CU: sixteen waves each, eight per SIMD, 64 VGPRs).  It is launched first, when it is
// launched at all (mic_launch_enc_tables), and builds nothing for a unit that is not its own; a unit that fails a histogram gate
// (USE_RLE, INCOMPRESSIBLE: known before the class is) gets its status, max_count and symbol_len from whichever instance scans it
// first, tb_inst stays 0 and the other instance skips it by its status.  The standard instance takes every unit that does not
// carry the compact one's mark.
template <bool C4K>
__global__ void __launch_bounds__(TP_THREADS, C4K ? 8 : 4) k_enc_tables_wg(MicUnit *units) {
    typedef TbLds<C4K> L;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    __shared__ uint32_t s_misc[8];
    MicUnit &u = units[blockIdx.x];
    if (u.status != MICD_OK) return;
    if (C4K ? u.nstates == 108 : u.tb_inst == MIC_TBI_C4K) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *s_tmp = (uint32_t *)(s_raw + L::TMP);
    // ---- histogram scan: symbolLen and maxCount (fsecompressu16.go:438-462) -------------------------
    uint32_t m = 0, sl = 0;
    const uint32_t hist_hi = min(u.tab_cap, (u.hist_hi >= 1 && u.hist_hi <= MIC_MAXSYM) ? u.hist_hi : MIC_MAXSYM + 1u);   // (the tokeniser's bound on what it counted)
    for (uint32_t i = tid; i < hist_hi; i += TP_THREADS) {
        const uint32_t c = u.hist[i];
        if (c) { m = max(m, c); sl = max(sl, i + 1); }
    }
    m = mic_wave_reduce_max(m); sl = mic_wave_reduce_max(sl);
    if (lane == 0) { s_tmp[wave] = m; s_tmp[16 + wave] = sl; }
    __syncthreads();
    if (tid == 0) {
        uint32_t mm = 0, ss = 0;
        for (int w = 0; w < TP_WAVES; w++) { mm = max(mm, s_tmp[w]); ss = max(ss, s_tmp[16 + w]); }
        const uint32_t n = u.ntok;
        int rc = MICD_OK;
        // gate order of FSECompressU16* (fse2state.go:23-42); the flavour's length gate is applied in k_enc_tans_wg
        // (a bare FSE call has no fallback chain: its own flavour's length gate comes before the histogram gates, fse8state.go:32-34)
        const uint32_t lanes0 = u.nstates == 108 ? 8u : (uint32_t)u.nstates;
        if (n <= 1 || (u.no_fallback && n <= lanes0 - 1)) rc = MICD_ERR_INCOMPRESSIBLE;
        else if (mm == n) rc = MICD_ERR_USE_RLE;
        else if (mm == 1 || mm < (n >> 15)) rc = MICD_ERR_INCOMPRESSIBLE;
        uint32_t tl = 0;
        if (rc == MICD_OK) tl = mic_optimal_table_log(n, ss, u.req_tl);
        if (C4K && rc == MICD_OK && !tb_is_c4k(ss, tl, u.nstates)) rc = MICD_ERR_UNSUPPORTED;   // (the standard instance's: nothing is written)
        else {
            u.max_count = mm; u.symbol_len = ss;
            if (rc == MICD_OK) { u.table_log = tl; u.tb_inst = C4K ? MIC_TBI_C4K : MIC_TBI_STD; }
            if (rc == MICD_OK && (1u << tl) > u.tab_cap) rc = MICD_INT_GROW;  // (tier 1: the table slabs hold 8192 states)
            if (rc != MICD_OK) u.status = rc;
        }
        s_misc[0] = (uint32_t)rc; s_misc[1] = tl; s_misc[4] = ss; s_misc[5] = n;
    }
    __syncthreads();
    if ((int)s_misc[0] != MICD_OK) return;
    const uint32_t tl = mic_uniform(s_misc[1]), symbol_len = mic_uniform(s_misc[4]), n = mic_uniform(s_misc[5]);
    uint32_t *bitmap = (uint32_t *)(s_raw + L::BITMAP), *wprefix = (uint32_t *)(s_raw + L::WPREF), *big = (uint32_t *)(s_raw + L::BIG);
    if (C4K || (symbol_len <= TB_SMALL_SYMS && tl <= TB_SMALL_TL)) {
        enc_tables_body<int16_t, uint16_t, !C4K>(u, (int16_t *)(s_raw + L::NORM), (uint16_t *)(s_raw + L::FIRST),
                                                 (uint16_t *)(s_raw + L::CUM), (uint16_t *)(s_raw + L::VISIT),
                                                 bitmap, wprefix, big, s_tmp, s_misc, n, symbol_len, tl);
    } else if (!C4K) {
        // HBM scratch: norm[] itself, cumul[] for the first visits, hist[] (dead after normalisation) for cum_all,
        // tab_sym[] for the visit sequence
        enc_tables_body<int32_t, uint32_t, true>(u, u.norm, (uint32_t *)u.cumul, (uint32_t *)u.hist, u.tab_sym,
                                                 bitmap, wprefix, big, s_tmp, s_misc, n, symbol_len, tl);
    }
}

// ------------------------------------------------------------------------------------------
template <typename NormT, typename IdxT, bool RANS>
__device__ void dec_tables_body(MicUnit &u, NormT *norm, IdxT *first_visit, IdxT *cum_all, uint16_t *visit_pos,
                                uint32_t *bitmap, uint32_t *wprefix, uint32_t *big_list, uint32_t *s_tmp,
                                uint32_t symbol_len, uint32_t tl, uint32_t flavour) {
    const uint32_t tid = threadIdx.x;
    const uint32_t size = 1u << tl;
    uint32_t *dt = u.tt_nb; uint16_t *ds = u.tab_sym;
    uint32_t bad = 0, zb = 0;
    uint32_t route = sizeof(NormT) == 2 ? MIC_TBR_SMALL : MIC_TBR_HBM;
    const int32_t large_limit = (int32_t)(size >> 1);
    for (uint32_t s = tid; s < symbol_len; s += TP_THREADS) if ((int32_t)norm[s] >= large_limit) zb = 1;   // fsedecompressu16.go:214-216
    if (RANS && flavour == 108) {
        // buildRansDecTable (ransu16.go:77-135): slots filled in symbol order, positives first, then the -1 symbols
        route |= MIC_TBR_RANS;
        uint32_t carry_pos = 0, carry_low = 0;
        for (uint32_t base = 0; base < symbol_len; base += TP_THREADS) {
            const uint32_t s = base + tid;
            const int32_t v = (s < symbol_len) ? (int32_t)norm[s] : 0;
            uint32_t tot;
            const uint32_t ex = tp_block_excl((v > 0 ? (uint32_t)v : 0u) | ((v == -1 ? 1u : 0u) << 20), s_tmp, &tot);
            if (s < symbol_len) { first_visit[s] = (IdxT)(v == -1 ? carry_low + (ex >> 20) : carry_pos + (ex & 0xFFFFF)); }
            carry_pos += tot & 0xFFFFF; carry_low += tot >> 20;
        }
        __syncthreads();
        if (carry_pos + carry_low != size) { if (tid == 0) u.status = MICD_ERR_CORRUPT; return; }
        for (uint32_t s = tid; s < symbol_len; s += TP_THREADS) {
            const int32_t v = (int32_t)norm[s];
            if (v == -1) { const uint32_t slot = carry_pos + (uint32_t)first_visit[s]; ds[slot] = (uint16_t)s; dt[slot] = 0u | (tl << 16); }
        }
        // positives: one thread per symbol walks its slots (long runs are rare and short relative to the table)
        for (uint32_t s = tid; s < symbol_len; s += TP_THREADS) {
            const int32_t v = (int32_t)norm[s];
            if (v <= 0) continue;
            const uint32_t a = (uint32_t)first_visit[s];
            for (uint32_t j = 0; j < (uint32_t)v; j++) {
                const uint32_t x_next = (uint32_t)v + j;
                const uint32_t nb = tl - mic_high_bits(x_next);
                ds[a + j] = (uint16_t)s; dt[a + j] = ((x_next << nb) - size) | (nb << 16);
            }
        }
    } else {
        TpScratch<NormT, IdxT> S;
        S.norm = norm; S.first_visit = first_visit; S.cum_all = cum_all; S.visit_pos = visit_pos;
        S.bitmap = bitmap; S.wprefix = wprefix; S.big_list = big_list; S.s_tmp = s_tmp;
        const int rc = tp_build(S, symbol_len, tl, [&](uint32_t p, uint32_t s, uint32_t r, uint32_t slots) {
            const uint32_t next = slots + r;                              // symbolNext[s]++ in table order, :244-246
            const uint32_t nb = tl - mic_high_bits(next);
            const uint32_t ns = (next << nb) - size;
            if (ns >= size || (ns == p && nb == 0)) bad = 1;              // :250-256
            ds[p] = (uint16_t)s; dt[p] = ns | (nb << 16);
        });
        if (rc != MICD_OK) { if (tid == 0) u.status = MICD_ERR_CORRUPT; return; }
    }
    const int anybad = __syncthreads_or((int)bad);
    const int anyzb = __syncthreads_or((int)zb);
    if (tid == 0) {
        if (anybad) u.status = MICD_ERR_CORRUPT;
        u.zero_bits = anyzb ? 1u : 0u;
        u.tb_route |= route | (flavour == 108 ? 0u : s_tmp[TP_WAVES] << 16);   // (beside k_dec_parse's bits; tp_build's nbig is still there)
    }
}

// Stream prefix + NCount parse (FSEDecompressU16Auto, fse2state.go:102-116; readNCount, fsedecompressu16.go:48-167).
// The parse is a serial bit reader, so it gets a kernel of its own with one wave per unit: all units of a
// launch parse side by side instead of one after the other under a 1024-thread group.  The head of the
// blob is staged in LDS (the reader hops byte-wise); counts go to the unit's HBM norm[] slab.
// Two classes: BIG = false stages 8 KiB and handles alphabets up to 8192 symbols (every depth <= 13: many groups per
// CU, 32 KiB of counts to clear); what it cannot take -- a longer header, a larger alphabet: 16-bit-depth frames --
// it leaves marked for BIG = true (40 KiB stage, all 65536 counts cleared).
#define DP_DEFER 0xDEFE7u      // in u.flavour: parse left to the BIG class
template <bool BIG>
__global__ void __launch_bounds__(64) k_dec_parse(MicUnit *units) {
    constexpr uint32_t DP_STAGE = BIG ? 40u * 1024u : 8u * 1024u;
    constexpr uint32_t DP_SYMS = BIG ? 65536u : 8192u;
    __shared__ __attribute__((aligned(16))) uint8_t s_in[DP_STAGE + 16];
    MicUnit &u = units[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint32_t len = u.comp_len;
    if (BIG && u.flavour != DP_DEFER) return;
    // the counts array starts out zero (the zero-runs of the header then cost nothing but a cursor move)
    if (u.norm) { uint4 *z = (uint4 *)u.norm; for (uint32_t i = tid; i < DP_SYMS / 4; i += 64) z[i] = make_uint4(0, 0, 0, 0); }
    if (u.comp_in) {
        const uint32_t nst = min(len, (uint32_t)DP_STAGE);
        const uint32_t head = (uint32_t)((16 - ((uintptr_t)u.comp_in & 15)) & 15);          // bytes up to 16-byte alignment
        for (uint32_t i = tid; i < min(head, nst); i += 64) s_in[i] = u.comp_in[i];
        if (nst > head) {
            const uint32_t nvec = (nst - head) / 16;
            typedef uint32_t v4 __attribute__((ext_vector_type(4)));
            typedef v4 v4u __attribute__((aligned(1)));
            for (uint32_t i = tid; i < nvec; i += 64) *(v4u *)(s_in + head + i * 16) = *(const v4 *)(u.comp_in + head + i * 16);
            for (uint32_t i = head + nvec * 16 + tid; i < nst; i += 64) s_in[i] = u.comp_in[i];
        }
    }
    __syncthreads();
    if (tid == 0) {
        u.status = MICD_OK; u.ntok = 0;
        int rc = MICD_OK;
        uint32_t flavour = 1, count = 0, off = 0, used = 0, symbol_len = 0, tl = 0;
        uint32_t win = 0, route = BIG ? MIC_TBR_P_BIG_STAGE : MIC_TBR_P_SMALL, defer = MIC_TBR_P_DEFER_TL;
        do {
            if ((u.mode == 0 && (u.w <= 0 || u.h <= 0)) || !u.comp_in) { rc = MICD_ERR_ARGS; break; }
            if (len >= 2 && s_in[0] == 0xFF) {
                if (s_in[1] == 0x84) flavour = 8;
                else if (s_in[1] == 0x08) flavour = 108;
                else if (s_in[1] == 0x04) flavour = 4;
                else if (s_in[1] == 0x02) flavour = 2;
            }
            // a WaveletV2 stream is decoded by FSEDecompressU16FourState and nothing else (waveletfsecompressu16.go:504): on the
            // device-resident path nobody has looked at the magic bytes yet
            if (u.walk_mode == 1 && flavour != 4) { rc = MICD_ERR_CORRUPT; break; }
            if (flavour != 1) {
                if (len < 6) { rc = MICD_ERR_CORRUPT; break; }
                count = (uint32_t)s_in[2] | ((uint32_t)s_in[3] << 8) | ((uint32_t)s_in[4] << 16) | ((uint32_t)s_in[5] << 24);
                off = 6;
                if (count > u.tok_cap) { rc = u.tier == 1 ? MICD_INT_GROW : MICD_ERR_CORRUPT; break; }   // (tier 1: a small token slab; tier 2 decides)
            }
            // (a table of more than 8192 states is the BIG class's whatever its alphabet -- the table slabs of this class's tier hold
            // 8192: a WaveletV2 stream, tableLog 16, was parsed half way here, 8192 of its ~16 k symbols, before it was handed over)
            if (!BIG && off < len && (uint32_t)(s_in[off] & 0xF) + MIC_MIN_TABLELOG > 13u) { rc = MICD_ERR_UNSUPPORTED; break; }
            // Parse from the staged bytes when that is certain to be identical: the whole blob is staged, or the
            // header ends well inside the stage; otherwise from HBM.
            // (the window reader may look 8 bytes past the bytes it is given: the stage is DP_STAGE + 16 bytes long)
            if (len <= DP_STAGE) {
                rc = mic_read_ncount<int32_t, true>(s_in + off, len - off, u.norm, &symbol_len, &tl, &used, DP_SYMS, (const uint32_t *)s_in, off, &win);
                defer = MIC_TBR_P_DEFER_SYMS;
            } else {
                rc = mic_read_ncount<int32_t, true>(s_in + off, DP_STAGE - off, u.norm, &symbol_len, &tl, &used, DP_SYMS, (const uint32_t *)s_in, off, &win);
                if (!(rc == MICD_OK && used + 8 < DP_STAGE - off)) {
                    if (!BIG) { rc = MICD_ERR_UNSUPPORTED; defer = MIC_TBR_P_DEFER_LEN; }
                    else {
                        for (uint32_t i = 0; i < 65536; i++) u.norm[i] = 0;    // (rare: header longer than the stage) start over from HBM
                        rc = mic_read_ncount<int32_t, true>(u.comp_in + off, len - off, u.norm, &symbol_len, &tl, &used, 65536u, nullptr, 0, &win);
                        route = MIC_TBR_P_BIG_HBM;
                    }
                }
            }
        } while (0);
        if (!BIG && rc == MICD_ERR_UNSUPPORTED) {
            if (u.tier == 1) { u.status = MICD_INT_GROW; return; }            // (more than 8192 symbols: the count slab is tier 1's)
            u.flavour = DP_DEFER; u.tb_route = defer; return;
        }
        if (rc == MICD_OK && (1u << tl) > u.tab_cap) rc = MICD_INT_GROW;       // (tier 1: the decode table slabs hold 8192 states)
        if (rc == MICD_OK) { u.flavour = flavour; u.count = count; u.symbol_len = symbol_len; u.table_log = tl; u.bits_off = off + used;
                            u.tb_route = (BIG ? u.tb_route : 0u) | route | (win ? MIC_TBR_P_WINDOW : 0u); }
        else u.status = rc;
    }
}

// (the parse has left the unit's class in its descriptor: each instance takes its own units; c4k_launched = 0: the compact
// instance is not in this chain and the standard one takes every unit)
template <bool C4K>
__global__ void __launch_bounds__(TP_THREADS, C4K ? 8 : 4) k_dec_tables_wg(MicUnit *units, int c4k_launched) {
    typedef TbLds<C4K> L;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    MicUnit &u = units[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    if (u.status != MICD_OK) return;                                      // k_dec_parse already failed this unit
    const uint32_t tl = u.table_log, symbol_len = u.symbol_len, flavour = u.flavour;
    if (C4K ? !tb_is_c4k(symbol_len, tl, flavour) : (c4k_launched && tb_is_c4k(symbol_len, tl, flavour))) return;
    if (tid == 0) u.tb_inst = C4K ? MIC_TBI_C4K : MIC_TBI_STD;
    int16_t *norm16 = (int16_t *)(s_raw + L::NORM);
    uint32_t *s_tmp = (uint32_t *)(s_raw + L::TMP);
    const bool small = C4K || (symbol_len <= TB_SMALL_SYMS && tl <= TB_SMALL_TL);
    if (small) for (uint32_t s2 = tid; s2 < symbol_len; s2 += TP_THREADS) norm16[s2] = (int16_t)u.norm[s2];
    __syncthreads();
    uint32_t *bitmap = (uint32_t *)(s_raw + L::BITMAP), *wprefix = (uint32_t *)(s_raw + L::WPREF), *big = (uint32_t *)(s_raw + L::BIG);
    if (small) {
        dec_tables_body<int16_t, uint16_t, !C4K>(u, norm16, (uint16_t *)(s_raw + L::FIRST), (uint16_t *)(s_raw + L::CUM),
                                                 (uint16_t *)(s_raw + L::VISIT), bitmap, wprefix, big, s_tmp, symbol_len, tl, flavour);
    } else if (!C4K) {
        // HBM scratch: cumul[] first visits, tt_find[] cum_all (not hist[]: the encode side keeps that slab zero between calls),
        // state_tab[] (u32, first half used as u16) visit sequence
        dec_tables_body<int32_t, uint32_t, true>(u, u.norm, (uint32_t *)u.cumul, (uint32_t *)u.tt_find, (uint16_t *)u.state_tab,
                                                 bitmap, wprefix, big, s_tmp, symbol_len, tl, flavour);
    }
}

void mic_launch_enc_tables(MicUnit *d_units, int n, hipStream_t stream, bool c4k) {
    static MicPerDeviceOnce once;
    once.run([] {
        (void)hipFuncSetAttribute((const void *)k_enc_tables_wg<true>, hipFuncAttributeMaxDynamicSharedMemorySize, TbLds<true>::BYTES);
        (void)hipFuncSetAttribute((const void *)k_enc_tables_wg<false>, hipFuncAttributeMaxDynamicSharedMemorySize, TbLds<false>::BYTES);
    });
    if (c4k) hipLaunchKernelGGL(k_enc_tables_wg<true>, dim3(n), dim3(TP_THREADS), TbLds<true>::BYTES, stream, d_units);
    hipLaunchKernelGGL(k_enc_tables_wg<false>, dim3(n), dim3(TP_THREADS), TbLds<false>::BYTES, stream, d_units);
}
void mic_launch_dec_tables(MicUnit *d_units, int n, hipStream_t stream, bool c4k) {
    static MicPerDeviceOnce once;
    once.run([] {
        (void)hipFuncSetAttribute((const void *)k_dec_tables_wg<true>, hipFuncAttributeMaxDynamicSharedMemorySize, TbLds<true>::BYTES);
        (void)hipFuncSetAttribute((const void *)k_dec_tables_wg<false>, hipFuncAttributeMaxDynamicSharedMemorySize, TbLds<false>::BYTES);
    });
    hipLaunchKernelGGL(k_dec_parse<false>, dim3(n), dim3(64), 0, stream, d_units);
    hipLaunchKernelGGL(k_dec_parse<true>, dim3(n), dim3(64), 0, stream, d_units);
    if (c4k) hipLaunchKernelGGL(k_dec_tables_wg<true>, dim3(n), dim3(TP_THREADS), TbLds<true>::BYTES, stream, d_units, 1);
    hipLaunchKernelGGL(k_dec_tables_wg<false>, dim3(n), dim3(TP_THREADS), TbLds<false>::BYTES, stream, d_units, c4k ? 1 : 0);
}
