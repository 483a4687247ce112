// mic_dev.h -- device-side data layout shared by the encode / decode kernels and the launcher.
//
// One "unit" is one independently coded stream of the reference: a PICS strip
// (parallelstrips.go:77-93), a MIC2 frame (multiframecompress.go:186-209) or a MIC3 plane
// (wsicompress.go:373-421).  The launcher fills an array of MicUnit in HBM; every kernel
// is launched over that array (blockIdx.x or blockIdx.y = unit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MIC_MAXSYM        65535u
#define MIC_MIN_TABLELOG  5      // fseu16.go:26
#define MIC_MAX_TABLELOG  16     // fseu16.go:23
#define MIC_DEF_TABLELOG  11     // fseu16.go:25
#define MIC_GAP_HDR_MAX   8195u      // 3 + 8192: the bitmap of a 65536-symbol alphabet bounds every map the encoder chooses
// MicUnit.gap_buf: tab_cap u16 (enc: compact index per token value, dec: the map's first tab_cap entries), then the encoder's
// mode || map bytes; mic_gap_stride(tab_cap) bytes per unit
__host__ __device__ inline uint32_t mic_gap_map_off(uint32_t tab_cap) { return 2u * tab_cap; }
__host__ __device__ inline uint32_t mic_gap_stride(uint32_t tab_cap) { return (2u * tab_cap + MIC_GAP_HDR_MAX + 255u) & ~255u; }

// status codes: keep in sync with include/mic_hip.h
#define MICD_OK                  0
#define MICD_ERR_ARGS           -1
#define MICD_ERR_USE_RLE        -3
#define MICD_ERR_CAPACITY       -5
#define MICD_ERR_CORRUPT        -6
#define MICD_ERR_INTERNAL       -8
#define MICD_ERR_UNSUPPORTED    -9
#define MICD_ERR_INCOMPRESSIBLE -10
#define MICD_ERR_MISMATCH      -12    // the verify calls: decoded pixels differ from the reference (mic_verify.hip; the host sets it)
#define MICD_INT_GROW           -21    // internal: a tier-1 slab would overflow; the host runs the batch again in tier 2 (never surfaces)
#define MICD_GAP_CHECK          -22    // internal: a gap-removal unit for k_dec_gap_check, the checking decode path (never surfaces)
// MicUnit.dec_kernel behind the 30 lane-per-state classes (1 .. 30)
#define MIC_DEC_BY_GL           31u
#define MIC_DEC_BY_SERIAL       32u
// MicUnit.split[0]: what a split instance of the two-state chain (k_dec_tans_ls_parts, mic_decode_ls.hip) made of the unit
#define MIC_SPLIT_NOT_TRIED     0u     // classified as before: not on a split list
#define MIC_SPLIT_DONE          1u     // all parts decoded and joined: split[1] = I_1, split[2] = W, ... (MicUnit.split below)
#define MIC_SPLIT_NOT_MET       2u     // fell back to the unsplit instance: two neighbouring parts did not meet inside the overlap
#define MIC_SPLIT_BAD_COUNT     3u     // fell back: the last part does not end with the stream's last symbol (cut or damaged stream)
#define MIC_SPLIT_NO_ROOM       4u     // fell back: a part does not fit its scratch region, or the first two meet behind the last whole chunk
#define MIC_SPLIT_STALLED       5u     // handed back by the eight-part instance: a chain wave and its partner wave gave each other up (a wait ran
                                       // into its bound: MicSplitCfg::partner_bound); nothing is wrong with the stream
// Which two-state tableLog-13 units are split, and how far the parts overlap.  Defaults below; a session's
// values come from mic_hip_debug_split_config.
struct MicSplitCfg {
    uint32_t min_tokens = 131072u;     // shorter units are not worth a second decoder's start-up
    uint32_t overlap = 32768u;         // W: symbols a part decodes before its state is taken as the meeting point (a multiple of 64)
    uint32_t min_bits16 = 144u;        // G: 16 x the mean bits per token from which on a wrong start is forgotten inside W
    uint32_t min_tokens4 = 262144u;    // units that pass the gate above and are at least this long go to the four-part instance
                                       // (the others to the two-part one); mic_hip_debug_split4_config sets it, mic_hip_debug_split_config does not
    uint32_t min_tokens8 = 393216u;    // ... and those of at least max(min_tokens8, min_tokens4) tokens to the eight-part instance, whose regions
                                       // hold a part's steps from W on only: break-even against four parts is about 5.3 W, twelve W is the
                                       // default; mic_hip_debug_split8_config sets it
    uint32_t partner_bound = 1u << 18; // eight parts: polls (about 400 cycles each) a chain wave waits for its partner wave before it gives the
                                       // wave's units up as MIC_SPLIT_STALLED (k_dec_tans_ls_parts<8>); mic_hip_debug_partner_config sets it
};
// MicUnit.enc_kernel: 1 + the bit index of the MIC_ENC_CLS_* class (mic_launch.h) whose k_enc_tans_wg instance gave the unit its tANS
// verdict (1 .. 7), or MIC_ENC_BY_SERIAL; MIC_ENC_HANDED is set beside it when the two-state instance had handed the unit over first
#define MIC_ENC_BY_SERIAL       8u
#define MIC_ENC_HANDED          0x100u
// MicUnit.tk_paths: routes of k_enc_tokens_wg (mic_encode.hip).  A pass is one walk over a symbol window: one per tile, two for a tile
// that holds an escape, one more for the flush; a wave-pass is one wave's share of it.
#define MIC_TKP_FAST            0      // passes that took the fast tile
#define MIC_TKP_REFUSED         1      // fast votes that were refused (each starts a cool-down)
#define MIC_TKP_ESC             2      // tiles that held an escape
#define MIC_TKP_GENERAL         3      // passes that took the general route (the flush included)
#define MIC_TKP_PERLANE         4      // wave-passes that wrote their boundary threads one position per lane
#define MIC_TKP_ROUND2          5      // ... of which needed a second round of eight threads
#define MIC_TKP_SERIAL          6      // wave-passes whose boundary threads (more than sixteen) walked their positions serially
#define MIC_TKP_PACKED          7      // thread-tiles whose eight symbols came from the packed residuals (symbol units: from the vector load)
#define MIC_TKP_KIND2           8      // thread-tiles that fetched pixel by pixel
#define MIC_TK_PATHS            9
// MicUnit.tb_route: which forks of the table stage (mic_tables.hip, mic_tables_par.h, mic_read_ncount) a unit took.  Lane 0 writes it
// next to the unit's other results.  A unit that fails in k_enc_tables_wg keeps 0; on decode a failing unit keeps what was stored
// before it failed (a P_DEFER_* bit from k_dec_parse<false>, the parse bits when k_dec_tables_wg refuses the counts): read it with the status.  The upper 16 bits hold tp_build's count of symbols
// of more than TP_SMALLV slots (0 on the rANS branch, which has no spread).  Predicted by tests/table_routes.py.
#define MIC_TBR_SMALL           (1u << 0)    // scratch class: 16-bit values in LDS (alphabet <= 8192 symbols, tableLog <= 13)
#define MIC_TBR_HBM             (1u << 1)    // scratch class: 32-bit values in the unit's HBM slabs
#define MIC_TBR_RANS            (1u << 2)    // the rANS table branch (flavour 108) instead of tp_build
// k_enc_tables_wg
#define MIC_TBR_PRIMARY         (1u << 3)    // the primary normaliser finished the unit
#define MIC_TBR_N2_PAR          (1u << 4)    // normalizeCount2, weights by the whole group
#define MIC_TBR_N2_UNIFORM      (1u << 5)    // ... its "uniform" second classification pass was taken (with N2_PAR or N2_SERIAL)
#define MIC_TBR_N2_SERIAL       (1u << 6)    // ... one of its two serial corner cases: mic_normalize_count2 on one lane
#define MIC_TBR_W_PAR           (1u << 7)    // header by tb_write_ncount_par
#define MIC_TBR_W_SERIAL        (1u << 8)    // header by mic_write_ncount on one lane
// k_dec_parse / k_dec_tables_wg (a deferred unit carries its P_DEFER_* bit and the P_BIG_* bit of the parse that finished it)
#define MIC_TBR_P_SMALL         (1u << 9)    // parsed by k_dec_parse<false> from its 8 KiB stage
#define MIC_TBR_P_DEFER_TL      (1u << 10)   // left to <true>: tableLog > 13
#define MIC_TBR_P_DEFER_LEN     (1u << 11)   // left to <true>: a blob longer than the stage whose header did not end 8 bytes inside it
#define MIC_TBR_P_DEFER_SYMS    (1u << 12)   // left to <true>: a wholly staged blob with more than 8192 symbols
#define MIC_TBR_P_BIG_STAGE     (1u << 13)   // parsed by k_dec_parse<true> from its 40 KiB stage
#define MIC_TBR_P_BIG_HBM       (1u << 14)   // parsed by k_dec_parse<true> starting over from HBM
#define MIC_TBR_P_WINDOW        (1u << 15)   // the window loop of mic_read_ncount read at least one field (clear: the byte-wise loop read them all)
// MicUnit.tb_inst: the instance of the table kernel that took the unit (mic_tables.hip).  A word of its own, not a seventeenth route
// bit: tb_route's upper half is the big-symbol count, and its value is compared as a whole with the model of tests/table_routes.py
#define MIC_TBI_STD             1u           // the standard instance: one work-group per CU, any alphabet, rANS, HBM scratch
#define MIC_TBI_C4K             2u           // the compact instance: tANS, at most 4096 symbols, tableLog <= 13; two work-groups per CU

// MicUnit.px_paths: which forks of the tokens-to-pixels stage a decode unit took (tests/test_gpu_px_seams.py)
#define MIC_PXP_PLAIN_TILE      (1u << 0)    // k_dec_pixels_wg: a tile without a delimiter, entered with marker state 0: no scan
#define MIC_PXP_SCAN_TILE       (1u << 1)    // ... a tile that took the marker scan
#define MIC_PXP_SCAN_ENTRY1     (1u << 2)    // ... and was entered with marker state 1 (its first symbol is the payload of the tile before's last)
#define MIC_PXP_TABLE_RELOAD    (1u << 3)    // ... the LDS segment table did not reach a tile's end: a second round of the r0 loop inside one tile
#define MIC_PXP_PREFETCH        (1u << 4)    // ... a tile took the symbols fetched while the tile before was scanned
#define MIC_PXP_ROW_GATHER      (1u << 8)    // k_dec_rows_tok: a row of up to eight pieces, gathered
#define MIC_PXP_ROW_PIECEWISE   (1u << 9)    // ... a row of nine pieces or more, copied piece by piece
#define MIC_PXP_ROW_ESCAPE      (1u << 10)   // ... a row with a delimiter: the marker scan over the row and its slack
#define MIC_PXP_ROW_REDO        (1u << 11)   // ... a row the 16-bit wrap-around fired in: done again lane by lane
// MicUnit.dec_stage: a decode unit's place in the chain behind the tANS kernels (DESIGN.md section 4 has the table).  Device code only;
// every enqueue starts at NONE (lay_out: MicUnit{}).  The chain's other two hand-off signals: ntok != 0 ("decoded"), and wv_slow.
enum MicStage : uint32_t {
    MIC_STAGE_NONE   = 0,   // headers not walked.  Set: k_dec_translate (walk error, or no frame), k_rle_walk_fix (refused).  Read: k_dec_pixels_wg, k_wv_scatter
    MIC_STAGE_SEGS   = 1,   // seg / nseg / nsym valid.  Set: MicRleWalk::finish (k_dec_tans_gl, k_dec_translate), k_rle_walk_fix.  Read: k_dec_rows_tok,
                            // k_dec_pixels_wg (skips its own walk), k_rle_walk_compact, k_wv_scatter
    MIC_STAGE_STATES = 2,   // tok (split units: and sym) holds tANS STATES.  Set: k_dec_tans_ls, k_dec_tans_ls_parts.  Read and replaced: k_dec_translate{,_wide}
    MIC_STAGE_PARTS  = 3,   // translated, headers left to the walk in parts (mode 1, walk_mode 1).  Set: k_dec_translate{,_wide}.  Read: k_rle_walk_parts, _fix (replaces it)
    MIC_STAGE_PIXELS = 4,   // px_out done.  Set: k_dec_rows_tok.  Read: k_dec_pixels_wg, k_dec_predict_rows (both skip the unit)
};

struct MicUnit {
    // ---- inputs ------------------------------------------------------------------
    const uint16_t *px_in;    // encode: source pixels (w*h u16)
    uint16_t       *px_out;   // decode: destination pixels
    const uint8_t  *comp_in;  // decode: compressed blob
    uint32_t        comp_len;
    int32_t         w, h;
    uint16_t        max_value;
    uint16_t        nstates;  // encode: requested flavour 1/2/4/8, 108 = rANS-8
    uint32_t        mode;     // 0 = frame (Delta+RLE around the FSE stage), 1 = bare FSE: px_in / px_out hold u16 symbols, w = count
    uint32_t        no_fallback; // 1 = FSECompressU16* semantics (no N -> ... -> 1 chain)
    uint32_t        req_tl;   // ScratchU16.TableLog of a bare FSE call (fseu16.go:101-102); 0 = the default 11
    uint32_t        pred;     // mode 0: 0 = avg(left, top) predictor, 1 = gradient-adaptive (deltagradrlecompressu16.go)
    uint32_t        tier;     // 1: the slabs below are the small ones -- crossing one of their capacities is MICD_INT_GROW, not an error
    uint32_t        tab_cap;  // entries of hist / norm / tt_* / state_tab / tab_sym (8192 or 65536)
    // ---- per-unit workspace (HBM) ------------------------------------------------
    uint16_t *tok;            // RLE token stream (encode: produced, decode: FSE output)
    uint32_t  tok_cap;
    uint32_t *hist;           // [65536] symbol histogram (fseu16.go:64)
    int32_t  *norm;           // [65536] normalised counts (fseu16.go:65)
    uint32_t *tt_nb;          // [65536] enc: symbolTT.deltaNbBits ; dec: dtab (newState | nbBits<<16)
    int32_t  *tt_find;        // [65536] enc: symbolTT.deltaFindState ; dec: symbolNext scratch
    uint32_t *state_tab;      // [65536] enc: stateTable
    uint16_t *tab_sym;        // [65536] enc: tableSymbol ; dec: symbol of each state
    int32_t  *cumul;          // [65538]
    uint8_t  *blob;           // encode: staging output (NCount + bitstream, 6-byte prefix first)
    uint32_t  blob_cap;
    uint2    *seg;            // decode: RLE segments {token index of the payload | same-run << 31, first symbol index}
    uint32_t  seg_cap;
    uint16_t *sym;            // decode: expanded delta-symbol stream; encode: per-token tANS states
    uint32_t  sym_cap;
    uint32_t *flags;          // decode: 1 bit per pixel, set = pixel stored raw behind an escape
    uint32_t  nseg;
    uint32_t  nsym;
    uint32_t  dec_stage;      // decode: how far the chain behind the tables has brought the unit (MIC_STAGE_* above)
    uint32_t  dec_thr;        // decode: delta threshold (1 << (depth-1)) - 1 of the stream's own max value
    uint32_t  walk_mode;      // decode, mode 1 units: 1 = the symbols are a length-prefixed RLE stream (WaveletV2): the translate kernels mark it
                              // MIC_STAGE_PARTS and k_rle_walk_* (mic_wavelet.hip) walk its headers in parts: seg / nseg / nsym,
                              // MIC_STAGE_SEGS, and in `flags` the segment that holds every 8192nd symbol
    uint32_t  wv_slow;        // WaveletV2: this frame takes the one-group kernels (escape words in its stream, or a stream the walker refused)
    uint32_t  wv_zmax;        // WaveletV2 encode: largest zigzag symbol of the frame
    uint32_t  hist_hi;        // encode: every token the tokeniser counted is below this (0: unknown -- all 65536 bins are scanned)
    // gap removal (CompressSingleFrameGapRemoval / DecompressSingleFrameGapRemoval, gapremovalcompressu16.go; mic_gap.hip)
    uint32_t  gap;            // 0: plain unit; 1: a gap-removal unit; 2: its tokens use the compact alphabet behind a map
    uint32_t  gap_hdr_len;    // encode: bytes of mode || map written in front of the FSE stream; decode: bytes skipped
    uint32_t  gap_nsym;       // decode: numSymbols of the map
    uint8_t  *gap_buf;        // mic_gap_stride(tab_cap) bytes: enc compact-index table / dec expand table, then enc mode || map
    // ---- results -----------------------------------------------------------------
    uint32_t ntok;            // number of u16 in tok
    uint32_t blob_len;
    int32_t  status;
    int32_t  nstates_used;
    uint32_t symbol_len;
    uint32_t max_count;
    uint32_t table_log;
    uint32_t zero_bits;
    uint32_t hdr_len;         // NCount header bytes
    uint32_t bits_off;        // decode: offset of the bitstream inside comp_in
    uint32_t count;           // decode: symbol count from the 6-byte prefix
    uint32_t flavour;         // decode: 1/2/4/8, 108 = rANS-8
    uint32_t packed_direct;   // encode: 1 = the bitstream goes straight to the packed buffer (k_enc_tans_pack); the blob holds only the framing
    uint32_t skip_pack;       // encode: 1 = the losing candidate of a PICA strip (k_pica_pick): k_scan_lens does not count it, the pack kernels leave it alone
    uint32_t dec_kernel;      // decode: which kernel ran the unit's tANS chain -- 1 + its class (mic_dec_cls) for k_dec_tans_ls,
                              // MIC_DEC_BY_GL for k_dec_tans_gl, MIC_DEC_BY_SERIAL for k_dec_tans_serial; 0: nobody (tests/test_gpu_decode_classes.py).  Cleared with the
                              // other results: every enqueue's lay_out() starts each descriptor again from MicUnit{}
    uint32_t dbg[16];         // MIC_STAMP builds: shader-clock ticks per kernel phase (tools/stamp_*.py)
    uint32_t tb_route;        // which forks of the table stage the unit took (MIC_TBR_*), nbig << 16; read by mic_hip_debug_tab_route,
                              // predicted by tests/table_routes.py
    uint32_t tk_paths[MIC_TK_PATHS];   // encode: which routes k_enc_tokens_wg took through the unit (MIC_TKP_*), written once next to ntok;
                              // read by mic_hip_debug_tok_paths, predicted by tests/tokeniser_paths.py
    uint32_t enc_kernel;      // encode: which kernel gave the unit's tANS stage its verdict, coded or refused (MIC_ENC_BY_SERIAL, MIC_ENC_HANDED
                              // above); 0: nobody -- the unit failed in front of the stage, or no launched instance matched it.  Thread 0
                              // writes it next to nstates_used / status; cleared with the other results (lay_out: MicUnit{})
    uint32_t enc_rounds;      // encode: fix-up rounds te_encode ran in the attempt that decided the unit (>= 1; 0: k_enc_tans_serial, or no
                              // walk ran).  Read by mic_hip_debug_enc_kernel, predicted by tests/tans_encode_model.py
    // ---- input, decode (WaveletV2 at reduced resolution, mic_wavelet.hip) -----------
    uint32_t sym_limit;       // 0: the whole stream.  Else the chain kernels that honour it decode only the first
                              // round_up(sym_limit, 128) symbols (whole 128-symbol chunks) and leave ntok < count: a PREFIX unit,
                              // whose bits behind the prefix are never read (no over-read check)
    // ---- result, decode (behind the inputs above: the older fields keep their offsets) -----
    uint32_t split[8];        // decode, a unit of a split instance of the two-state chain (k_dec_tans_ls_parts): 0 MIC_SPLIT_* outcome, 1 I_1
                              // (two parts: i_sync), 2 W (j_sync), 3 I_2, 4 I_3 (two parts: ~0, no such bound) -- tokens [I_p, I_p+1) are the
                              // states sym[(p - 1) R + W + i - I_p] until k_dec_translate has moved them, I_parts = count --, 5 R (tokens per
                              // scratch region), 6 the failing boundary (1 .. parts - 1: the join of parts p - 1 and p, parts: the stream's
                              // end, 0: none), 7 parts.  Read by mic_hip_debug_split and mic_hip_debug_split4, predicted by
                              // tests/tans_split_model.py.  Cleared with the other results
    uint32_t split_hi[4];     // ... of the eight-part instance (split[7] = 8): I_4 .. I_7, and its regions hold no dead steps -- tokens
                              // [I_p, I_p+1) are the states sym[(p - 1) R + i - I_p].  Read by mic_hip_debug_split8, predicted by
                              // tests/tans_split8_model.py
    uint32_t tb_inst;         // which instance of k_enc_tables_wg / k_dec_tables_wg took the unit (MIC_TBI_*; 0: neither -- the unit failed in
                              // front of the table stage).  Thread 0 writes it; on encode it is also what keeps the standard instance
                              // off a unit the compact one has built.  Read by mic_hip_debug_tab_inst.  Cleared with the other results
    uint32_t partner[4];      // decode, a unit the eight-part instance ran: 0 who did the per-chunk upkeep (0 the chain wave itself, 1 a partner
                              // wave), 1 chunks of the unit the partner served, 2 chunks the chain wave found its partner not ready for (the
                              // wave's count), 3 stalled (MIC_SPLIT_STALLED; kept when the four-part instance then takes the unit).  Read by
                              // mic_hip_debug_partner, predicted by tests/tans_partner_model.py.  Cleared with the other results
    uint32_t px_paths;        // decode: which forks the tokens-to-pixels kernel that made the unit's symbols or pixels took (MIC_PXP_* above): thread 0
                              // of k_dec_pixels_wg writes it once behind the tile loop, lane 0 of k_dec_rows_tok next to dec_stage (a unit it
                              // declines keeps the zero, and k_dec_pixels_wg's bits follow).  Read by mic_hip_debug_px_paths, predicted by
                              // tests/px_seam_streams.py.  Cleared with the other results
};
// a prefix unit: the tANS chain stopped at the ceiling (tANS yields symbols in forward order, so the ntok it decoded are exact)
__host__ __device__ inline bool mic_is_prefix(const MicUnit &u) { return u.sym_limit != 0 && u.ntok < u.count; }
// the symbols a chain kernel decodes of a unit: count, or the ceiling in whole 128-symbol chunks when that is less
__host__ __device__ inline uint32_t mic_sym_ceiling(const MicUnit &u, uint32_t count) {
    if (u.sym_limit == 0 || u.sym_limit > 0xFFFFFF00u) return count;
    const uint32_t c = (u.sym_limit + 127u) & ~127u;
    return c < count ? c : count;
}

// One image of a PICA sub-batch (mic_pica.hip): where its pixels, its row costs and its strip boundaries lie.
struct MicPicaImage {
    uint64_t px_off;          // first pixel, in u16 from the sub-batch's pixel buffer
    int32_t  w, h;
    int32_t  nstrips;         // 1 .. h (the host has clamped it, parallelstripsadaptive.go:61-66)
    uint32_t rows;            // h when the partition needs the row costs (1 < nstrips < h), else 0
    uint32_t row0;            // the image's first entry of the cost array (running sum of rows)
    uint32_t start0;          // the image's first entry of the boundary array (running sum of nstrips)
};

// A pointer read out of a MicUnit is "generic" to the compiler, and generic accesses are flat_load / flat_store: those count on
// lgkmcnt as well as on vmcnt, so every s_waitcnt lgkmcnt(0) -- there is one in front of every work-group barrier -- waits for the
// HBM loads and stores in flight (a prefetch issued before a barrier is no prefetch any more).  mic_g() states what every
// workspace pointer is: global memory (global_load / global_store: vmcnt only).
#define MIC_GLOBAL __attribute__((address_space(1)))
template <class T> using mic_gp = MIC_GLOBAL T *;
template <class T> __device__ __forceinline__ mic_gp<T> mic_g(T *p) { return (mic_gp<T>)p; }

// Phase stamps for diagnostic builds (EXTRA_FLAGS=-DMIC_STAMP); they compile to nothing otherwise.
#ifdef MIC_STAMP
#define MIC_STAMP_BEGIN() uint64_t _mic_t0 = __builtin_amdgcn_s_memtime()
#define MIC_STAMP_AT(u, k) do { const uint64_t _t = __builtin_amdgcn_s_memtime(); if (threadIdx.x == 0) (u).dbg[k] += (uint32_t)(_t - _mic_t0); _mic_t0 = _t; } while (0)
#else
#define MIC_STAMP_BEGIN() do { } while (0)
#define MIC_STAMP_AT(u, k) do { } while (0)

#endif

// A barrier across which threads of one work-group hand GLOBAL memory to each other where the order matters to something outside the
// group's own L1 -- the tANS encoder's plain stores of 64-bit units, then the atomic ORs other threads make into them (executed at L2).
// __syncthreads() / __threadfence_block() emit no wait for outstanding stores at work-group scope on gfx950 (the memory model leaves
// that order to the CU's L1, which is enough for loads, not for an L2 atomic that could overtake a store still in flight): the writers
// wait for their stores to be acknowledged, the readers drop their L1 lines.
#define MIC_GROUP_HANDOFF() do { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); \
                                 __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); } while (0)

__device__ __forceinline__ int mic_len16(uint32_t v) { return v ? 32 - __clz(v) : 0; }
// gradPredict (deltagradcompressu16.go:147-167): avg(W, N) + clamp((NE - NW) >> 3, +-(|W - NW| + |N - NW|) / 2); no gradient, no correction
__device__ __forceinline__ int32_t mic_grad_predict(int32_t w, int32_t n, int32_t nw, int32_t ne) {
    const int32_t lim = (int32_t)((__sad((unsigned)w, (unsigned)nw, 0u) + __sad((unsigned)n, (unsigned)nw, 0u)) >> 1);
    const int32_t corr = (ne - nw) >> 3;
    return ((w + n) >> 1) + min(max(corr, -lim), lim);
}
// the gradient-adaptive prediction of pixel (x, y) from a plain pixel array (deltagradrlecompressu16.go:36-53)
__device__ __forceinline__ int32_t mic_grad_predict_at(const uint16_t *px, int w, int x, int y) {
    const size_t idx = (size_t)y * (size_t)w + (size_t)x;
    if (y == 0) return x ? (int32_t)px[idx - 1] : 0;
    if (x == 0) return (int32_t)px[idx - (size_t)w];
    const int32_t nw = px[idx - (size_t)w - 1];
    return mic_grad_predict(px[idx - 1], px[idx - (size_t)w], nw, (x + 1 < w) ? (int32_t)px[idx - (size_t)w + 1] : nw);
}
// fseu16.go:170-172 -- Len32(v)-1, wraps to 0xFFFFFFFF for 0
__device__ __forceinline__ uint32_t mic_high_bits(uint32_t v) { return (uint32_t)(31 - __clz(v)) ; }
__device__ __forceinline__ uint32_t mic_table_step(uint32_t size) { return (size >> 1) + (size >> 3) + 3; }
