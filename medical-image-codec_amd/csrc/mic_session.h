// mic_session.h -- host-side session state shared by mic_api.hip and mic_api_ext.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <atomic>
#include <vector>

#include "../../include/mic_hip.h"
#include "mic_dev.h"
#include "mic_launch.h"
#include "mic_verify.h"

struct mic_hip_session;

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) {                                                           \
            if (getenv("MIC_HIP_DEBUG"))                                                  \
                fprintf(stderr, "mic_hip: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return _e == hipErrorOutOfMemory ? MIC_ERR_NOMEM : MIC_ERR_DEVICE;            \
        }                                                                                 \
    } while (0)

namespace micapi {

// No C++ exception crosses the C ABI: every extern "C" entry point is a function-try-block closed by MIC_ABI_CATCH.
// exception_code(): the status of the exception in flight (call it inside a catch block only).
inline int exception_code() {
    try { throw; } catch (const std::bad_alloc &) { return MIC_ERR_NOMEM; } catch (...) { return MIC_ERR_INTERNAL; }
}
#define MIC_ABI_CATCH catch (...) { return micapi::exception_code(); }

// little-endian fields of the container headers
inline void put_u32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
inline uint32_t get_u32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline void put_u64(uint8_t *p, uint64_t v) { put_u32(p, (uint32_t)v); put_u32(p + 4, (uint32_t)(v >> 32)); }
inline uint64_t get_u64(const uint8_t *p) { return (uint64_t)get_u32(p) | ((uint64_t)get_u32(p + 4) << 32); }

extern std::mutex g_mu;     // guards the device choice and the pool of default sessions (mic_api.hip)
extern int g_device;
int ensure_device();
int check_device(int device);      // MIC_OK when `device` exists and is gfx950 (cached per device)

// A session's stream.  MIC_HIP_SESSION_PRIO_CYCLE=1 (experiments): successive sessions get successive priority levels, i.e.
// hardware queues of their own -- the runtime keeps a queue per level, and streams of one level may share one.
inline hipError_t mic_stream_create(hipStream_t *st) {
    static const bool cycle = getenv("MIC_HIP_SESSION_PRIO_CYCLE") != nullptr;
    if (!cycle) return hipStreamCreate(st);
    static std::atomic<int> next{0};
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);                       // (lo is the numerically larger, least urgent one)
    const int span = lo - hi + 1, k = next.fetch_add(1) % (span > 0 ? span : 1);
    return hipStreamCreateWithPriority(st, hipStreamDefault, lo - k);
}

struct DevBuf {
    void *p = nullptr; size_t cap = 0;
    uint64_t gen = 0;                       // bumped by every (re)allocation: the contents are undefined from then on, whatever the address
    int reserve(size_t bytes) {
        if (bytes <= cap) return MIC_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 4096;
        gen++;
        HIP_TRY(hipMalloc(&p, want));
        cap = want;
        return MIC_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; gen++; }
};

// The host copy of a launch's unit descriptors, in pinned memory: the upload in front of every launch chain and the download of
// the results behind it are DMA transfers that really are asynchronous (a pageable vector cost ~0.1 ms of staging each way per call).
// Because the upload is asynchronous, the descriptors may not be rewritten while it is in flight: assign() waits for it.
// Only the session's chain protocol (lay_out / run_encode / run_decode) writes and uploads them.
struct PinnedUnits {
    MicUnit *data() { return p; }
    MicUnit &operator[](size_t i) { return p[i]; }
    const MicUnit &operator[](size_t i) const { return p[i]; }
    size_t size() const { return n; }
    void release() { if (inflight) (void)hipEventSynchronize(ev); inflight = false; if (p) (void)hipHostFree(p); p = nullptr; cap = n = 0; if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
private:
    friend struct ::mic_hip_session;
    MicUnit *p = nullptr; size_t cap = 0, n = 0;
    hipEvent_t ev = nullptr; bool inflight = false;
    int assign(size_t count, const MicUnit &v) {
        if (inflight) { (void)hipEventSynchronize(ev); inflight = false; }
        if (count > cap) {
            if (p) (void)hipHostFree(p);
            p = nullptr; cap = 0;
            const size_t want = count + count / 4 + 16;
            HIP_TRY(hipHostMalloc((void **)&p, want * sizeof(MicUnit), hipHostMallocDefault));
            cap = want;
        }
        for (size_t i = 0; i < count; i++) p[i] = v;
        n = count;
        return MIC_OK;
    }
    int upload(void *d_dst, size_t count, hipStream_t stream) {
        HIP_TRY(hipMemcpyAsync(d_dst, p, sizeof(MicUnit) * count, hipMemcpyHostToDevice, stream));
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ev, stream));
        inflight = true;
        return MIC_OK;
    }
};

// a small pinned array the device writes results into (offsets of the packed streams)
struct PinnedU64 {
    uint64_t *p = nullptr; size_t cap = 0;
    int reserve(size_t count) {
        if (count <= cap) return MIC_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        const size_t want = count + count / 4 + 64;
        HIP_TRY(hipHostMalloc((void **)&p, want * sizeof(uint64_t), hipHostMallocDefault));
        cap = want;
        return MIC_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

constexpr size_t kSym = 65536;

// Two tiers of per-unit slabs.  Tier 2 is the worst case: two tokens per pixel (every pixel an escape), a 65536-symbol alphabet,
// a segment per token pair -- 42 bytes per pixel + 1.66 MB of tables.  Tier 1 is what well-formed data needs: one token per
// pixel and an eighth, tables for 8192 symbols / tableLog 13, a segment per eight pixels -- 7 bytes per pixel + 0.2 MB.  The unit
// codec runs in tier 1 first; a kernel that would cross a tier-1 capacity marks its unit MICD_INT_GROW and the batch is run
// again in tier 2 (session_*_finish), so results never depend on the tier.
inline size_t tok_cap_for(size_t px) { return 4 * px + 16; }                                  // tier 2 (and the legit bound of a stream's token count)
inline size_t tok_cap_tier(size_t px, int tier) { return tier == 1 ? px + px / 8 + 4096 : tok_cap_for(px); }
inline size_t blob_cap_tok(size_t tokc) { return 8 + 131080 + 2 * tokc + 16; }
inline size_t blob_cap_for(size_t px) { return blob_cap_tok(tok_cap_for(px)); }
inline size_t seg_cap_tier(size_t px, int tier) { return tier == 1 ? px / 8 + 1024 : 2 * px + 8; }
inline size_t tab_syms_tier(int tier) { return tier == 1 ? 8192 : 65536; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace micapi
using namespace micapi;

struct mic_hip_wsi_store;                       // MIC3 store of a device-resident slide (mic_api_ext.hip)
void mic_wsi_store_free(mic_hip_wsi_store *w);
struct mic_hip_tile_cache;                      // MIC3 tile cache (mic_tile_cache.h)
void mic_tile_cache_detach(mic_hip_tile_cache *c, uint64_t owner);

struct mic_hip_session {
    int device = 0;                         // the HIP device this session's stream and workspace live on (mic_hip_session_create_on)
    int max_units = 0; size_t max_px = 0;   // shape of the current workspace layout (see ensure)
    int tier = 2;                           // tier of the current layout
    bool force_big = false;                 // a batch of this session needed tier 2: later ones start there ...
    int calm_batches = 0;                   // ... until kTierCalm batches in a row would have fitted tier 1 (tier_review, mic_api.hip):
    bool shrink_pending = false;            //     set there; the next tier-1 layout then starts from released slabs
    static constexpr int kTierCalm = 8;     //     the session goes back to the small slabs and gives the large ones' memory back
    // what a tier-1 launch chain needs to be run again in tier 2 (session_*_finish)
    struct Retry { int kind = 0; bool pairs = false; const void *d_in = nullptr; void *d_out = nullptr; std::vector<mic_hip_unit> units; std::vector<uint64_t> begins, ends; } retry;
    hipStream_t stream = nullptr;
    // Entry points may be called from any OS thread (cgo: any goroutine's thread), and a process may hold sessions on several
    // devices: every public call makes the session's device the calling thread's current one first.
    int activate() { return hipSetDevice(device) == hipSuccess ? MIC_OK : MIC_ERR_DEVICE; }
    DevBuf units, cls, tok, hist, norm, tt_nb, tt_find, state_tab, tab_sym, cumul, blob, packed, offsets, seg, sym, flags;
    DevBuf gap;                            // gap-removal units' map slabs (mic_gap_stride(tab_syms) each), reserved by the first batch that has one
    DevBuf io_px, io_comp;                 // staging for the host-pointer entry points
    DevBuf io_px2, io_comp2, packed2;      // their second halves: sub-batch k + 1 comes up while k is coded and k - 1 goes down (mic_host_io.hip)
    DevBuf pica_tab, pica_cost, pica_starts;   // PICA: a sub-batch's image table, row costs and strip boundaries (mic_pica.hip)
    PinnedU64 pica_pin[2];                 // ... and the host's copy of table + boundaries, one per staging half
    DevBuf wv_a, wv_b;                     // WaveletV2 coefficient planes (int32, two per frame of the batch)
    DevBuf wv_tab_enc, wv_tab_dec;         // WaveletV2: a launch chain's frame records and work records (mic_wavelet.hip), encode's and decode's
    struct WvTabHeld { std::vector<uint8_t> key; std::vector<uint32_t> spans; uint64_t gen = ~0ull; } wv_tab_held[2];   // ... and what each holds: the frame records it was built from, its work lists, the allocation
    mic_hip_wsi_store *wsi = nullptr;      // mic_hip_session_wsi_*: coded planes of a slide, on the device
    DevBuf wsi_planes, wsi_stats, wsi_payload, wsi_recs; std::vector<DevBuf> wsi_pyr;
    mic_hip_tile_cache *tile_cache = nullptr; uint64_t tile_owner = 0;   // mic_hip_session_set_tile_cache: the cache of decoded tiles the store's patch calls use, and the store generation's owner number in it
    DevBuf pieces;                         // patch and crop calls: the call's piece list (GatherPiece, mic_pieces.h; MIC2 temporal: its footprints)
    DevBuf crop_stage;                     // MIC2 crops into a typed tensor: the u16 tensor the temporal volumes' running sums live in (mic_mic2_crops.hip)
    DevBuf wsi_stage;                      // MIC3 scaled patches: a group's native source rectangles, its patch records and the affine table (mic_api_ext.hip)
    DevBuf wsi_fills;                      // MIC3 decode: a slab's constant-plane spans (mic_api_ext.hip)
    std::vector<uint8_t> wsi_host_bytes;   // MIC3 patches from blobs: a sub-batch's stream bytes on their way up; kept, so that a loop of calls touches the same pages
    DevBuf rgb_planes, rgb_aux;            // RGB batches: a sub-batch's YCoCg-R planes; its tables, statistics and records (mic_rgb_batch.hip)
    DevBuf rgb_payload, rgb_payload2;      // ... and its assembled blobs: two halves, one goes down while the other is written
    DevBuf mic2_files, mic2_payload;       // mic_hip_session_mic2_encode: the call's MIC2 files back to back; the streams of its sub-batches until they are assembled (mic_mic2_batch.hip)
    PinnedU64 rgb_pin;                     // ... the host's copy of the plane statistics / the blob heads
    DevBuf verify_px;                      // mic_hip_session_verify / _encode_verified: the pixels the checked streams decode to (empty until the first such call)
    DevBuf verify_tab;                     // the digest kernels' unit records, chunk table, chunk registers and per-unit results (mic_verify.h)
    std::vector<uint8_t> verify_up; std::vector<uint64_t> verify_down;   // ... their host copies on the way up and down
    std::map<uint64_t, uint32_t> verify_init;                             // ... and 0xFFFFFFFF * x^(8 * bytes) per unit size seen (the CRC's init, carried to the unit's end)
    PinnedUnits h_units;
    std::vector<uint64_t> h_off;
    // what an enqueue has already put behind its chain (session_*_finish then only synchronises): the read-back of the descriptors;
    // for encode also scan + pack into `packed` (capacity pack_cap at that time) and the read-back of the offsets into pin_off
    bool readback_queued = false, pack_queued = false;
    size_t pack_cap = 0, pack_hint = 0;           // pack_hint: bytes the session's last batch packed to
    PinnedU64 pin_off;
    int n_last = 0;
    bool learn_decode = false, learn_encode = false;   // the chain in flight was launched under the session's class masks: finish updates them
    int variant = 0;                        // launch flags (MIC_VARIANT_GRAD is OR-ed in per call)
    // Kernel classes this session's last batches used (mic_launch.h: launch masks): age[c] = batches since class c was last seen;
    // a class is launched while its age is below kClsKeep.  Nothing seen yet: everything is launched.
    static constexpr uint8_t kClsKeep = 8;
    struct ClsMemory {
        uint8_t age[32]; bool any = false;
        ClsMemory() { for (uint8_t &a : age) a = 255; }
        uint32_t mask() const { if (!any) return ~0u; uint32_t m = 0; for (int c = 0; c < 32; c++) if (age[c] < kClsKeep) m |= 1u << c; return m; }
        void learn(uint32_t seen) { any = true; for (int c = 0; c < 32; c++) age[c] = ((seen >> c) & 1u) ? 0 : (uint8_t)std::min<int>(age[c] + 1, 255); }
    } dec_classes, enc_classes;
    MicSplitCfg split_cfg;                  // which two-state units the split decode instance takes (mic_hip_debug_split_config)
    // The per-unit 65536-bin histograms are ZERO between calls: the encode chain leaves them so (k_enc_hist_clean re-zeroes what a
    // unit's tokeniser counted), and nothing else writes them.  hist_zero_units = leading unit slabs known to be zero (0 after a
    // reallocation, after a failed launch).  The invariant is tied to the ALLOCATION (DevBuf::gen),
    // not to the address: hipFree + a larger hipMalloc may hand the same address back with undefined contents.
    uint64_t hist_zero_gen = ~0ull; size_t hist_zero_units = 0;
    MicTimer timer;
    std::vector<std::string> t_names; std::vector<float> t_ms;
    size_t tok_stride = 0, blob_stride = 0, seg_stride = 0, sym_stride = 0, flag_stride = 0;

    size_t tab_syms = kSym;                  // symbols / states the table slabs of the current layout hold per unit
    int ensure(int n, size_t px, int want_tier = 2) {
        if (!stream) HIP_TRY(mic_stream_create(&stream));
        // The workspace takes the shape of the current call (n units of up to px pixels, in the tier asked for); buffers only ever
        // grow.  Sizing for max(n) x max(px) over a session's history would ask for the bounding box of unrelated calls (one
        // 4-megapixel wavelet frame, then 3000 WSI planes of 256 x 256).
        if (n == max_units && px == max_px && want_tier == tier) return MIC_OK;
        // From here on the layout is in flux: a reservation that fails half way (DevBuf::reserve frees before it allocates) must not
        // leave the old shape key standing over new strides and freed slabs -- the next call of the old shape would take the early
        // return above and hand the kernels null or short slabs.  The key is cleared first and set again only when every slab stands.
        // (a session also goes from a tier-2 layout to a tier-1 one when its caller alternates between paths -- a WaveletV2 or pyramid
        // call lays out in tier 2, the unit codec in tier 1: that is no reason to give memory back, it would be bought again at once)
        const bool back_to_small = shrink_pending && want_tier == 1;
        if (back_to_small) shrink_pending = false;
        max_units = 0; max_px = 0; tier = 0;
        if (back_to_small) {                                            // the worst-case slabs go back to the device: reserve() only ever grows
            DevBuf *slabs[] = { &tok, &hist, &norm, &tt_nb, &tt_find, &state_tab, &tab_sym, &cumul, &blob, &seg, &sym, &flags };
            for (DevBuf *b : slabs) b->release();
            hist_unknown();
        }
        int nn = n; size_t pp = px;
        const size_t tokc = tok_cap_tier(pp, want_tier), ts = tab_syms_tier(want_tier);
        const size_t tok_s = align_up(tokc * 2, 256);
        const size_t blob_s = align_up(blob_cap_tok(tokc), 256);   // (te_encode's bit grid starts (6 + hdr_len) & 15 bytes into its 16-byte unit because of this
                                                                   // alignment: tests/tans_encode_model.py, STAGING_ALIGN, aims streams at the grid's 64-bit units with it)
        const size_t seg_s = align_up(seg_cap_tier(pp, want_tier) * 8, 256);
        const size_t sym_s = align_up((tokc + 64) * 2, 256);       // + a block: the tANS encoder rounds its per-token states up to 32
        const size_t flag_s = align_up(pp / 8 + 16, 256);          // + the predictor's 3-word read at the last pixel
        const int rc = [&]() -> int {
            int r;
            if ((r = units.reserve(sizeof(MicUnit) * (size_t)nn))) return r;
            if ((r = cls.reserve(4 * MIC_CLS_INTS(nn)))) return r;
            if ((r = tok.reserve(tok_s * (size_t)nn))) return r;
            if ((r = hist.reserve(ts * 4 * (size_t)nn))) return r;
            if ((r = norm.reserve(ts * 4 * (size_t)nn))) return r;
            if ((r = tt_nb.reserve(ts * 4 * (size_t)nn))) return r;
            if ((r = tt_find.reserve(ts * 4 * (size_t)nn))) return r;
            if ((r = state_tab.reserve(ts * 4 * (size_t)nn))) return r;
            if ((r = tab_sym.reserve(ts * 2 * (size_t)nn))) return r;
            if ((r = cumul.reserve((ts + 64) * 4 * (size_t)nn))) return r;
            if ((r = blob.reserve(blob_s * (size_t)nn))) return r;
            if ((r = offsets.reserve(8 * ((size_t)nn + 1)))) return r;
            if ((r = seg.reserve(seg_s * (size_t)nn))) return r;
            if ((r = sym.reserve(sym_s * (size_t)nn))) return r;
            return flags.reserve(flag_s * (size_t)nn);
        }();
        if (rc) { hist_unknown(); return rc; }             // (whatever the histogram slab holds now, nothing of it is known to be zero)
        if (ts != tab_syms) hist_unknown();                // (the histogram slabs are laid out anew: nothing is known to be zero)
        tok_stride = tok_s; blob_stride = blob_s; seg_stride = seg_s; sym_stride = sym_s; flag_stride = flag_s;
        max_units = nn; max_px = pp; tier = want_tier; tab_syms = ts;
        return MIC_OK;
    }
    // ---- the launch-chain protocol: every kernel chain over unit descriptors goes through these three ----------------------------
    // lay_out(): the workspace takes the shape of n units of up to px pixels and the host descriptors 0 .. n-1 are reset and pointed
    // at their slabs, capacities set to the slabs' sizes.  The caller then fills in its own fields of h_units[i] -- a capacity
    // override (a frame's own tok_cap, a stream's sym_cap) included, which therefore always comes after the slab's -- and runs the chain.
    // want_tier: the frame-unit codec starts in tier 1 and runs again in tier 2 (session_*_finish).  The paths that lay out symbol
    // units themselves (bare FSE, MIC2 temporal residuals, WaveletV2) have no second run and take tier 2, the worst case; tier_review
    // (mic_api.hip) leaves their batches (mode != 0) out of its count for that reason.
    int lay_out(int n, size_t px, int want_tier = 2) {
        int rc = ensure(n, px, want_tier);                              // (before anything points into a slab)
        if (rc || (rc = h_units.assign((size_t)n, MicUnit{}))) return rc;   // (waits for the previous chain's upload)
        for (int i = 0; i < n; i++) fill_workspace(h_units[(size_t)i], i);
        return MIC_OK;
    }
    // run_encode / run_decode(launch): the laid-out descriptors go up, the slabs are put in the state the chain assumes, `launch()`
    // enqueues the kernels on `stream` -- mic_launch_encode / mic_launch_decode with the path's own kernels in front of or behind it, in
    // the caller's order; every launch that `timer` is to see belongs in there -- and the chain is the session's current one:
    // session_*_finish reads it back.  Anything the caller queues behind the chain (pack, read-back) and the flags that say so
    // (readback_queued, pack_queued, learn_*) come AFTER the call returns: the call clears them.
    template <class F> int run_encode(F &&launch) {
        return run_chain(true, false, launch);
    }
    // The escape-flag slab (a bit per pixel "stored raw behind an escape", mic_decode_px.hip) is OR-ed into by the pixel kernels, so
    // units that reach them -- frames, mode 0 -- need it zero: Clear.  Symbol units (mode 1 / 3: bare FSE, temporal residuals,
    // WaveletV2) stop at tokens or symbols and never read it, and k_rle_walk_compact uses it as scratch: Idle, no memset.  A batch that
    // may hold a frame among its symbol units (MIC2 temporal: unit 0 of the first sub-batch) is Clear.
    enum class FlagSlab { Clear, Idle };
    template <class F> int run_decode(FlagSlab flag_slab, F &&launch) {
        return run_chain(false, flag_slab == FlagSlab::Clear, launch);
    }

private:
    template <class F> int run_chain(bool encode, bool clear_flags, F &&launch) {
        const int n = (int)h_units.size();
        int rc = h_units.upload(units.p, (size_t)n, stream);
        if (rc || (encode && (rc = prepare_hist(n)))) return rc;
        if (clear_flags) HIP_TRY(hipMemsetAsync(flags.p, 0, flag_stride * (size_t)n, stream));
        timer.reset(stream);                                            // (in front of the first timed kernel)
        launch();
        if (hipGetLastError() != hipSuccess) { if (encode) hist_unknown(); return MIC_ERR_DEVICE; }   // (whatever a chain that failed left in its histograms)
        // the chain over n units is enqueued; nothing is queued behind it yet
        n_last = n; readback_queued = false; pack_queued = false; learn_decode = learn_encode = false;
        return MIC_OK;
    }
    int prepare_hist(int n) {
        if (hist.gen != hist_zero_gen) { hist_zero_gen = hist.gen; hist_zero_units = 0; }
        if ((size_t)n > hist_zero_units) {
            HIP_TRY(hipMemsetAsync((char *)hist.p + tab_syms * 4 * hist_zero_units, 0, tab_syms * 4 * ((size_t)n - hist_zero_units), stream));
            hist_zero_units = (size_t)n;
        }
        return MIC_OK;
    }
    void hist_unknown() { hist_zero_units = 0; }
    void fill_workspace(MicUnit &u, int i) {
        const size_t ts = tab_syms;
        u.tier = (uint32_t)tier; u.tab_cap = (uint32_t)ts;
        u.tok = (uint16_t *)((char *)tok.p + tok_stride * (size_t)i);
        u.tok_cap = (uint32_t)std::min<size_t>(tok_cap_tier(max_px, tier), 0xFFFFFFF0u);
        u.hist = (uint32_t *)hist.p + ts * (size_t)i;
        u.norm = (int32_t *)norm.p + ts * (size_t)i;
        u.tt_nb = (uint32_t *)tt_nb.p + ts * (size_t)i;
        u.tt_find = (int32_t *)tt_find.p + ts * (size_t)i;
        u.state_tab = (uint32_t *)state_tab.p + ts * (size_t)i;
        u.tab_sym = (uint16_t *)tab_sym.p + ts * (size_t)i;
        u.cumul = (int32_t *)cumul.p + (ts + 64) * (size_t)i;
        u.blob = (uint8_t *)blob.p + blob_stride * (size_t)i;
        u.blob_cap = (uint32_t)std::min<size_t>(blob_cap_tok(tok_cap_tier(max_px, tier)), 0xFFFFFFF0u);
        u.seg = (uint2 *)((char *)seg.p + seg_stride * (size_t)i);
        u.seg_cap = (uint32_t)std::min<size_t>(seg_cap_tier(max_px, tier), 0xFFFFFFF0u);
        u.sym = (uint16_t *)((char *)sym.p + sym_stride * (size_t)i);
        u.sym_cap = (uint32_t)std::min<size_t>(tok_cap_tier(max_px, tier) + 64, 0xFFFFFFF0u);
        u.flags = (uint32_t *)((char *)flags.p + flag_stride * (size_t)i);
    }
public:
    size_t reserved_bytes() const {
        const DevBuf *all[] = { &units, &gap, &cls, &tok, &hist, &norm, &tt_nb, &tt_find, &state_tab, &tab_sym, &cumul, &blob, &packed, &offsets, &seg, &sym, &flags, &io_px, &io_comp, &io_px2, &io_comp2, &packed2, &pica_tab, &pica_cost, &pica_starts, &wv_a, &wv_b, &wv_tab_enc, &wv_tab_dec, &wsi_planes, &wsi_stats, &wsi_payload, &wsi_recs, &pieces, &crop_stage, &wsi_stage, &wsi_fills, &rgb_planes, &rgb_aux, &rgb_payload, &rgb_payload2, &mic2_files, &mic2_payload, &verify_px, &verify_tab };
        size_t t = 0;
        for (const DevBuf *b : all) t += b->cap;
        return t;
    }
    void release() {
        DevBuf *all[] = { &units, &gap, &cls, &tok, &hist, &norm, &tt_nb, &tt_find, &state_tab, &tab_sym, &cumul, &blob, &packed, &offsets, &seg, &sym, &flags, &io_px, &io_comp, &io_px2, &io_comp2, &packed2, &pica_tab, &pica_cost, &pica_starts, &wv_a, &wv_b, &wv_tab_enc, &wv_tab_dec, &wsi_planes, &wsi_stats, &wsi_payload, &wsi_recs, &pieces, &crop_stage, &wsi_stage, &wsi_fills, &rgb_planes, &rgb_aux, &rgb_payload, &rgb_payload2, &mic2_files, &mic2_payload, &verify_px, &verify_tab };
        for (DevBuf *b : all) b->release();
        for (DevBuf &b : wsi_pyr) b.release();
        wsi_pyr.clear();
        if (wsi) { mic_wsi_store_free(wsi); wsi = nullptr; }
        if (tile_cache) { mic_tile_cache_detach(tile_cache, tile_owner); tile_cache = nullptr; }
        h_units.release(); pin_off.release(); pica_pin[0].release(); pica_pin[1].release(); rgb_pin.release();
        readback_queued = pack_queued = false;
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
        timer.destroy();
    }
};


namespace micapi {
// A session of the default pool, held by the calling thread for the duration of a host-pointer entry point (mic_api.hip).
struct DefaultLease {
    mic_hip_session *s = nullptr; bool held = false;
    int acquire(int device = -1);   // MIC_OK, or why there is no device; blocks while every pooled session of the device is out.
                                    // device: one of mic_hip_set_devices' list (-1: its first -- the default)
    ~DefaultLease();
    DefaultLease() = default;
    DefaultLease(const DefaultLease &) = delete;
    DefaultLease &operator=(const DefaultLease &) = delete;
};
mic_hip_session *cur_default();     // the session the calling thread holds
std::vector<int> default_devices(); // the devices of the host-pointer entry points (mic_hip_set_devices), the default first
// pica_pairs: units 2 p and 2 p + 1 are the two candidates of one PICA strip -- k_pica_pick runs between the chain and the pack, the
// loser is not packed and takes no room in the offsets session_encode_finish returns (its status is still reported)
int session_encode_enqueue(mic_hip_session *s, const uint16_t *d_pixels, const mic_hip_unit *units, int n, bool pica_pairs = false);
int session_encode_finish(mic_hip_session *s, const uint8_t **d_blobs, uint64_t *h_offsets, int32_t *h_status, int32_t *h_nstates);
int session_decode_enqueue(mic_hip_session *s, const uint8_t *d_blobs, const uint64_t *h_offsets,
                           const mic_hip_unit *units, int n, uint16_t *d_pixels_out);
// the same with an explicit byte range [begins[i], ends[i]) of d_base per unit (streams that do not lie back to back)
int session_decode_enqueue_spans(mic_hip_session *s, const uint8_t *d_base, const uint64_t *begins, const uint64_t *ends,
                                 const mic_hip_unit *units, int n, uint16_t *d_pixels_out);
int session_decode_finish(mic_hip_session *s, int32_t *h_status);
// Digests and compares (mic_verify.hip).  session_digest_run: res[i].crc32 = the CRC-32 of unit i of d_ref; with d_dec, units whose
// compare[i] is set (null: all) are compared with their counterparts in d_dec (same px_offset): res[i].mismatches / first_mismatch,
// 0 / -1 for the others.  res[i].status is left alone.  Complete on return.
int session_digest_run(mic_hip_session *s, const uint16_t *d_ref, const uint16_t *d_dec, const mic_hip_unit *units, int n,
                       const uint8_t *compare, mic_hip_verify_result *res);
// The streams d_base + begins[i] .. ends[i] decoded into the session's scratch and compared with d_ref: res[i] in full.  skip
// (nullable): units whose skip[i] is not MIC_OK are not decoded -- res[i].status = skip[i], the CRC is still taken.
int session_verify(mic_hip_session *s, const uint8_t *d_base, const uint64_t *begins, const uint64_t *ends, const mic_hip_unit *units, int n,
                   const uint16_t *d_ref, const int32_t *skip, mic_hip_verify_result *res);
size_t unit_ws_bytes(size_t px);
size_t unit_ws_bytes_tier(size_t px, int tier);
size_t batch_units_for(size_t px, size_t mult, size_t extra = 0);   // units per sub-batch of the tiered unit codec (mic_api.hip)
// MIC2, one temporal volume per call (mic_mic2_batch.hip): its frames through the sub-batch cores below, cut by mic2_batch_cuts;
// decompress: frames 0 .. n-1 of the file's n_total
int mic2_temporal_compress(const uint16_t *frames, int width, int height, int nframes, uint16_t max_value,
                           uint8_t *out, size_t out_cap, size_t *out_len);
int mic2_temporal_decompress(const uint8_t *c, size_t len, int w, int h, int n_total, int n, uint16_t *frames_out);
// What the patch and crop readers share beside the gather (mic_gather.hip; patch_pointer and the kernels' launcher: mic_pieces.h).
// A sub-batch's nb streams, len(i) bytes at src(i) -- host memory, or (device) the session's device --, back to back into s->io_comp
// (reserved here, with the 64 bytes the decode kernels may read past a stream's end): neighbours in the source go in one copy.
// begins[i] .. ends[i]: stream i in the buffer.
int pack_streams(mic_hip_session *s, int nb, const std::function<uint64_t(int)> &len, const std::function<const uint8_t *(int)> &src, bool device,
                 std::vector<uint64_t> &begins, std::vector<uint64_t> &ends);
// What a crop door does once it has a plan: the session -- *s, made current, or when NULL one leased here --, then d_out judged for a
// tensor of `need` bytes in o's type (patch_pointer; an allocation that ends before the tensor does and an address that is not
// aligned to the sample -- u16 for the native format, no demand on the u8 RGB one -- are MIC_ERR_ARGS: out_cap held the tensor).
struct OutFormat;                 // (mic_pieces.h)
int crop_door(mic_hip_session **s, DefaultLease &lease, void **d_out, size_t need, const OutFormat &o);
// MIC2 crops (mic_mic2_crops.hip).  A piece is one (crop, frame) overlap: w x h samples from (sx, sy) of frame `frame` to (dx, dy) of
// slice dz of crop `crop`, k = the frame's place in the plan's frame list.  The temporal kernel takes one record per crop instead,
// its footprint: frame = max(z, 0), the crop's first frame inside the volume, dz = that frame's slice, k = its last frame inside it.
struct CropPiece { int32_t crop, frame, sx, sy, dx, dy, dz, w, h, k; };
struct CropPlan {
    std::vector<uint32_t> frames;           // frames whose streams are entropy-decoded, ascending, each once
    std::vector<CropPiece> pieces;          // sorted by frame (stable: crop order inside a frame)
    std::vector<CropPiece> prints;          // one per crop with a non-empty overlap, in crop order
};
int mic2_plan_crops(int width, int height, int nframes, int temporal, const int32_t *xyz, int n, int cw, int ch, int cd, CropPlan &plan);
// where a one-volume crop door finds the stream of a frame: blob(frame) -> its first byte, on the host or (device = true) on the session's device
struct Mic2Source { bool device = false; std::function<const uint8_t *(uint32_t frame)> blob; };
struct Mic2Head { int w = 0, h = 0, n = 0, temporal = 0; const uint8_t *table = nullptr; uint64_t file_len = 0; };   // table: the 8 n bytes behind the fixed header (host)
int mic2_crop_args(const Mic2Head &m, const int32_t *xyz, int n, int cw, int ch, int cd, size_t sample_bytes, size_t out_cap, size_t *need);
size_t workspace_budget();        // per-call workspace ceiling (mic_api.hip)
// Units [i0, return) of the next sub-batch of a list of units of px[i] pixels each, for the readers that decode units of mixed sizes
// into one slab (strip-file crops, MIC2 crops of many volumes; mic_strip_crops.hip): next_sub_batch (mic_staged.h) under their capacity
size_t next_strip_cut(const std::vector<size_t> &px, size_t i0);
size_t next_strip_cut(const std::vector<size_t> &px, size_t i0, size_t budget);   // ... under a ceiling of `budget` bytes instead of the default
// MIC2 whole-volume batches (mic_mic2_batch.hip; the host doors: mic_host_io.hip).  The units of a call's volumes -- volume order, then
// frame order -- go through the unit codec in sub-batches cut by their sizes alone: next_strip_cut's rule under `budget` bytes.
// -> [0, ..., px.size()]
std::vector<size_t> mic2_batch_cuts(const std::vector<size_t> &px, size_t budget);
// One unit of an encode sub-batch: the frame at `cur` on the session's device.  residual: coded as TemporalDeltaEncode against the
// frame that lies directly in front of it (cur - w * h: the volume's own predecessor, or the lead frame a host part uploads).
struct Mic2EncUnit { const uint16_t *cur; int32_t w, h; uint16_t max_value, residual; };
// The MIC2 unit chains, written once: the single calls, the batches and the crop readers (mic_mic2_crops.hip) all run through them.
// nb units through ONE encode chain (k_mic2_residual in front); on return the streams of the units that coded lie
// packed at *d_blobs + offs[i] .. offs[i + 1] (s->packed, until the session's next chain), st[i] = the unit's code.
int mic2_batch_encode_units(mic_hip_session *s, const Mic2EncUnit *u, int nb, const uint8_t **d_blobs, uint64_t *offs, int32_t *st);
// One unit of a decode sub-batch: its stream on the session's device (64 readable bytes behind it); a frame unit decodes to `out`, a
// residual unit (out unused) into its symbol slab.
struct Mic2DecUnit { const uint8_t *comp; uint32_t len; int32_t w, h; uint16_t *out; uint32_t residual; };
// What a sub-batch holds of one temporal volume: its units u0 .. u0 + nb - 1 are the volume's frames f0 .. f0 + nb - 1, which go to
// dst, dst + npx, ...; carry = frame f0 - 1 (unused when f0 == 0: unit u0 decoded frame 0 into dst); fbad = the volume's first failed
// frame so far (INT_MAX: none) -- the sum stops in front of it.
struct Mic2DecSpan { const uint16_t *carry; uint16_t *dst; uint32_t npx; int32_t u0, nb, f0, fbad, pad; };
// nb units through ONE decode chain -- frame units and symbol units (tANS, RLE expansion, k_mic2_check_units: a residual expands to
// exactly its own frame) --, complete on return with st[i] = the unit's code; then, for the temporal spans of that chain (built from
// st), the running sums -- one launch, complete on return.
int mic2_batch_decode_units(mic_hip_session *s, const Mic2DecUnit *u, int nb, int32_t *st);
int mic2_batch_accumulate(mic_hip_session *s, const Mic2DecSpan *spans, int nspans);
// a MIC2 file's 20-byte header and frame table (multiframe.go:49-91) from its frames' stream lengths
void mic2_write_head(uint8_t *out, int w, int h, int n, bool temporal, const uint32_t *lens);
// what the decode doors ask of a file's head before a frame is looked at (mic_hip_mic2_decompress's checks): MIC_OK, or the volume's code
int mic2_batch_parse(const uint8_t *head, size_t head_len, uint64_t file_len, Mic2Head &m);
// RGB batches (mic_rgb_batch.hip): many images of different sizes per call, CompressRGB / DecompressRGB (rgbcompress.go:25-33) of each.
// One image of a sub-batch on the encode side: its RGB at d_rgb + rgb_off; container 1 = a MICR header in front of its blob.
// status on entry: not MIC_OK = skip the image.  On return: status / failed_plane (0 Y, 1 Co, 2 Cg, -1 not a plane's), and the
// blob at [blob_off, blob_off + blob_len) of the payload buffer (a failed image has none).
struct RgbImage { uint64_t rgb_off; int32_t w, h, container; int32_t status = MIC_OK, failed_plane = -1; uint64_t blob_off = 0, blob_len = 0; };
// a plane of a blob as decompressWSIPlane sees it (wsicompress.go:487-524): mode 0 zero, 1 `value`, 2 a stream, 3 raw; off / len:
// the bytes of modes 2 / 3, off from the blob's first byte
struct RgbPlaneRec { uint8_t mode; uint16_t value; uint64_t off, len; };
// One blob of a sub-batch on the decode side: [blob_off, blob_off + blob_len) of d_blobs, pixels to d_rgb_out + rgb_off
struct RgbBlob { uint64_t blob_off, blob_len, rgb_off; int32_t w, h; int32_t status = MIC_OK, failed_plane = -1; RgbPlaneRec pl[3]; };
// what the host needs of a blob to check it: the three plane lengths and the first three bytes of each plane (zero where the blob ends before)
struct RgbHead { uint32_t len[3]; uint8_t b[3][3]; uint8_t pad[3]; };
void rgb_head_of(const uint8_t *blob, uint64_t bl, RgbHead &h);
// ... of n blobs of a device buffer, blob i at d_begins[i] .. d_ends[i] of d_blobs (device arrays), behind what `stream` holds (k_rgb_batch_heads)
int rgb_heads_enqueue(hipStream_t stream, const uint8_t *d_blobs, const uint64_t *d_begins, const uint64_t *d_ends, int n, RgbHead *d_heads);
// u16 samples from a plane of an image of npx pixels to the next in a slab of YCoCg-R planes
__host__ __device__ inline size_t rgb_stride(size_t npx) { return (npx + 7) & ~(size_t)7; }       // planes start 16-byte aligned
// decompressRGBTileBlob's checks (wsicompress.go:431-461) + decompressWSIPlane's for every plane: the blob's status, the plane it names
int rgb_parse_head(const RgbHead &h, uint64_t bl, size_t npx, RgbPlaneRec pl[3], int32_t *failed_plane);
// images [i0, return) of the next sub-batch of images [.., n), npx(i) pixels each: their three units a launch's grid y and under the
// workspace ceiling, about target_px pixels
int rgb_next_cut(const std::function<size_t(int)> &npx, int i0, int n, size_t target_px);
// the core, on device buffers: the plane kernel, ONE unit batch over every non-constant plane, the blobs assembled in `payload` from
// byte pay0 on (a caller that passes pay0 > 0 has reserved the buffer; *pay_end: where they end).  Complete on return.
int rgb_encode_run(mic_hip_session *s, const uint8_t *d_rgb, RgbImage *img, int n, DevBuf &payload, uint64_t pay0, uint64_t *pay_end);
// the blobs (checked: pl[] filled in, status MIC_OK) -> pixels: fills, ONE unit batch over every mode-2 plane, the inverse transform
int rgb_decode_run(mic_hip_session *s, const uint8_t *d_blobs, RgbBlob *blobs, int n, uint8_t *d_rgb_out);
// WaveletV2 batches of frames of any shapes and level counts (mic_wavelet.hip; the host doors: mic_host_io.hip).
// the argument gate of every entry point: MIC_OK, or why rows x cols (a decode: at `level` of a header's `levels`) is not coded here
int wv_check_shape(int rows, int cols, int levels = 0, int level = 0);
// the level count the header carries: `levels` clamped to 1 .. 8, stopped where a side falls below 2 (waveletfsecompressu16.go:321-330)
int wv_levels_applied(int rows, int cols, int levels);
void wv_put_header(uint8_t *out, int rows, int cols, uint16_t max_value, int applied);     // the 11 bytes of :346-350
// frames [i0, return) of the next sub-batch of frames [.., n) of px(i) pixels: budget / (unit_ws_bytes(2 mp + 16) + 8 mp) frames of the
// largest so far (every unit is laid out by it), at most 65535 (the chain's grids) and 2^30 pixels (the position groups of a launch
// stay below 2^31 whatever the shapes)
size_t wv_next_cut(const std::function<size_t(size_t)> &px, size_t i0, size_t n, size_t budget);
// One frame of an encode sub-batch: rows x cols at d_px + px_off, `applied` levels.  The core: ONE launch chain over the n frames; on
// return the streams (no 11-byte header) of the frames that coded lie packed at *d_blobs + offs[i] .. offs[i + 1] (s->packed).
struct WvEncFrame { uint64_t px_off; int32_t rows, cols, applied; };
int wv_encode_run(mic_hip_session *s, const uint16_t *d_px, const WvEncFrame *f, int n, const uint8_t **d_blobs, uint64_t *offs, int32_t *st);
// One frame of a decode sub-batch: the stream d_comp + begin .. end of a rows x cols frame of `levels`, wanted at `level`; its
// nr[level] x nc[level] pixels go to d_out + px_off.  The core: one launch chain, and one more over the frames that the prefix rule of a
// reduced decode sends round again (*redone += their count).  syms (nullable): tANS symbols decoded per frame.
struct WvDecFrame { uint64_t begin, end, px_off; int32_t rows, cols, levels, level; };
int wv_decode_run(mic_hip_session *s, const uint8_t *d_comp, uint16_t *d_out, const WvDecFrame *f, int n, int32_t *st, uint64_t *syms, uint64_t *redone);
// Strip files (PICS: parallelstrips.go, PICA: parallelstripsadaptive.go): a header, a table and one unit per strip.  Strip k of a
// file of height h and n strips as its header states it -- rows [y0, y1), bytes [start, start + len) of the file, the unit's flags --
// read from the header and the table alone; what the whole-image decoders (mic_host_io.hip) and the crop calls (mic_strip_crops.hip) decode by.
struct StripEntry { long y0, y1; size_t start, len; uint16_t flags; };
inline StripEntry pics_strip_entry(const uint8_t *c, int h, int n, int k) {       // strip_height rows from k * strip_height (:288-304)
    const long sh = (long)get_u32(c + 16), y0 = k * sh;
    return StripEntry{ y0, std::min<long>(h, y0 + sh), 20 + (size_t)n * 8 + get_u32(c + 20 + (size_t)k * 8), get_u32(c + 24 + (size_t)k * 8), 0 };
}
inline StripEntry pica_strip_entry(const uint8_t *c, int h, int n, int k) {       // from its y0 to the next strip's (:186-202)
    const uint8_t *e = c + 16 + (size_t)k * 16;
    return StripEntry{ (long)get_u32(e), (k + 1 < n) ? (long)get_u32(e + 16) : h, 16 + (size_t)n * 16 + get_u32(e + 4), get_u32(e + 8),
                       (uint16_t)(2 | ((get_u32(e + 12) & 1u) ? MIC_HIP_PRED_GRAD : 0)) };   // picaFlagGradPredictor
}
// what a decoder asks of an entry of a w x h file of file_len bytes before it decodes the strip: MIC_OK, or the file's code
inline int strip_entry_check(const StripEntry &e, int w, int h, size_t file_len) {
    const size_t end = e.start + e.len;
    if (end > file_len || e.start > end) return MIC_ERR_CORRUPT;                 // parallelstrips.go:300-304, parallelstripsadaptive.go:186-190
    if (e.y0 < 0 || e.y1 <= e.y0 || e.y1 > h) return MIC_ERR_CORRUPT;            // Go: make / slice panics
    if (e.len == 0) return MIC_ERR_CORRUPT;
    if ((size_t)w * (size_t)(e.y1 - e.y0) > ((size_t)1 << 28)) return MIC_ERR_UNSUPPORTED;
    return MIC_OK;
}
// adaptiveStripBoundaries as the reference states it, on the host (mic_pica.hip); cost[y] = rowCost[y], cost[0] ignored
std::vector<int> pica_boundaries(const std::vector<unsigned long long> &cost, int height, int num_strips);
// one blocking host <-> device copy through the transfer engine of mic_host_io.hip (pinned host memory: DMA in place; ordinary
// memory: staged through pinned slots by the worker threads).  The device side must be ready / is complete on return.
int host_copy(int device, void *dev, void *host, size_t bytes, bool to_device);
// the cut of n weighted items into `shards` contiguous shards (mic_hip_shard_plan; first has shards + 1 entries)
void plan_shards(const uint64_t *w, int n, int shards, int *first);
// work(0 .. n - 1) side by side, each on a thread of its own (work(0) on the calling thread); returns the code of the first
// (lowest) k that failed.  An exception inside work(k) is that k's MIC_ERR_NOMEM / MIC_ERR_INTERNAL.
int run_parallel(int n, const std::function<int(int)> &work);
// THE fan-out of a host entry point over the devices of mic_hip_set_devices ("several devices"): shard k -- items
// [first[k], first[k + 1]) -- runs work(s, i0, i1) on a thread of its own (run_parallel) with a session `s` leased from devs[k]; empty
// shards are skipped, the lowest failing shard's code comes back.  ONE shard over all the items, on the default device or the session
// the thread already holds, when `first` has two entries, the call is nested, or there are fewer devices than shards.
// MIC_HIP_TRACE=1: a line per shard on stderr.  (MIC_LOCAL: for the library's own sources, not among its dynamic symbols.)
#define MIC_LOCAL __attribute__((visibility("hidden")))
using ShardWork = std::function<int(mic_hip_session *s, int i0, int i1)>;
MIC_LOCAL int over_devices(const std::vector<int> &first, const ShardWork &work);
// the same over items [0, n) cut by plan_shards: min(devices, n) shards, item i weighing weight(i)
MIC_LOCAL int over_devices(int n, const std::function<uint64_t(int)> &weight, const ShardWork &work);
#define kWorkspaceBudget (micapi::workspace_budget())
}  // namespace micapi
