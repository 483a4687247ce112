// mic_api.hip -- host side of libmic_hip.so: the C ABI of include/mic_hip.h, the HIP batch
// launcher that replaces the reference's goroutine / pthread fan-out
// (parallelstrips.go:77-93, mic_parallel.c:146-181, wsicompress.go:126-145) and the
// PICS / MIC2 container assembly (parallelstrips.go:101-123, multiframe.go:49-91).
//
// There is no CPU codec in this file: every pixel and every compressed byte is produced by
// the kernels in mic_encode.hip / mic_decode.hip.  The host only moves buffers, fills unit
// descriptors and writes container headers.
#include "mic_session.h"

namespace micapi {

// The entry points that take host pointers run on a small POOL of default sessions (ojph/mic_parallel.h:47-48 promises re-entrancy;
// one session behind one mutex would serialise every goroutine of a Go host): a call leases a free session for its duration,
// creates one while the pool is below its size (MIC_HIP_POOL, default 3), waits otherwise.  g_mu guards the device choice and
// the pool's lists; a leased session is used without any lock.
// Several devices (mic_hip_set_devices): a pool per device; the batch entry points cut their jobs into one contiguous shard per
// listed device and run the shards side by side, each on a session of its device's pool (mic_host_io.hip).  g_device is the first
// of the list: what every other host-pointer entry point runs on.
std::mutex g_mu;
std::condition_variable g_pool_cv;
int g_device = 0;
std::vector<int> g_devices(1, 0);
bool g_device_ok = false;
std::string g_device_name;
struct DevPool { std::vector<mic_hip_session *> free_; int made = 0; };
std::map<int, DevPool> g_pools;                        // by device
thread_local mic_hip_session *tl_default = nullptr;   // the session the calling thread holds (leases nest: containers call the unit codec)
thread_local int tl_depth = 0;

static int pool_max() {
    static const int v = [] { const char *e = getenv("MIC_HIP_POOL"); const int n = e ? atoi(e) : 3; return std::min(std::max(n, 1), 16); }();
    return v;
}

// gfx950 or nothing: the code objects are built for that target only.  One answer per device, remembered.
int check_device(int device) {
    static std::mutex mu; static std::vector<int8_t> known;              // 0 unknown, 1 ok, -1 not usable
    std::lock_guard<std::mutex> lk(mu);
    int n = 0;
    if (device < 0 || hipGetDeviceCount(&n) != hipSuccess || device >= n) return MIC_ERR_DEVICE;
    if (known.size() < (size_t)n) known.resize((size_t)n, 0);
    if (known[(size_t)device] == 0) {
        hipDeviceProp_t p;
        known[(size_t)device] = (hipGetDeviceProperties(&p, device) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ? 1 : -1;
    }
    return known[(size_t)device] == 1 ? MIC_OK : MIC_ERR_DEVICE;
}

static int ensure_device_locked() {                                     // g_mu held
    if (g_device_ok) { return hipSetDevice(g_device) == hipSuccess ? MIC_OK : MIC_ERR_DEVICE; }
    int rc = check_device(g_device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(g_device));
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, g_device));
    char buf[256];
    snprintf(buf, sizeof buf, "%s %d CUs %.0f GiB (%s)", p.gcnArchName, p.multiProcessorCount,
             (double)p.totalGlobalMem / (1024.0 * 1024.0 * 1024.0), p.name);
    g_device_name = buf;
    g_device_ok = true;
    return MIC_OK;
}
int ensure_device() { std::lock_guard<std::mutex> lk(g_mu); return ensure_device_locked(); }

mic_hip_session *cur_default() { return tl_default; }

int DefaultLease::acquire(int device) {
    if (tl_default) {                                                   // nested call on this thread: the session it already holds
        s = tl_default; tl_depth++; held = true;
        return s->activate();
    }
    {
        std::unique_lock<std::mutex> lk(g_mu);
        int rc = ensure_device_locked();
        if (rc) return rc;
        if (device < 0) device = g_device;
        else if (std::find(g_devices.begin(), g_devices.end(), device) == g_devices.end()) return MIC_ERR_ARGS;
        DevPool &pool = g_pools[device];
        while (pool.free_.empty() && pool.made >= pool_max()) g_pool_cv.wait(lk);
        if (!pool.free_.empty()) { s = pool.free_.back(); pool.free_.pop_back(); }
        else { s = new mic_hip_session(); s->device = device; pool.made++; }
    }
    tl_default = s; tl_depth = 1; held = true;
    int rc = s->activate();
    if (rc) return rc;
    if (!s->stream) HIP_TRY(mic_stream_create(&s->stream));
    return MIC_OK;
}
DefaultLease::~DefaultLease() {
    if (!held) return;
    if (--tl_depth > 0) return;
    tl_default = nullptr;
    std::lock_guard<std::mutex> lk(g_mu);
    g_pools[s->device].free_.push_back(s);
    g_pool_cv.notify_all();
}
std::vector<int> default_devices() { std::lock_guard<std::mutex> lk(g_mu); return g_devices; }

// Per-call workspace ceiling (the container entry points cut their unit lists into sub-batches that stay under it): what the session
// already holds, or -- never more than a quarter of the device -- half of what is free right now, so that several sessions on one GPU
// (the pool, explicit sessions, the caller's own tensors) do not each grow towards the same ceiling.  MIC_HIP_WS_BUDGET_MB overrides it
// (tests walk the sub-batch loops with small inputs).
// Sessions of this thread's device that are out on lease right now (this thread's included; at least 1): each of them reads the same
// free-memory figure at about the same time, so each may plan with its share of it only.
static size_t leased_here() {
    std::lock_guard<std::mutex> lk(g_mu);
    const int dev = tl_default ? tl_default->device : g_device;
    auto it = g_pools.find(dev);
    if (it == g_pools.end()) return 1;
    return (size_t)std::max(1, it->second.made - (int)it->second.free_.size());
}
size_t workspace_budget() {
    static const long env_mb = [] { const char *e = getenv("MIC_HIP_WS_BUDGET_MB"); return e ? atol(e) : 0L; }();
    if (env_mb > 0) return (size_t)env_mb << 20;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) { tot = (size_t)96 << 30; fr = tot / 2; }
    const size_t held = tl_default ? tl_default->reserved_bytes() : 0;
    return std::max<size_t>(std::max<size_t>(held, std::min<size_t>(tot / 4, fr / 2 / leased_here())), (size_t)1 << 30);
}

// ---- encode -------------------------------------------------------------------------------
// A launch chain in the given tier.  Tier 1 (the small slabs) is where a batch starts unless the session has needed tier 2 before or
// a unit's depth says so (14 bits and more: an alphabet past the 8192-bin tables); session_*_finish runs the batch again in tier 2
// when a unit reports MICD_INT_GROW.
static int encode_enqueue_tier(mic_hip_session *s, const uint16_t *d_pixels, const mic_hip_unit *units, int n, int tier, bool pairs) {
    size_t max_px = 0;
    for (int i = 0; i < n; i++) max_px = std::max(max_px, (size_t)units[i].width * (size_t)units[i].height);
    int rc = s->lay_out(n, max_px, tier);
    if (rc) return rc;
    // The packed buffer is sized from what the session's last batch needed; it is reserved here, in front of the chain (a reallocation
    // behind it would wait for the queued chain to drain).
    {
        size_t raw = 0;
        for (int i = 0; i < n; i++) raw += (size_t)units[i].width * (size_t)units[i].height * 2;
        const size_t want = std::max(s->pack_hint + s->pack_hint / 8, raw / 3) + ((size_t)64 << 10);
        if ((rc = s->packed.reserve(want))) return rc;
        if ((rc = s->pin_off.reserve((size_t)n + 1))) return rc;
    }
    bool any_grad = false, narrow = true, any_gap = false;
    for (int i = 0; i < n; i++) any_gap |= (units[i].nstates & MIC_HIP_GAP_REMOVAL) != 0;
    if (any_gap && (rc = s->gap.reserve((size_t)mic_gap_stride((uint32_t)s->tab_syms) * (size_t)n))) return rc;
    for (int i = 0; i < n; i++) {
        MicUnit &u = s->h_units[(size_t)i];
        narrow &= (units[i].nstates & 0xFF) <= 2;
        u.px_in = d_pixels + units[i].px_offset;
        u.w = units[i].width; u.h = units[i].height;
        u.max_value = units[i].max_value; u.nstates = units[i].nstates & 0xFF;
        u.pred = (units[i].nstates & MIC_HIP_PRED_GRAD) ? 1u : 0u; any_grad |= u.pred != 0;
        if (units[i].nstates & MIC_HIP_GAP_REMOVAL) { u.gap = 1; u.gap_buf = (uint8_t *)s->gap.p + (size_t)mic_gap_stride((uint32_t)s->tab_syms) * (size_t)i; }
        u.tok_cap = (uint32_t)tok_cap_tier((size_t)u.w * (size_t)u.h, tier);
    }
    // The encoder's classes: what the session's last batches used, plus what the HOST can tell -- the two big instances always (a
    // two-state unit whose attempt fails is handed to the wide one; a miss there is the serial encoder, 0.8 s for an XR batch:
    // tools/mask_miss.py), the one-wave instances when a unit is small enough for them, the tableLog 14-16 ones when a unit is deep
    // enough to have such an alphabet.  What is left to memory alone costs ~5 us a launch when it is wrong the other way.
    uint32_t enc_hint = MIC_ENC_CLS_NARROW2 | MIC_ENC_CLS_WIDE;
    for (int i = 0; i < n; i++) {
        if ((size_t)units[i].width * (size_t)units[i].height <= 131072u) enc_hint |= MIC_ENC_CLS_SMALL12 | MIC_ENC_CLS_SMALL13;
        if (units[i].max_value >= 2048u) enc_hint |= MIC_ENC_CLS_TL14 | MIC_ENC_CLS_TL15 | MIC_ENC_CLS_TL16;
        if (units[i].max_value < 4096u) enc_hint |= MIC_ENC_TBL_C4K;                 // (tokens of a frame of up to 12 bits stay below 4096: the compact table instance)
    }
    const int variant = s->variant | MIC_VARIANT_FRAMES | (any_grad ? MIC_VARIANT_GRAD : 0) | (narrow ? MIC_VARIANT_NARROW : 0) | (any_gap ? MIC_VARIANT_GAP : 0);
    if ((rc = s->run_encode([&] {
            mic_launch_encode((MicUnit *)s->units.p, n, s->stream, variant, &s->timer, s->enc_classes.mask() | enc_hint);
#ifndef MIC_PICA_NO_PICK   // (A / B builds, tools/bench_pica_batch.py: both candidates are packed and the host picks)
            if (pairs) mic_launch_pica_pick((MicUnit *)s->units.p, n / 2, s->stream, &s->timer);   // (the sizes are final: pick before the scan and the pack)
#endif
        }))) return rc;
    s->learn_encode = true;
    // Compaction and the read-back of the results ride behind the chain, so that session_encode_finish is ONE synchronisation (round 3:
    // descriptors down, a synchronisation, sizes summed on the host, scan + pack launched, a second synchronisation -- 86 us of idle
    // device between the chain and the pack of every call).  The pack kernels leave a batch that does not fit the packed buffer alone
    // and finish packs it again into a buffer of the right size.
    {
        mic_launch_pack((const MicUnit *)s->units.p, n, (uint64_t *)s->offsets.p, (uint8_t *)s->packed.p, (uint64_t)s->packed.cap, s->stream, &s->timer);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(s->h_units.data(), s->units.p, sizeof(MicUnit) * (size_t)n, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(s->pin_off.p, s->offsets.p, 8 * ((size_t)n + 1), hipMemcpyDeviceToHost, s->stream));
        s->readback_queued = true; s->pack_queued = true; s->pack_cap = s->packed.cap;
    }
    return MIC_OK;
}

int session_encode_enqueue(mic_hip_session *s, const uint16_t *d_pixels, const mic_hip_unit *units, int n, bool pica_pairs) {
    if (n <= 0 || (pica_pairs && (n & 1))) return MIC_ERR_ARGS;
    if (n > 65535) return MIC_ERR_UNSUPPORTED;                           // units are a launch's grid y in several kernels: callers sub-batch
    size_t max_px = 0;
    bool deep = false;
    for (int i = 0; i < n; i++) {
        if (units[i].width <= 0 || units[i].height <= 0) return MIC_ERR_ARGS;
        max_px = std::max(max_px, (size_t)units[i].width * (size_t)units[i].height);
        const int ns = units[i].nstates & 0xFF;
        if (!(ns == 2 || ns == 4 || ns == 8) || (units[i].nstates & ~(0xFF | MIC_HIP_PRED_GRAD | MIC_HIP_GAP_REMOVAL))) return MIC_ERR_ARGS;
        if ((units[i].nstates & MIC_HIP_PRED_GRAD) && (units[i].nstates & MIC_HIP_GAP_REMOVAL)) return MIC_ERR_ARGS;   // (no such codec in the reference)
        deep |= units[i].max_value >= (1u << 13);                        // depth 14+: tokens reach past 8192
    }
    if (max_px > ((size_t)1 << 28)) return MIC_ERR_UNSUPPORTED;
    const int tier = (s->force_big || deep) ? 2 : 1;
    s->retry.kind = 0;
    if (tier == 1) { s->retry.kind = 1; s->retry.pairs = pica_pairs; s->retry.d_in = d_pixels; s->retry.units.assign(units, units + n); }
    return encode_enqueue_tier(s, d_pixels, units, n, tier, pica_pairs);
}

// reads the units back; a tier-1 chain that reported MICD_INT_GROW somewhere is run again in tier 2 first
static int finish_units(mic_hip_session *s, int n) {
    for (int pass = 0; pass < 2; pass++) {
        if (!s->readback_queued) HIP_TRY(hipMemcpyAsync(s->h_units.data(), s->units.p, sizeof(MicUnit) * (size_t)n, hipMemcpyDeviceToHost, s->stream));
        s->readback_queued = false;
        HIP_TRY(hipStreamSynchronize(s->stream));
        bool grow = false;
        for (int i = 0; i < n; i++) grow |= s->h_units[(size_t)i].status == MICD_INT_GROW;
        if (!grow) return MIC_OK;
        if (pass == 1 || s->retry.kind == 0) break;                      // (tier 2 never reports it; a caller that laid the units out itself has no retry)
        s->force_big = true;
        const mic_hip_session::Retry r = s->retry;                       // (the enqueue below rewrites it)
        int rc;
        if (r.kind == 1) rc = encode_enqueue_tier(s, (const uint16_t *)r.d_in, r.units.data(), n, 2, r.pairs);
        else rc = session_decode_enqueue_spans(s, (const uint8_t *)r.d_in, r.begins.data(), r.ends.data(), r.units.data(), n, (uint16_t *)r.d_out);
        if (rc) return rc;
    }
    for (int i = 0; i < n; i++) if (s->h_units[(size_t)i].status == MICD_INT_GROW) s->h_units[(size_t)i].status = MICD_ERR_INTERNAL;
    return MIC_OK;
}

// The tier is sticky, not permanent: a session that one escape-heavy (or 16-bit) batch sent to the worst-case slabs -- 42 bytes a pixel
// -- goes back to the ordinary ones when kTierCalm batches in a row would have fitted them (every unit's tokens, segments, alphabet
// and table inside the tier-1 capacities), and ensure() then returns the large slabs' memory.  Called with the descriptors read back.
static void tier_review(mic_hip_session *s, int n) {
    if (!s->force_big || s->tier != 2) return;
    bool fits = true;
    const size_t ts1 = tab_syms_tier(1);
    for (int i = 0; i < n && fits; i++) {
        const MicUnit &u = s->h_units[(size_t)i];
        if (u.mode != 0) { fits = false; break; }                       // (symbol units: laid out in tier 2 by their paths, mic_hip_session::lay_out)
        const size_t px = (size_t)std::max(u.w, 0) * (size_t)std::max(u.h, 0);
        const size_t ntok = std::max<size_t>(u.ntok, u.count);
        fits = u.status == MICD_OK && ntok + 64 <= tok_cap_tier(px, 1) && (size_t)u.nseg + 8 <= seg_cap_tier(px, 1) &&
               u.symbol_len <= ts1 && u.table_log <= 13 && u.max_value < (1u << 13);
    }
    if (!fits) { s->calm_batches = 0; return; }
    if (++s->calm_batches >= mic_hip_session::kTierCalm) { s->force_big = false; s->calm_batches = 0; s->shrink_pending = true; }
}

// what the batch just finished tells the next one (mic_launch.h: launch masks)
static void learn_classes(mic_hip_session *s, int n) {
    tier_review(s, n);
    if (s->learn_decode) {
        uint32_t seen = 0;
        for (int i = 0; i < n; i++) {
            const MicUnit &u = s->h_units[(size_t)i];
            const int c = mic_dec_cls(u.flavour, u.table_log, u.zero_bits);
            if (c >= 0 && u.comp_len - u.bits_off < (1u << 27)) {
                seen |= 1u << c;
                if (c == 0 && mic_split_gate(u, s->split_cfg)) seen |= MIC_CLS_SPLIT | MIC_CLS_RETRY;   // (the retry launch stands behind every split launch)
            }
        }
        s->dec_classes.learn(seen);
    }
    if (s->learn_encode) {
        uint32_t seen = 0;
        for (int i = 0; i < n; i++) {
            const MicUnit &u = s->h_units[(size_t)i];
            const uint32_t tl = u.table_log;
            if (tl < MIC_MIN_TABLELOG || tl > MIC_MAX_TABLELOG) continue;                 // (the chain stopped in front of the tANS stage)
            if (tl <= 13 && u.symbol_len <= 4096u && u.nstates != 108) seen |= MIC_ENC_TBL_C4K;   // tb_is_c4k, mic_tables.hip: by the rule, whichever instance ran
            if (tl == 14) seen |= MIC_ENC_CLS_TL14;
            else if (tl == 15) seen |= MIC_ENC_CLS_TL15;
            else if (tl == 16) seen |= MIC_ENC_CLS_TL16;
            else if (u.ntok <= 98304u && u.symbol_len <= 1024u) seen |= (tl <= 12 && u.symbol_len <= 512u) ? MIC_ENC_CLS_SMALL12 : MIC_ENC_CLS_SMALL13;   // te_small_class, mic_encode.hip
            else if (u.nstates == 2 && u.symbol_len <= 4096u) seen |= MIC_ENC_CLS_NARROW2 | (u.nstates_used != 2 ? MIC_ENC_CLS_WIDE : 0u);
            else seen |= MIC_ENC_CLS_WIDE;
        }
        s->enc_classes.learn(seen);
    }
    s->learn_decode = s->learn_encode = false;
}

int session_encode_finish(mic_hip_session *s, const uint8_t **d_blobs, uint64_t *h_offsets, int32_t *h_status, int32_t *h_nstates) {
    int n = s->n_last;
    if (n <= 0) return MIC_ERR_ARGS;
    { const int frc = finish_units(s, n); if (frc) return frc; }
    learn_classes(s, n);
    uint64_t total = 0;
    for (int i = 0; i < n; i++) {
        const MicUnit &u = s->h_units[(size_t)i];
        h_offsets[i] = total;
        if (u.status == MICD_OK && !u.skip_pack) total += u.blob_len;        // (as k_scan_lens counts: a PICA strip's loser takes no room)
        h_status[i] = u.status;
        if (h_nstates) h_nstates[i] = u.nstates_used;
    }
    h_offsets[n] = total;
    const bool packed_already = s->pack_queued && (size_t)total + 16 <= s->pack_cap && s->pin_off.cap > (size_t)n && s->pin_off.p[n] == total;
    s->pack_queued = false;
    s->pack_hint = (size_t)total;
    if (!packed_already) {                         // a caller that launched its own chain, or a batch larger than the session's last
        int rc = s->packed.reserve((size_t)total + (size_t)total / 8 + ((size_t)64 << 10));   // (what the next enqueue of such a batch will ask for: no second reallocation)
        if (rc) return rc;
        mic_launch_pack((const MicUnit *)s->units.p, n, (uint64_t *)s->offsets.p, (uint8_t *)s->packed.p, (uint64_t)s->packed.cap, s->stream, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    if (d_blobs) *d_blobs = (const uint8_t *)s->packed.p;
    return MIC_OK;
}

// ---- decode -------------------------------------------------------------------------------
int session_decode_enqueue(mic_hip_session *s, const uint8_t *d_blobs, const uint64_t *h_offsets,
                           const mic_hip_unit *units, int n, uint16_t *d_pixels_out) {
    if (n <= 0) return MIC_ERR_ARGS;
    return session_decode_enqueue_spans(s, d_blobs, h_offsets, h_offsets + 1, units, n, d_pixels_out);
}

int session_decode_enqueue_spans(mic_hip_session *s, const uint8_t *d_blobs, const uint64_t *begins, const uint64_t *ends,
                                 const mic_hip_unit *units, int n, uint16_t *d_pixels_out) {
    if (n <= 0) return MIC_ERR_ARGS;
    if (n > 65535) return MIC_ERR_UNSUPPORTED;
    size_t max_px = 0;
    bool any_gap = false;
    for (int i = 0; i < n; i++) {
        if (units[i].width <= 0 || units[i].height <= 0) return MIC_ERR_ARGS;
        max_px = std::max(max_px, (size_t)units[i].width * (size_t)units[i].height);
        if ((units[i].nstates & MIC_HIP_PRED_GRAD) && (units[i].nstates & MIC_HIP_GAP_REMOVAL)) return MIC_ERR_ARGS;
        any_gap |= (units[i].nstates & MIC_HIP_GAP_REMOVAL) != 0;
    }
    if (max_px > ((size_t)1 << 28)) return MIC_ERR_UNSUPPORTED;
    for (int i = 0; i < n; i++) if (ends[i] < begins[i] || ends[i] - begins[i] > 0xFFFFFFF0ull) return MIC_ERR_ARGS;
    const int tier = s->force_big ? 2 : 1;                               // (a stream's alphabet is not known before its header is parsed)
    if (tier == 1) {                                                     // what a second run in tier 2 needs (the arrays may be the caller's temporaries)
        mic_hip_session::Retry r;
        r.kind = 2; r.d_in = d_blobs; r.d_out = d_pixels_out; r.units.assign(units, units + n);
        r.begins.assign(begins, begins + n); r.ends.assign(ends, ends + n);
        s->retry = std::move(r);
        begins = s->retry.begins.data(); ends = s->retry.ends.data(); units = s->retry.units.data();
    } else if (s->retry.kind != 0 && begins != s->retry.begins.data()) s->retry.kind = 0;
    int rc = s->lay_out(n, max_px, tier);
    if (rc) return rc;
    if (any_gap && (rc = s->gap.reserve((size_t)mic_gap_stride((uint32_t)s->tab_syms) * (size_t)n))) return rc;
    bool any_grad = false;
    uint32_t rows_kmask = 0;                                             // predictor classes (by width) this batch holds
    for (int i = 0; i < n; i++) {
        MicUnit &u = s->h_units[(size_t)i];
        rows_kmask |= mic_pred_bit(units[i].width);
        const uint64_t len = ends[i] - begins[i];
        u.comp_in = d_blobs + begins[i]; u.comp_len = (uint32_t)len;
        u.px_out = d_pixels_out + units[i].px_offset;
        u.w = units[i].width; u.h = units[i].height;
        u.pred = (units[i].nstates & MIC_HIP_PRED_GRAD) ? 1u : 0u; any_grad |= u.pred != 0;
        if (units[i].nstates & MIC_HIP_GAP_REMOVAL) { u.gap = 1; u.gap_buf = (uint8_t *)s->gap.p + (size_t)mic_gap_stride((uint32_t)s->tab_syms) * (size_t)i; }
        u.tok_cap = (uint32_t)tok_cap_tier((size_t)u.w * (size_t)u.h, tier);
        u.sym_cap = (uint32_t)std::min<size_t>(tok_cap_for((size_t)u.w * (size_t)u.h) + 64, 0xFFFFFFF0u);   // (a bound on the symbols a frame can use, not a slab size: the symbol slab is idle on this side)
    }
    const int variant = s->variant | (any_grad ? MIC_VARIANT_GRAD : 0) | (any_gap ? MIC_VARIANT_GAP : 0);
    if ((rc = s->run_decode(mic_hip_session::FlagSlab::Clear, [&] {
            mic_launch_decode((MicUnit *)s->units.p, n, s->stream, variant, &s->timer, (int *)s->cls.p, rows_kmask, s->dec_classes.mask(), &s->split_cfg); }))) return rc;
    s->learn_decode = true;
    HIP_TRY(hipMemcpyAsync(s->h_units.data(), s->units.p, sizeof(MicUnit) * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    s->readback_queued = true;
    return MIC_OK;
}

int session_decode_finish(mic_hip_session *s, int32_t *h_status) {
    int n = s->n_last;
    if (n <= 0) return MIC_ERR_ARGS;
    { const int frc = finish_units(s, n); if (frc) return frc; }
    learn_classes(s, n);
    for (int i = 0; i < n; i++) h_status[i] = s->h_units[(size_t)i].status;
    return MIC_OK;
}

// ---- digests and compares (mic_verify.hip) -------------------------------------------------------
// The host's part: the chunk -> unit table of the flat grid (a unit's body is cut from its END, mic_verify.h), built the way the
// readers build their piece lists; one upload, two launches, one download; the CRC's init and final xor once per unit.
int session_digest_run(mic_hip_session *s, const uint16_t *d_ref, const uint16_t *d_dec, const mic_hip_unit *units, int n,
                       const uint8_t *compare, mic_hip_verify_result *res) {
    if (n <= 0) return MIC_ERR_ARGS;
    for (int i = 0; i < n; i++) {
        if (units[i].width <= 0 || units[i].height <= 0) return MIC_ERR_ARGS;
        if ((size_t)units[i].width * (size_t)units[i].height > ((size_t)1 << 28)) return MIC_ERR_UNSUPPORTED;   // (a pixel index fits the kernels' 32 bits)
    }
    if (d_dec && (((uintptr_t)d_ref ^ (uintptr_t)d_dec) & 15u)) return MIC_ERR_INTERNAL;   // (the two copies share their 16-byte boundaries: mic_verify.h)
    if (!s->stream) HIP_TRY(mic_stream_create(&s->stream));
    const size_t units_bytes = align_up(sizeof(MicVerifyUnit) * (size_t)n, 16);
    s->verify_up.resize(units_bytes);
    std::vector<uint32_t> first_chunk((size_t)n + 1);
    uint64_t nchunks = 0;
    bool any_compare = false;
    for (int i = 0; i < n; i++) {
        const uint64_t npx = (uint64_t)units[i].width * (uint64_t)units[i].height;
        const uint16_t *ref = d_ref + units[i].px_offset;
        const uint64_t base = (uint64_t)(uintptr_t)ref;
        const int64_t body = (int64_t)(((base + 2 * npx) & ~(uint64_t)15) - base);
        const uint64_t nch = body > 0 ? ((uint64_t)body + MIC_VFY_CHUNK_BYTES - 1) / MIC_VFY_CHUNK_BYTES : 0;
        const bool cmp = d_dec && (!compare || compare[i]);
        any_compare |= cmp;
        MicVerifyUnit vu{ ref, cmp ? d_dec + units[i].px_offset : nullptr, npx, (uint32_t)nchunks, (uint32_t)nch };
        memcpy(s->verify_up.data() + sizeof(MicVerifyUnit) * (size_t)i, &vu, sizeof vu);
        first_chunk[(size_t)i] = (uint32_t)nchunks;
        nchunks += nch;
        if (nchunks > 0x7FFFFFFFull) return MIC_ERR_UNSUPPORTED;           // (a launch's grid)
    }
    first_chunk[(size_t)n] = (uint32_t)nchunks;
    const size_t table_bytes = align_up(4 * (size_t)nchunks, 16);
    s->verify_up.resize(units_bytes + table_bytes);
    uint32_t *tab = (uint32_t *)(s->verify_up.data() + units_bytes);
    for (int i = 0; i < n; i++) std::fill(tab + first_chunk[(size_t)i], tab + first_chunk[(size_t)i + 1], (uint32_t)i);
    // device layout: [unit records][chunk -> unit][chunk registers][mism n x u64][first n x u64][reg n x u32]
    const size_t off_partial = units_bytes + table_bytes, off_mism = off_partial + table_bytes, off_first = off_mism + 8 * (size_t)n,
                 off_reg = off_first + 8 * (size_t)n, total = off_reg + align_up(4 * (size_t)n, 8);
    int rc = s->verify_tab.reserve(total);
    if (rc) return rc;
    char *d = (char *)s->verify_tab.p;
    HIP_TRY(hipMemcpyAsync(d, s->verify_up.data(), units_bytes + table_bytes, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemsetAsync(d + off_mism, 0, 8 * (size_t)n, s->stream));
    HIP_TRY(hipMemsetAsync(d + off_first, 0xFF, 8 * (size_t)n, s->stream));
    s->timer.stream = s->stream;
    mic_launch_units_digest((const MicVerifyUnit *)d, n, (const uint32_t *)(d + units_bytes), (uint32_t)nchunks, any_compare, (uint32_t *)(d + off_partial),
                            (uint32_t *)(d + off_reg), (unsigned long long *)(d + off_mism), (unsigned long long *)(d + off_first), s->stream, &s->timer);
    HIP_TRY(hipGetLastError());
    s->verify_down.resize((total - off_mism) / 8);
    HIP_TRY(hipMemcpyAsync(s->verify_down.data(), d + off_mism, total - off_mism, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const uint64_t *mism = s->verify_down.data(), *first = mism + n;
    const uint32_t *reg = (const uint32_t *)(first + n);
    for (int i = 0; i < n; i++) {
        const uint64_t bytes = 2 * (uint64_t)units[i].width * (uint64_t)units[i].height;
        auto it = s->verify_init.find(bytes);
        if (it == s->verify_init.end()) {
            if (s->verify_init.size() > 4096) s->verify_init.clear();
            it = s->verify_init.emplace(bytes, mic_crc_mul(0xFFFFFFFFu, mic_crc_xpow8(bytes))).first;
        }
        res[i].crc32 = reg[i] ^ it->second ^ 0xFFFFFFFFu;
        res[i].mismatches = mism[i];
        res[i].first_mismatch = first[i] == ~0ull ? -1 : (int64_t)first[i];
    }
    return MIC_OK;
}

int session_verify(mic_hip_session *s, const uint8_t *d_base, const uint64_t *begins, const uint64_t *ends, const mic_hip_unit *units, int n,
                   const uint16_t *d_ref, const int32_t *skip, mic_hip_verify_result *res) {
    if (n <= 0) return MIC_ERR_ARGS;
    // the units that are decoded, in their order; each keeps its px_offset in the scratch buffer
    std::vector<int> idx;
    std::vector<mic_hip_unit> du; std::vector<uint64_t> b, e;
    size_t extent = 0;
    for (int i = 0; i < n; i++) {
        if (units[i].width <= 0 || units[i].height <= 0) return MIC_ERR_ARGS;
        res[i].status = skip ? skip[i] : MIC_OK;
        if (res[i].status != MIC_OK) continue;
        idx.push_back(i); du.push_back(units[i]); b.push_back(begins[i]); e.push_back(ends[i]);
        extent = std::max(extent, (size_t)units[i].px_offset + (size_t)units[i].width * (size_t)units[i].height);
    }
    std::vector<uint8_t> cmp((size_t)n, 0);
    uint16_t *d_dec = nullptr;
    if (!idx.empty()) {
        int rc = s->verify_px.reserve(extent * 2 + 16 + 64);
        if (rc) return rc;
        // (the scratch copy starts where the reference does modulo 16, whatever the caller's pointer: the compare kernel's 16-byte loads then serve both)
        d_dec = (uint16_t *)((char *)s->verify_px.p + ((uintptr_t)d_ref & 15u));
        std::vector<int32_t> st(idx.size());
        if ((rc = session_decode_enqueue_spans(s, d_base, b.data(), e.data(), du.data(), (int)idx.size(), d_dec))) return rc;
        // (the compare is launched behind the finish: a tier-1 chain that ran again in tier 2 wrote the pixels twice, and these are the run that counted)
        if ((rc = session_decode_finish(s, st.data()))) return rc;
        for (size_t k = 0; k < idx.size(); k++) { res[idx[k]].status = st[k]; cmp[(size_t)idx[k]] = st[k] == MIC_OK; }
    }
    const int rc = session_digest_run(s, d_ref, d_dec, units, n, cmp.data(), res);
    if (rc) return rc;
    for (int i = 0; i < n; i++) if (res[i].status == MIC_OK && res[i].mismatches) res[i].status = MIC_ERR_MISMATCH;
    return MIC_OK;
}

// (the host-pointer batch and container entry points live in mic_host_io.hip)

size_t unit_ws_bytes_tier(size_t px, int tier) {
    const size_t tokc = tok_cap_tier(px, tier), ts = tab_syms_tier(tier);
    return tokc * 4 + blob_cap_tok(tokc) + seg_cap_tier(px, tier) * 8 + px / 8 + ts * 4 * 6 + ts * 2 + 8192;
}
size_t unit_ws_bytes(size_t px) { return unit_ws_bytes_tier(px, 2); }      // (the paths that lay their units out themselves: tier 2)
// Units of px pixels (x `mult` slabs each) a sub-batch of the tiered unit codec may hold: tier-1 slabs under the workspace ceiling --
// and tier-2 slabs, should the batch have to run again, inside nine tenths of what the device can give this session.
// `extra`: bytes per unit the caller holds beside the slabs (the host path's staging halves).
size_t batch_units_for(size_t px, size_t mult, size_t extra) {
    const size_t n1 = workspace_budget() / (mult * (unit_ws_bytes_tier(px, 1) + extra));
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = (size_t)32 << 30; }
    const size_t held = tl_default ? tl_default->reserved_bytes() : 0;
    const size_t n2 = (size_t)((double)(fr / leased_here() + held) * 0.9) / (mult * (unit_ws_bytes_tier(px, 2) + extra));
    return std::max<size_t>(1, std::min(n1, n2));
}

}  // namespace micapi

// ================================================================================ C ABI

extern "C" {

const char *mic_hip_version(void) { return "mic-hip 0.2 (gfx950)"; }

// device -> device copy on the calling thread's current device, complete on return (a session's result buffers are reused by its
// next call: a caller that keeps them copies them out)
int mic_hip_device_copy(void *d_dst, const void *d_src, size_t bytes) try {
    if ((!d_dst || !d_src) && bytes) return MIC_ERR_ARGS;
    if (bytes) HIP_TRY(hipMemcpy(d_dst, d_src, bytes, hipMemcpyDeviceToDevice));
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_set_device(int device) try { return mic_hip_set_devices(&device, 1); } MIC_ABI_CATCH

int mic_hip_set_devices(const int *devices, int n) try {
    if (!devices || n <= 0 || n > 64) return MIC_ERR_ARGS;
    for (int i = 0; i < n; i++) {
        if (devices[i] < 0) return MIC_ERR_ARGS;
        const int rc = check_device(devices[i]);
        if (rc) return rc;
    }
    std::unique_lock<std::mutex> lk(g_mu);
    // the pools move with the list: wait for every leased session to come back, then drop those of devices that left it
    auto all_home = [&] { for (auto &kv : g_pools) if ((int)kv.second.free_.size() != kv.second.made) return false; return true; };
    while (!all_home()) g_pool_cv.wait(lk);
    for (auto it = g_pools.begin(); it != g_pools.end();) {
        if (std::find(devices, devices + n, it->first) == devices + n) {
            for (mic_hip_session *p : it->second.free_) { (void)p->activate(); p->release(); delete p; }
            it = g_pools.erase(it);
        } else ++it;
    }
    g_devices.assign(devices, devices + n);
    if (g_device != devices[0]) g_device_ok = false;
    g_device = devices[0];
    return ensure_device_locked();
} MIC_ABI_CATCH
int mic_hip_get_devices(int *devices, int cap) try {
    std::lock_guard<std::mutex> lk(g_mu);
    for (int i = 0; i < (int)g_devices.size() && i < cap; i++) if (devices) devices[i] = g_devices[(size_t)i];
    return (int)g_devices.size();
} MIC_ABI_CATCH

const char *mic_hip_device_name(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (ensure_device_locked() != MIC_OK) return "";
    return g_device_name.c_str();
}

int mic_hip_compress_frame(const uint16_t *pixels, int width, int height, uint16_t max_value, int nstates,
                           uint8_t *out, size_t out_cap, size_t *out_len) try {
    if (!pixels || !out || !out_len || width <= 0 || height <= 0) return MIC_ERR_ARGS;
    mic_hip_enc_job j{};
    j.pixels = pixels; j.width = width; j.height = height; j.max_value = max_value; j.nstates = (uint16_t)nstates;
    j.out = out; j.out_cap = out_cap;
    if (!(nstates == 2 || nstates == 4 || nstates == 8)) return MIC_ERR_ARGS;
    int rc = mic_hip_compress_batch(&j, 1);
    if (rc) return rc;
    if (j.status == MIC_OK) *out_len = j.out_len;
    return j.status;
} MIC_ABI_CATCH

int mic_hip_decompress_frame(const uint8_t *compressed, size_t compressed_len, uint16_t *pixels_out, int width, int height) try {
    if (!compressed || !pixels_out || width <= 0 || height <= 0) return MIC_ERR_ARGS;
    mic_hip_dec_job j{};
    j.compressed = compressed; j.compressed_len = compressed_len; j.pixels_out = pixels_out; j.width = width; j.height = height;
    int rc = mic_hip_decompress_batch(&j, 1);
    if (rc) return rc;
    return j.status;
} MIC_ABI_CATCH

// ---- gap removal (gapremovalcompressu16.go:52-282): the unit codec with MIC_HIP_GAP_REMOVAL, through the batch pipeline
int mic_hip_compress_frame_gap(const uint16_t *pixels, int width, int height, uint16_t max_value, int nstates,
                               uint8_t *out, size_t out_cap, size_t *out_len) try {
    if (!pixels || !out || !out_len || width <= 0 || height <= 0) return MIC_ERR_ARGS;
    if (!(nstates == 2 || nstates == 4 || nstates == 8)) return MIC_ERR_ARGS;
    mic_hip_enc_job j{};
    j.pixels = pixels; j.width = width; j.height = height; j.max_value = max_value; j.nstates = (uint16_t)nstates;
    j.out = out; j.out_cap = out_cap;
    int rc = mic_hip_compress_batch_gap(&j, 1);
    if (rc) return rc;
    if (j.status == MIC_OK) *out_len = j.out_len;
    return j.status;
} MIC_ABI_CATCH

int mic_hip_decompress_frame_gap(const uint8_t *compressed, size_t compressed_len, uint16_t *pixels_out, int width, int height) try {
    if (!compressed || !pixels_out || width <= 0 || height <= 0) return MIC_ERR_ARGS;
    mic_hip_dec_job j{};
    j.compressed = compressed; j.compressed_len = compressed_len; j.pixels_out = pixels_out; j.width = width; j.height = height;
    int rc = mic_hip_decompress_batch_gap(&j, 1);
    if (rc) return rc;
    return j.status;
} MIC_ABI_CATCH

// ---- bare FSE stage (fsecompressu16.go:19, fse2state.go:22/102, fse4state.go:24, fse8state.go:31, rans8state.go:31)
int mic_hip_fse_compress_u16(const uint16_t *symbols, size_t n, int flavour, uint8_t *out, size_t out_cap, size_t *out_len) try {
    return mic_hip_fse_compress_u16_ex(symbols, n, flavour, 0, out, out_cap, out_len);
} MIC_ABI_CATCH

int mic_hip_fse_compress_u16_ex(const uint16_t *symbols, size_t n, int flavour, int table_log, uint8_t *out, size_t out_cap, size_t *out_len) try {
    if (!symbols || !out || !out_len) return MIC_ERR_ARGS;
    if (!(flavour == 1 || flavour == 2 || flavour == 4 || flavour == 8 || flavour == 108)) return MIC_ERR_ARGS;
    if (table_log < 0 || table_log > MIC_MAX_TABLELOG) return MIC_ERR_ARGS;   // prepare(): "tableLog (%d) > maxTableLog (%d)", fseu16.go:136-138
    if (n <= 1) return MIC_ERR_INCOMPRESSIBLE;                          // first gate of every FSECompressU16* variant
    if (n > ((size_t)1 << 30)) return MIC_ERR_UNSUPPORTED;
    DefaultLease lease;
    int rc = lease.acquire();
    if (rc) return rc;
    mic_hip_session *s = cur_default();
    const size_t px = (n + 3) / 4 + 16;
    if ((rc = s->lay_out(1, px))) return rc;
    if ((rc = s->io_px.reserve(n * 2 + 64))) return rc;
    HIP_TRY(hipMemcpyAsync(s->io_px.p, symbols, n * 2, hipMemcpyHostToDevice, s->stream));
    MicUnit &u = s->h_units[0];
    u.px_in = (const uint16_t *)s->io_px.p; u.w = (int32_t)n; u.h = 1; u.max_value = 0;
    u.nstates = (uint16_t)flavour; u.mode = 1; u.no_fallback = 1; u.req_tl = (uint32_t)table_log;
    if ((rc = s->run_encode([&] { mic_launch_encode((MicUnit *)s->units.p, 1, s->stream, s->variant, nullptr); }))) return rc;
    uint64_t offs[2]; int32_t st = 0, ns = 0; const uint8_t *d_blobs = nullptr;
    if ((rc = session_encode_finish(s, &d_blobs, offs, &st, &ns))) return rc;
    if (st != MIC_OK) return st;
    const size_t len = (size_t)offs[1];
    if (len > out_cap) return MIC_ERR_CAPACITY;
    HIP_TRY(hipMemcpy(out, d_blobs, len, hipMemcpyDeviceToHost));
    *out_len = len;
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_fse_decompress_u16_auto(const uint8_t *in, size_t in_len, uint16_t *out, size_t out_cap, size_t *out_n) try {
    return mic_hip_fse_decompress_u16_ex(in, in_len, 0, out, out_cap, out_n);
} MIC_ABI_CATCH

// ScratchU16.DecompressLimit (fseu16.go:87-91): the reference compares len(OutU16) with the limit every time its 65536-symbol ring
// wraps (fse2state.go:249/283, fse4state.go:246/..., fse8state.go, fsedecompressu16.go:318/353) and, for 1-state streams, once more
// at the end (fsedecompressu16.go:372): an N-state stream of `count` symbols fails iff floor(count / 65536) * 65536 >= limit,
// a 1-state stream iff its symbol count >= limit.  0 = the default, 2 GiB - 1.
int mic_hip_fse_decompress_u16_ex(const uint8_t *in, size_t in_len, int64_t decompress_limit, uint16_t *out, size_t out_cap, size_t *out_n) try {
    if (decompress_limit < 0) return MIC_ERR_ARGS;
    const uint64_t limit = decompress_limit ? (uint64_t)decompress_limit : ((2ull << 30) - 1);
    if (in && in_len >= 6 && in[0] == 0xFF && (in[1] == 0x02 || in[1] == 0x04 || in[1] == 0x84 || in[1] == 0x08)) {
        const uint64_t count = (uint64_t)in[2] | ((uint64_t)in[3] << 8) | ((uint64_t)in[4] << 16) | ((uint64_t)in[5] << 24);
        if (count >= 65536 && (count / 65536) * 65536 >= limit) return MIC_ERR_CAPACITY;   // "output size (%d) > DecompressLimit (%d)"
    }
    if (!in || !out || !out_n || in_len == 0) return in && in_len == 0 ? MIC_ERR_CORRUPT : MIC_ERR_ARGS;
    if (in_len > 0xFFFFFFF0ull || out_cap > ((size_t)1 << 30)) return MIC_ERR_UNSUPPORTED;
    DefaultLease lease;
    int rc = lease.acquire();
    if (rc) return rc;
    mic_hip_session *s = cur_default();
    const size_t px = (out_cap + 3) / 4 + 16;
    if ((rc = s->lay_out(1, px))) return rc;
    if ((rc = s->io_comp.reserve(in_len + 64))) return rc;
    HIP_TRY(hipMemcpyAsync(s->io_comp.p, in, in_len, hipMemcpyHostToDevice, s->stream));
    MicUnit &u = s->h_units[0];
    u.comp_in = (const uint8_t *)s->io_comp.p; u.comp_len = (uint32_t)in_len; u.w = 1; u.h = 1; u.mode = 1;
    u.tok_cap = (uint32_t)std::min<size_t>(out_cap, u.tok_cap);
    if ((rc = s->run_decode(mic_hip_session::FlagSlab::Idle, [&] { mic_launch_decode((MicUnit *)s->units.p, 1, s->stream, s->variant, nullptr, (int *)s->cls.p); }))) return rc;
    int32_t st = 0;
    if ((rc = session_decode_finish(s, &st))) return rc;
    if (st != MIC_OK) return st;
    const size_t n = s->h_units[0].ntok;
    if (s->h_units[0].flavour == 1 && (uint64_t)n >= limit) return MIC_ERR_CAPACITY;        // fsedecompressu16.go:372
    if (n > out_cap) return MIC_ERR_CAPACITY;
    if (n) HIP_TRY(hipMemcpy(out, s->h_units[0].tok, n * 2, hipMemcpyDeviceToHost));
    *out_n = n;
    return MIC_OK;
} MIC_ABI_CATCH

// ---- PICS / MIC2 headers (the container codecs themselves: mic_host_io.hip) ------------------------
int mic_hip_pics_info(const uint8_t *c, size_t len, int *width, int *height, int *num_strips, int *strip_height) try {
    if (!c) return MIC_ERR_ARGS;
    if (len < 20 || memcmp(c, "PICS", 4) != 0) return MIC_ERR_CORRUPT;   // parallelstrips.go:271-273
    int w = (int)get_u32(c + 4), h = (int)get_u32(c + 8), n = (int)get_u32(c + 12), sh = (int)get_u32(c + 16);
    if (n < 0 || (size_t)n > (len - 20) / 8) return MIC_ERR_CORRUPT;     // truncated header, :281-283
    if (w <= 0 || h <= 0 || n <= 0 || sh <= 0) return MIC_ERR_CORRUPT;   // :284-286
    if (width) *width = w; if (height) *height = h; if (num_strips) *num_strips = n; if (strip_height) *strip_height = sh;
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_mic2_compress_temporal(const uint16_t *frames, int width, int height, int nframes, uint16_t max_value,
                                   uint8_t *out, size_t out_cap, size_t *out_len) try {
    if (!frames || !out || !out_len || width <= 0 || height <= 0 || nframes <= 0) return MIC_ERR_ARGS;
    return mic2_temporal_compress(frames, width, height, nframes, max_value, out, out_cap, out_len);
} MIC_ABI_CATCH

int mic_hip_mic2_info(const uint8_t *c, size_t len, int *width, int *height, int *nframes, int *temporal) try {
    if (!c) return MIC_ERR_ARGS;
    if (len < 20 || memcmp(c, "MIC2", 4) != 0) return MIC_ERR_CORRUPT;   // multiframe.go:96-103
    int w = (int)get_u32(c + 4), h = (int)get_u32(c + 8), n = (int)get_u32(c + 12);
    if (n < 0 || (size_t)n > (len - 20) / 8) return MIC_ERR_CORRUPT;     // :112-116
    if (width) *width = w; if (height) *height = h; if (nframes) *nframes = n; if (temporal) *temporal = (c[16] & 0x02) != 0;
    return MIC_OK;
} MIC_ABI_CATCH

// DecompressFrame (multiframecompress.go:266-315): one frame of a MIC2 file.  Independent mode decodes just that
// frame; temporal mode needs frames 0..idx (all their residual streams are decoded at once, mic_mic2_batch.hip).
int mic_hip_mic2_decompress_frame(const uint8_t *c, size_t len, int frame_idx, uint16_t *pixels_out, size_t pixels_cap) try {
    if (!c || !pixels_out) return MIC_ERR_ARGS;
    int w, h, n, temporal;
    int rc = mic_hip_mic2_info(c, len, &w, &h, &n, &temporal);
    if (rc) return rc;
    if (frame_idx < 0 || frame_idx >= n) return MIC_ERR_ARGS;           // "frame index out of range"
    if (w <= 0 || h <= 0) return MIC_ERR_CORRUPT;
    const size_t npx = (size_t)w * (size_t)h;
    if (npx > pixels_cap) return MIC_ERR_CAPACITY;
    const size_t data_off = 20 + (size_t)n * 8;
    if (!temporal) {
        const size_t start = data_off + get_u32(c + 20 + (size_t)frame_idx * 8), bl = get_u32(c + 24 + (size_t)frame_idx * 8);
        if (start + bl > len) return MIC_ERR_CORRUPT;                     // ExtractFrame, multiframe.go:131-142
        return mic_hip_decompress_frame(c + start, bl, pixels_out, w, h);
    }
    std::vector<uint16_t> tmp(npx * (size_t)(frame_idx + 1));
    rc = mic2_temporal_decompress(c, len, w, h, n, frame_idx + 1, tmp.data());
    if (rc) return rc;
    memcpy(pixels_out, tmp.data() + npx * (size_t)frame_idx, npx * 2);
    return MIC_OK;
} MIC_ABI_CATCH

// ---- sessions ------------------------------------------------------------------------------------
int mic_hip_session_create_on(int device, mic_hip_session **out, int max_units, size_t max_px_per_unit) try {
    if (!out || max_units <= 0 || max_px_per_unit == 0) return MIC_ERR_ARGS;
    int rc = check_device(device);
    if (rc) return rc;
    mic_hip_session *s = new mic_hip_session();
    s->device = device;
    if ((rc = s->activate())) { delete s; return rc; }
    rc = s->ensure(max_units, max_px_per_unit, 1);                      // tier-1 slabs; a batch that needs the big ones grows them
    if (rc) { s->release(); delete s; return rc; }
    *out = s;
    return MIC_OK;
} MIC_ABI_CATCH
int mic_hip_session_create(mic_hip_session **out, int max_units, size_t max_px_per_unit) try {
    int dev;
    { std::lock_guard<std::mutex> lk(g_mu); dev = g_device; }
    return mic_hip_session_create_on(dev, out, max_units, max_px_per_unit);
} MIC_ABI_CATCH
int mic_hip_session_device(mic_hip_session *s) try { return s ? s->device : -1; } MIC_ABI_CATCH
// device memory the session holds right now (workspace slabs, staging, stores), and whether a batch has needed the tier-2 slabs
size_t mic_hip_session_workspace_bytes(mic_hip_session *s, int *tier2) {
    if (!s) return 0;
    if (tier2) *tier2 = s->force_big ? 1 : 0;
    return s->reserved_bytes();
}
void mic_hip_session_destroy(mic_hip_session *s) { if (s) { (void)s->activate(); s->release(); delete s; } }
void *mic_hip_session_stream(mic_hip_session *s) { return s ? (void *)s->stream : nullptr; }

int mic_hip_session_encode_enqueue(mic_hip_session *s, const uint16_t *d_pixels, const mic_hip_unit *units, int n) try {
    if (!s || !d_pixels || !units) return MIC_ERR_ARGS;
    { const int arc = s->activate(); if (arc) return arc; }
    return session_encode_enqueue(s, d_pixels, units, n);
} MIC_ABI_CATCH
int mic_hip_session_encode_finish(mic_hip_session *s, const uint8_t **d_blobs, uint64_t *h_offsets, int32_t *h_status, int32_t *h_nstates) try {
    if (!s || !h_offsets || !h_status) return MIC_ERR_ARGS;
    { const int arc = s->activate(); if (arc) return arc; }
    return session_encode_finish(s, d_blobs, h_offsets, h_status, h_nstates);
} MIC_ABI_CATCH
int mic_hip_session_encode(mic_hip_session *s, const uint16_t *d_pixels, const mic_hip_unit *units, int n,
                           const uint8_t **d_blobs, uint64_t *h_offsets, int32_t *h_status, int32_t *h_nstates) try {
    int rc = mic_hip_session_encode_enqueue(s, d_pixels, units, n);
    if (rc) return rc;
    return mic_hip_session_encode_finish(s, d_blobs, h_offsets, h_status, h_nstates);
} MIC_ABI_CATCH
int mic_hip_session_decode_enqueue(mic_hip_session *s, const uint8_t *d_blobs, const uint64_t *h_offsets,
                                   const mic_hip_unit *units, int n, uint16_t *d_pixels_out) try {
    if (!s || !d_blobs || !h_offsets || !units || !d_pixels_out) return MIC_ERR_ARGS;
    { const int arc = s->activate(); if (arc) return arc; }
    return session_decode_enqueue(s, d_blobs, h_offsets, units, n, d_pixels_out);
} MIC_ABI_CATCH
int mic_hip_session_decode_finish(mic_hip_session *s, int32_t *h_status) try {
    if (!s || !h_status) return MIC_ERR_ARGS;
    { const int arc = s->activate(); if (arc) return arc; }
    return session_decode_finish(s, h_status);
} MIC_ABI_CATCH
int mic_hip_session_decode(mic_hip_session *s, const uint8_t *d_blobs, const uint64_t *h_offsets, const mic_hip_unit *units, int n,
                           uint16_t *d_pixels_out, int32_t *h_status) try {
    int rc = mic_hip_session_decode_enqueue(s, d_blobs, h_offsets, units, n, d_pixels_out);
    if (rc) return rc;
    return mic_hip_session_decode_finish(s, h_status);
} MIC_ABI_CATCH
// ---- digests, verify, verified encode (session_digest_run / session_verify above)
int mic_hip_session_digest(mic_hip_session *s, const uint16_t *d_pixels, const mic_hip_unit *units, int n, uint32_t *h_crc) try {
    if (!s || !d_pixels || !units || !h_crc || n <= 0) return MIC_ERR_ARGS;
    { const int arc = s->activate(); if (arc) return arc; }
    std::vector<mic_hip_verify_result> res((size_t)n);
    s->timer.reset(s->stream);
    const int rc = session_digest_run(s, d_pixels, nullptr, units, n, nullptr, res.data());
    if (rc) return rc;
    for (int i = 0; i < n; i++) h_crc[i] = res[(size_t)i].crc32;
    return MIC_OK;
} MIC_ABI_CATCH
int mic_hip_session_verify(mic_hip_session *s, const uint8_t *d_blobs, const uint64_t *h_offsets, const mic_hip_unit *units, int n,
                           const uint16_t *d_pixels_ref, mic_hip_verify_result *h_res) try {
    if (!s || !d_blobs || !h_offsets || !units || !d_pixels_ref || !h_res || n <= 0) return MIC_ERR_ARGS;
    { const int arc = s->activate(); if (arc) return arc; }
    return session_verify(s, d_blobs, h_offsets, h_offsets + 1, units, n, d_pixels_ref, nullptr, h_res);
} MIC_ABI_CATCH
int mic_hip_session_encode_verified(mic_hip_session *s, const uint16_t *d_pixels, const mic_hip_unit *units, int n,
                                    const uint8_t **d_blobs, uint64_t *h_offsets, int32_t *h_nstates, mic_hip_verify_result *h_res) try {
    if (!s || !d_pixels || !units || !h_offsets || !h_res || n <= 0) return MIC_ERR_ARGS;
    { const int arc = s->activate(); if (arc) return arc; }
    std::vector<int32_t> st((size_t)n);
    const uint8_t *packed = nullptr;
    int rc = session_encode_enqueue(s, d_pixels, units, n);
    if (rc == MIC_OK) rc = session_encode_finish(s, &packed, h_offsets, st.data(), h_nstates);
    if (rc) return rc;
    if (d_blobs) *d_blobs = packed;
    // (the packed buffer is no slab of the workspace: it stands while the decode lays the workspace out anew)
    return session_verify(s, packed, h_offsets, h_offsets + 1, units, n, d_pixels, st.data(), h_res);
} MIC_ABI_CATCH
// debug probe (not in the public header): the digest kernels' geometry in PIXELS -- out[0] a lane's run, out[1] a wave's, out[2] a
// work-group's chunk (mic_verify.h); tests aim units at these seams
int mic_hip_debug_verify_geometry(uint32_t *out) try {
    if (!out) return MIC_ERR_ARGS;
    out[0] = MIC_VFY_LANE_BYTES / 2; out[1] = MIC_VFY_WAVE_BYTES / 2; out[2] = MIC_VFY_CHUNK_BYTES / 2;
    return MIC_OK;
} MIC_ABI_CATCH
// debug probe (not part of the public header): raw result fields of unit i after a *_finish
int mic_hip_debug_unit(mic_hip_session *s, int i, uint32_t *out8) try {
    if (!s || i < 0 || i >= s->n_last) return MIC_ERR_ARGS;
    const MicUnit &u = s->h_units[(size_t)i];
    out8[0] = u.ntok; out8[1] = u.blob_len; out8[2] = u.table_log; out8[3] = u.symbol_len;
    out8[4] = u.max_count; out8[5] = u.hdr_len; out8[6] = u.zero_bits; out8[7] = u.flavour;
    out8[8] = u.count; out8[9] = u.bits_off; out8[10] = (uint32_t)u.nstates_used; out8[11] = (uint32_t)u.status; out8[12] = u.nseg; out8[13] = u.nsym; out8[14] = u.seg_cap;
    out8[15] = u.dec_kernel;                                             // 1 + lane-per-state class, MIC_DEC_BY_GL, MIC_DEC_BY_SERIAL; 0: no tANS kernel took the unit
    for (int k = 0; k < 16; k++) out8[16 + k] = u.dbg[k];
    return MIC_OK;
} MIC_ABI_CATCH
// debug probe (not in the public header): what a split two-state decode instance made of unit i after a decode's *_finish --
// out[0]: MIC_SPLIT_* (mic_dev.h: 0 not tried, 1 split, 2 .. fell back and why), out[1]: i_sync (I_1), out[2]: j_sync (W)
int mic_hip_debug_split(mic_hip_session *s, int i, uint32_t *out) try {
    if (!s || !out || i < 0 || i >= s->n_last) return MIC_ERR_ARGS;
    for (int k = 0; k < 3; k++) out[k] = s->h_units[(size_t)i].split[k];
    return MIC_OK;
} MIC_ABI_CATCH
// debug setter (not in the public header): the session's split gate and overlap (MicSplitCfg, mic_dev.h); a zero keeps a value.
// The session forgets its launch masks, so the next batch is classified under the new values.
int mic_hip_debug_split_config(mic_hip_session *s, uint32_t min_tokens, uint32_t overlap, uint32_t min_bits16) try {
    if (!s || (overlap && (overlap < 64u || (overlap & 63u)))) return MIC_ERR_ARGS;
    if (min_tokens) s->split_cfg.min_tokens = min_tokens;
    if (overlap) s->split_cfg.overlap = overlap;
    if (min_bits16) s->split_cfg.min_bits16 = min_bits16;
    s->dec_classes = mic_hip_session::ClsMemory{};
    return MIC_OK;
} MIC_ABI_CATCH
// debug probe (not in the public header): the four-part instance's record of unit i after a decode's *_finish -- out[0]: MIC_SPLIT_*,
// out[1..3]: I_1, I_2, I_3 (token indices of the joins), out[4]: W, out[5]: R (0: not a four-part unit), out[6]: the failing boundary;
// of any other unit out[1..3], out[5] and out[6] are 0
int mic_hip_debug_split4(mic_hip_session *s, int i, uint32_t *out) try {
    if (!s || !out || i < 0 || i >= s->n_last) return MIC_ERR_ARGS;
    const uint32_t *r = s->h_units[(size_t)i].split;
    const uint32_t m = r[7] == 4u ? ~0u : 0u;
    out[0] = r[0]; out[1] = r[1] & m; out[2] = r[3] & m; out[3] = r[4] & m; out[4] = r[2]; out[5] = r[5] & m; out[6] = r[6] & m;
    return MIC_OK;
} MIC_ABI_CATCH
// debug setter (not in the public header): the length from which on a unit that passes the split gate goes to the four-part instance
// (MicSplitCfg::min_tokens4); a zero keeps the value.  The session forgets its launch masks, as above.
int mic_hip_debug_split4_config(mic_hip_session *s, uint32_t min_tokens4) try {
    if (!s) return MIC_ERR_ARGS;
    if (min_tokens4) s->split_cfg.min_tokens4 = min_tokens4;
    s->dec_classes = mic_hip_session::ClsMemory{};
    return MIC_OK;
} MIC_ABI_CATCH
// debug probe (not in the public header): the eight-part instance's record of unit i after a decode's *_finish -- out[0]: MIC_SPLIT_*,
// out[1..7]: I_1 .. I_7, out[8]: W, out[9]: R (0: not an eight-part unit -- one it handed back carries the four-part instance's
// record), out[10]: the failing boundary, out[11]: parts; of any other unit out[1..7], out[9] and out[10] are 0
int mic_hip_debug_split8(mic_hip_session *s, int i, uint32_t *out) try {
    if (!s || !out || i < 0 || i >= s->n_last) return MIC_ERR_ARGS;
    const MicUnit &u = s->h_units[(size_t)i];
    const uint32_t *r = u.split;
    const uint32_t m = r[7] == 8u ? ~0u : 0u;
    out[0] = r[0]; out[1] = r[1] & m; out[2] = r[3] & m; out[3] = r[4] & m;
    for (int k = 0; k < 4; k++) out[4 + k] = u.split_hi[k] & m;
    out[8] = r[2]; out[9] = r[5] & m; out[10] = r[6] & m; out[11] = r[7];
    return MIC_OK;
} MIC_ABI_CATCH
// debug setter (not in the public header): the length from which on a unit of the four-part list goes to the eight-part instance
// (MicSplitCfg::min_tokens8); a zero keeps the value.  The session forgets its launch masks, as above.
int mic_hip_debug_split8_config(mic_hip_session *s, uint32_t min_tokens8) try {
    if (!s) return MIC_ERR_ARGS;
    if (min_tokens8) s->split_cfg.min_tokens8 = min_tokens8;
    s->dec_classes = mic_hip_session::ClsMemory{};
    return MIC_OK;
} MIC_ABI_CATCH
// debug probe (not in the public header): who did the eight-part instance's per-chunk upkeep for unit i after a decode's *_finish --
// out[0]: 0 the chain wave, 1 a partner wave, out[1]: chunks the partner served, out[2]: chunks the chain wave found its partner not
// ready for, out[3]: stalled (MicUnit.partner; zeros of a unit the eight-part instance did not run)
int mic_hip_debug_partner(mic_hip_session *s, int i, uint32_t *out) try {
    if (!s || !out || i < 0 || i >= s->n_last) return MIC_ERR_ARGS;
    for (int k = 0; k < 4; k++) out[k] = s->h_units[(size_t)i].partner[k];
    return MIC_OK;
} MIC_ABI_CATCH
// debug setter (not in the public header): polls a chain wave of the eight-part instance waits for its partner wave before it gives
// up (MicSplitCfg::partner_bound; 1: at once); a zero puts the default back
int mic_hip_debug_partner_config(mic_hip_session *s, uint32_t bound) try {
    if (!s) return MIC_ERR_ARGS;
    s->split_cfg.partner_bound = bound ? bound : MicSplitCfg{}.partner_bound;
    return MIC_OK;
} MIC_ABI_CATCH
// debug probe (not in the public header): how far the chain behind the tables brought unit i (MicUnit.dec_stage: MIC_STAGE_*,
// mic_dev.h; 4 = k_dec_rows_tok made its pixels) after a decode's *_finish
int mic_hip_debug_dec_stage(mic_hip_session *s, int i, uint32_t *out) try {
    if (!s || !out || i < 0 || i >= s->n_last) return MIC_ERR_ARGS;
    *out = s->h_units[(size_t)i].dec_stage;
    return MIC_OK;
} MIC_ABI_CATCH
// debug probe (not in the public header): which forks of the tokens-to-pixels stage unit i took (MicUnit.px_paths: MIC_PXP_* bits,
// mic_dev.h -- k_dec_rows_tok's of a unit it made the pixels of, else k_dec_pixels_wg's) after a decode's *_finish
int mic_hip_debug_px_paths(mic_hip_session *s, int i, uint32_t *out) try {
    if (!s || !out || i < 0 || i >= s->n_last) return MIC_ERR_ARGS;
    *out = s->h_units[(size_t)i].px_paths;
    return MIC_OK;
} MIC_ABI_CATCH
// debug probe (not in the public header): mic_dec_cls as this build compiled it, gates and all (tests/test_decode_classes_cpu.py
// holds its own restatement against it, value by value)
int mic_hip_debug_dec_cls(uint32_t flavour, uint32_t table_log, uint32_t zero_bits) { return mic_dec_cls(flavour, table_log, zero_bits); }
// debug probe (not in the public header): bytes of unit i's histogram slab after a *_finish (LS_DEBUG builds dump there)
int mic_hip_debug_fetch_hist(mic_hip_session *s, int i, void *dst, size_t bytes) try {
    if (!s || i < 0 || i >= s->n_last || bytes > kSym * 4) return MIC_ERR_ARGS;
    HIP_TRY(hipMemcpy(dst, s->h_units[(size_t)i].hist, bytes, hipMemcpyDeviceToHost));
    return MIC_OK;
} MIC_ABI_CATCH
// debug probe (not in the public header): the MIC_TK_PATHS route counts k_enc_tokens_wg left in unit i (MIC_TKP_*, mic_dev.h) after an
// encode's *_finish
int mic_hip_debug_tok_paths(mic_hip_session *s, int i, uint32_t *out) try {
    if (!s || !out || i < 0 || i >= s->n_last) return MIC_ERR_ARGS;
    for (int k = 0; k < MIC_TK_PATHS; k++) out[k] = s->h_units[(size_t)i].tk_paths[k];
    return MIC_OK;
} MIC_ABI_CATCH
// debug probe (not in the public header): the first n u16 of unit i's token slab after a *_finish
int mic_hip_debug_fetch_tok(mic_hip_session *s, int i, void *dst, size_t n) try {
    if (!s || i < 0 || i >= s->n_last || n > s->h_units[(size_t)i].tok_cap) return MIC_ERR_ARGS;
    HIP_TRY(hipMemcpy(dst, s->h_units[(size_t)i].tok, n * 2, hipMemcpyDeviceToHost));
    return MIC_OK;
} MIC_ABI_CATCH
// debug probe (not in the public header): the table stage's route record of unit i (MicUnit.tb_route: MIC_TBR_* bits, nbig << 16,
// mic_dev.h) after a *_finish
int mic_hip_debug_tab_route(mic_hip_session *s, int i, uint32_t *out) try {
    if (!s || !out || i < 0 || i >= s->n_last) return MIC_ERR_ARGS;
    *out = s->h_units[(size_t)i].tb_route;
    return MIC_OK;
} MIC_ABI_CATCH
// debug probe (not in the public header): which instance of the table kernel built unit i's tables (MicUnit.tb_inst: MIC_TBI_*,
// mic_dev.h; 0: neither) after a *_finish
int mic_hip_debug_tab_inst(mic_hip_session *s, int i, uint32_t *out) try {
    if (!s || !out || i < 0 || i >= s->n_last) return MIC_ERR_ARGS;
    *out = s->h_units[(size_t)i].tb_inst;
    return MIC_OK;
} MIC_ABI_CATCH
// debug probe (not in the public header): which tANS encode kernel decided unit i (MicUnit.enc_kernel, mic_dev.h) after an encode's
// *_finish.  out[0]: 1 + the bit index of the MIC_ENC_CLS_* class, MIC_ENC_BY_SERIAL, or 0 for nobody; out[1]: MicUnit.enc_rounds,
// the fix-up rounds of the deciding attempt; out[2]: 1 when the two-state instance had handed the unit over (MIC_ENC_HANDED)
int mic_hip_debug_enc_kernel(mic_hip_session *s, int i, uint32_t *out) try {
    if (!s || !out || i < 0 || i >= s->n_last) return MIC_ERR_ARGS;
    const MicUnit &u = s->h_units[(size_t)i];
    out[0] = u.enc_kernel & 0xFFu; out[1] = u.enc_rounds; out[2] = (u.enc_kernel & MIC_ENC_HANDED) ? 1u : 0u;
    return MIC_OK;
} MIC_ABI_CATCH
// debug probe (not in the public header): the head of one of unit i's table slabs after a *_finish.
// which: 0 state_tab (u32), 1 tt_nb (u32), 2 tt_find (i32), 3 tab_sym (u16), 4 norm (i32)
int mic_hip_debug_fetch_table(mic_hip_session *s, int i, int which, void *dst, size_t bytes) try {
    if (!s || !dst || i < 0 || i >= s->n_last || which < 0 || which > 4) return MIC_ERR_ARGS;
    const MicUnit &u = s->h_units[(size_t)i];
    const void *slabs[5] = { u.state_tab, u.tt_nb, u.tt_find, u.tab_sym, u.norm };
    if (bytes > (size_t)u.tab_cap * (which == 3 ? 2 : 4)) return MIC_ERR_ARGS;
    { const int arc = s->activate(); if (arc) return arc; }
    if (bytes) HIP_TRY(hipMemcpy(dst, slabs[which], bytes, hipMemcpyDeviceToHost));
    return MIC_OK;
} MIC_ABI_CATCH
// debug doors (not in the public header): many bare FSE units side by side in ONE launch chain of the caller's session, laid out in
// tier 2 as mic_hip_fse_compress_u16_ex / mic_hip_fse_decompress_u16_ex lay out their one (tests/test_gpu_table_routes.py).
// Encode: unit i codes counts[i] symbols from d_symbols + sym_off[i] with FSECompressU16* semantics (mode 1, no fallback chain),
// flavour flavours[i], ScratchU16.TableLog req_tl[i]; mic_hip_session_encode_finish then returns blobs, offsets and statuses.
static int debug_fse_encode_enqueue(mic_hip_session *s, const uint16_t *d_symbols, const uint64_t *sym_off, const uint32_t *counts,
                                   const int32_t *flavours, const int32_t *req_tl, int n, bool chain) {
    if (!s || !d_symbols || !sym_off || !counts || !flavours || !req_tl || n <= 0 || n > 65535) return MIC_ERR_ARGS;
    size_t most = 0;
    for (int i = 0; i < n; i++) {
        const int f = flavours[i];
        if (!(f == 1 || f == 2 || f == 4 || f == 8 || (f == 108 && !chain)) || req_tl[i] < 0 || req_tl[i] > MIC_MAX_TABLELOG) return MIC_ERR_ARGS;
        if (counts[i] == 0 || counts[i] > (1u << 30)) return MIC_ERR_ARGS;
        most = std::max(most, (size_t)counts[i]);
    }
    int rc = s->activate();
    if (rc) return rc;
    s->retry.kind = 0;
    if ((rc = s->lay_out(n, (most + 3) / 4 + 16))) return rc;
    for (int i = 0; i < n; i++) {
        MicUnit &u = s->h_units[(size_t)i];
        u.px_in = d_symbols + sym_off[i]; u.w = (int32_t)counts[i]; u.h = 1; u.max_value = 0;
        u.nstates = (uint16_t)flavours[i]; u.mode = 1; u.no_fallback = chain ? 0u : 1u; u.req_tl = (uint32_t)req_tl[i];
    }
    return s->run_encode([&] { mic_launch_encode((MicUnit *)s->units.p, n, s->stream, s->variant, nullptr); });
}
int mic_hip_debug_fse_encode_enqueue(mic_hip_session *s, const uint16_t *d_symbols, const uint64_t *sym_off, const uint32_t *counts,
                                     const int32_t *flavours, const int32_t *req_tl, int n) try {
    return debug_fse_encode_enqueue(s, d_symbols, sym_off, counts, flavours, req_tl, n, false);
} MIC_ABI_CATCH
// The same door with the fallback chain of CompressSingleFrame* behind the table stage (no_fallback = 0: N -> N / 2 -> ... -> 1 over
// one table, as k_enc_tans_wg runs it for frames), so that bare token streams can take the two-state instance's hand-over; flavour
// 108 is not taken (the chain has no rANS member).  tests/test_gpu_tans_encode.py.
int mic_hip_debug_fse_encode_chain_enqueue(mic_hip_session *s, const uint16_t *d_symbols, const uint64_t *sym_off, const uint32_t *counts,
                                           const int32_t *flavours, const int32_t *req_tl, int n) try {
    return debug_fse_encode_enqueue(s, d_symbols, sym_off, counts, flavours, req_tl, n, true);
} MIC_ABI_CATCH
// Decode: unit i is the FSE stream at d_blobs + [begins[i], ends[i]) (FSEDecompressU16Auto), at most caps[i] symbols;
// mic_hip_session_decode_finish returns the statuses, mic_hip_debug_unit the counts and mic_hip_debug_fetch_tok the symbols.
int mic_hip_debug_fse_decode_enqueue(mic_hip_session *s, const uint8_t *d_blobs, const uint64_t *begins, const uint64_t *ends,
                                     const uint32_t *caps, int n) try {
    if (!s || !d_blobs || !begins || !ends || !caps || n <= 0 || n > 65535) return MIC_ERR_ARGS;
    size_t most = 0;
    for (int i = 0; i < n; i++) {
        if (ends[i] <= begins[i] || ends[i] - begins[i] > 0xFFFFFFF0ull || caps[i] > (1u << 30)) return MIC_ERR_ARGS;
        most = std::max(most, (size_t)caps[i]);
    }
    int rc = s->activate();
    if (rc) return rc;
    s->retry.kind = 0;
    if ((rc = s->lay_out(n, (most + 3) / 4 + 16))) return rc;
    for (int i = 0; i < n; i++) {
        MicUnit &u = s->h_units[(size_t)i];
        u.comp_in = d_blobs + begins[i]; u.comp_len = (uint32_t)(ends[i] - begins[i]); u.w = 1; u.h = 1; u.mode = 1;
        u.tok_cap = (uint32_t)std::min<size_t>(caps[i], u.tok_cap);
    }
    return s->run_decode(mic_hip_session::FlagSlab::Idle, [&] {
        mic_launch_decode((MicUnit *)s->units.p, n, s->stream, s->variant, nullptr, (int *)s->cls.p); });
} MIC_ABI_CATCH
int mic_hip_session_set_timing(mic_hip_session *s, int enabled) try {
    if (!s) return MIC_ERR_ARGS;
    s->timer.enabled = enabled != 0;
    s->timer.accumulate = enabled == 2;                                   // 2: sum over every launch chain until the next set_timing
    s->timer.clear();
    return MIC_OK;
} MIC_ABI_CATCH
int mic_hip_session_last_timings(mic_hip_session *s, const char **names, float *ms, int cap) try {
    if (!s) return 0;
    s->t_names.clear(); s->t_ms.clear();
    if (s->timer.used >= 2) {
        if (hipEventSynchronize(s->timer.pool[s->timer.used - 1]) != hipSuccess) return 0;
        for (size_t i = 0; i + 1 < s->timer.used; i++) {
            if (strcmp(s->timer.names[i], "end") == 0) continue;           // the gap between two launch chains
            float v = 0.f;
            if (hipEventElapsedTime(&v, s->timer.pool[i], s->timer.pool[i + 1]) != hipSuccess) v = -1.f;
            size_t k = 0;
            while (k < s->t_names.size() && s->t_names[k] != s->timer.names[i]) k++;
            if (k == s->t_names.size()) { s->t_names.push_back(s->timer.names[i]); s->t_ms.push_back(v); }
            else s->t_ms[k] += v;
        }
    }
    int n = (int)std::min<size_t>(s->t_names.size(), (size_t)std::max(cap, 0));
    for (int i = 0; i < n; i++) { names[i] = s->t_names[(size_t)i].c_str(); ms[i] = s->t_ms[(size_t)i]; }
    return n;
} MIC_ABI_CATCH

}  // extern "C"
