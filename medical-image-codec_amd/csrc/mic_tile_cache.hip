// mic_tile_cache.hip -- the tile cache object of the MIC3 patch readers (include/mic_hip.h: mic_hip_tile_cache_*): creation, the
// arena, statistics, and the policy over a trace.  The index and its policy are SlotIndex (mic_tile_cache.h); what a patch call does
// with a cache is in mic_api_ext.hip (read_patches), the kernels that read and write slots in mic_gather.hip.
#include "mic_session.h"
#include "mic_tile_cache.h"

#include <atomic>
#include <memory>

namespace micapi {
uint64_t tile_cache_new_owner() {
    static std::atomic<uint64_t> next{ 1 };
    return next.fetch_add(1);
}
}  // namespace micapi

namespace {
// The slide formats compressTileBlob codes with WSIOptions.defaults, as mic_hip_wsi_compress_ex judges them (wsi_options, mic_api_ext.hip)
int slot_format(int tile_w, int tile_h, int channels, int bits_per_sample, int *tw, int *th, uint64_t *bytes) {
    if (tile_w < 0 || tile_h < 0) return MIC_ERR_ARGS;
    if (!((channels == 3 && bits_per_sample == 8) || (channels == 1 && (bits_per_sample == 8 || bits_per_sample == 16)))) return MIC_ERR_UNSUPPORTED;
    *tw = tile_w ? tile_w : 256; *th = tile_h ? tile_h : 256;
    if ((size_t)*tw * (size_t)*th > ((size_t)1 << 26)) return MIC_ERR_UNSUPPORTED;
    const uint64_t px = (uint64_t)*tw * (uint64_t)*th * (uint64_t)channels * (bits_per_sample == 16 ? 2u : 1u);
    *bytes = (px + 255) / 256 * 256;
    return MIC_OK;
}
}  // namespace

int mic_hip_tile_cache::ensure_arena(int dev, bool *usable) {
    *usable = false;
    if (arena) { *usable = device == dev; return MIC_OK; }
    if (index.nslots() == 0) { *usable = true; return MIC_OK; }                          // (keeps nothing: every tile is bypassed)
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, (size_t)(index.nslots() * slot_bytes));
    if (e != hipSuccess) { (void)hipGetLastError(); return e == hipErrorOutOfMemory ? MIC_ERR_NOMEM : MIC_ERR_DEVICE; }
    arena = p; device = dev;
    *usable = true;
    return MIC_OK;
}

void mic_hip_tile_cache::detach(uint64_t owner) {
    std::lock_guard<std::mutex> lk(mu);
    index.drop_owner(owner);
    if (attached) attached--;
}

void mic_tile_cache_detach(mic_hip_tile_cache *c, uint64_t owner) { if (c) c->detach(owner); }

extern "C" {

int mic_hip_tile_cache_slot_bytes(int tile_w, int tile_h, int channels, int bits_per_sample, uint64_t *bytes) try {
    if (!bytes) return MIC_ERR_ARGS;
    int tw = 0, th = 0;
    return slot_format(tile_w, tile_h, channels, bits_per_sample, &tw, &th, bytes);
} MIC_ABI_CATCH

int mic_hip_tile_cache_create(int tile_w, int tile_h, int channels, int bits_per_sample, uint64_t nslots, mic_hip_tile_cache **c) try {
    if (!c) return MIC_ERR_ARGS;
    *c = nullptr;
    int tw = 0, th = 0; uint64_t sb = 0;
    const int rc = slot_format(tile_w, tile_h, channels, bits_per_sample, &tw, &th, &sb);
    if (rc) return rc;
    if (nslots >= micapi::SlotIndex::kNoSlot || (nslots && sb > (uint64_t)SIZE_MAX / nslots)) return MIC_ERR_UNSUPPORTED;
    *c = new mic_hip_tile_cache(tw, th, channels, bits_per_sample, sb, nslots);
    return MIC_OK;
} MIC_ABI_CATCH

// a cache of reconstructed MIC2 frames: the same object, a slot one frame of width x height u16 samples (mic2_crop_args' limits)
int mic_hip_frame_cache_slot_bytes(int width, int height, uint64_t *bytes) try {
    if (!bytes || width <= 0 || height <= 0) return MIC_ERR_ARGS;
    if ((size_t)width * (size_t)height > ((size_t)1 << 28)) return MIC_ERR_UNSUPPORTED;
    *bytes = ((uint64_t)width * (uint64_t)height * 2 + 255) / 256 * 256;
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_frame_cache_create(int width, int height, uint64_t nslots, mic_hip_tile_cache **c) try {
    if (!c) return MIC_ERR_ARGS;
    *c = nullptr;
    uint64_t sb = 0;
    const int rc = mic_hip_frame_cache_slot_bytes(width, height, &sb);
    if (rc) return rc;
    if (nslots >= micapi::SlotIndex::kNoSlot || (nslots && sb > (uint64_t)SIZE_MAX / nslots)) return MIC_ERR_UNSUPPORTED;
    *c = new mic_hip_tile_cache(width, height, 1, 16, sb, nslots);
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_tile_cache_clear(mic_hip_tile_cache *c) try {
    if (!c) return MIC_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    c->index.clear();
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_tile_cache_get_stats(const mic_hip_tile_cache *c, mic_hip_tile_cache_stats *st) try {
    if (!c || !st) return MIC_ERR_ARGS;
    mic_hip_tile_cache *m = const_cast<mic_hip_tile_cache *>(c);
    std::lock_guard<std::mutex> lk(m->mu);
    const micapi::SlotIndex::Counters &k = c->index.counters();
    *st = mic_hip_tile_cache_stats{ c->index.nslots(), c->index.resident(), k.hits, k.misses, k.bypassed, k.evictions, k.calls,
                                    c->arena ? c->index.nslots() * c->slot_bytes : 0 };
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_tile_cache_destroy(mic_hip_tile_cache *c) try {
    if (!c) return MIC_OK;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (c->attached) return MIC_ERR_ARGS;
    }
    if (c->arena) {
        int cur = -1;
        const bool back = hipGetDevice(&cur) == hipSuccess && cur != c->device;
        if (hipSetDevice(c->device) == hipSuccess) (void)hipFree(c->arena);
        if (back) (void)hipSetDevice(cur);
        (void)hipGetLastError();
    }
    delete c;
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_tile_cache_plan(uint64_t nslots, const uint64_t *keys, const uint32_t *call_len, int ncalls, uint8_t *outcome, uint64_t *evictions) try {
    if (ncalls < 0 || (ncalls > 0 && !call_len) || nslots >= micapi::SlotIndex::kNoSlot) return MIC_ERR_ARGS;
    uint64_t total = 0;
    for (int k = 0; k < ncalls; k++) total += call_len[k];
    if (total && (!keys || !outcome)) return MIC_ERR_ARGS;
    micapi::SlotIndex index(nslots);
    std::vector<micapi::SlotIndex::Key> call; std::vector<uint32_t> slot;
    uint64_t at = 0;
    for (int k = 0; k < ncalls; k++) {
        const size_t n = call_len[k];
        call.resize(n); slot.resize(n);
        for (size_t i = 0; i < n; i++) {
            if (i && keys[at + i] <= keys[at + i - 1]) return MIC_ERR_ARGS;               // (distinct and ascending: a plan's order)
            call[i] = micapi::SlotIndex::Key{ 0, keys[at + i] };
        }
        index.plan(call.data(), n, outcome + at, slot.data());
        index.commit();
        at += n;
    }
    if (evictions) *evictions = index.counters().evictions;
    return MIC_OK;
} MIC_ABI_CATCH

}  // extern "C"
