// mic_tile_cache.h -- a cache of decoded units in device memory (MIC3 tiles: mic_api_ext.hip; reconstructed MIC2 frames:
// mic_mic2_crops.hip).  Two things live here:
// SlotIndex, the host-side index and replacement policy, which knows nothing of containers or devices (a key is an owner and a unit
// number), and mic_hip_tile_cache, the object behind the C ABI: one SlotIndex, one arena of equal slots, one mutex.
//
// The policy, so that a host model can predict it.  Each call that uses the index gets the next call number.
//   1. The call's keys are walked in the caller's order; a resident key is a hit and is stamped with the call number.
//   2. Each miss, in the same order, takes the lowest-numbered free slot; else the entry with the smallest stamp below the call's
//      number (ties: the lowest slot), which is evicted; else -- every slot is stamped by this call -- it is bypassed.
//   3. release() frees an entry of the call whose unit turned out bad.
//   4. rollback() puts everything back as it was before plan(): entries, stamps, counters and the call number.
#pragma once
#include <algorithm>
#include <cstdint>
#include <mutex>
#include <unordered_map>
#include <vector>

namespace micapi {

class SlotIndex {
public:
    struct Key { uint64_t owner, unit; bool operator==(const Key &o) const { return owner == o.owner && unit == o.unit; } };
    enum Outcome : uint8_t { kHit = 0, kMiss = 1, kBypass = 2 };
    struct Counters { uint64_t hits = 0, misses = 0, bypassed = 0, evictions = 0, calls = 0; };
    static constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

    explicit SlotIndex(uint64_t nslots) : slots_((size_t)nslots) {}
    uint64_t nslots() const { return slots_.size(); }
    uint64_t resident() const { return map_.size(); }
    const Counters &counters() const { return cnt_; }
    bool has(const Key &k) const { return map_.find(k) != map_.end(); }
    uint32_t slot_of(const Key &k) const { const auto it = map_.find(k); return it == map_.end() ? kNoSlot : it->second; }   // (changes no state)

    // One call: n distinct keys in the caller's order -> outcome[i] and, for a hit or a miss, slot[i] (kNoSlot for a bypass).
    // What it changes is journalled until commit() or rollback().
    void plan(const Key *keys, size_t n, uint8_t *outcome, uint32_t *slot) {
        begin_ = cnt_;
        journal_.clear();
        const uint64_t call = ++cnt_.calls;
        size_t nmiss = 0;
        for (size_t i = 0; i < n; i++) {
            const auto it = map_.find(keys[i]);
            if (it == map_.end()) { outcome[i] = kMiss; slot[i] = kNoSlot; nmiss++; continue; }
            Slot &s = slots_[it->second];
            journal_.push_back(Undo{ it->second, s });
            s.stamp = call;
            outcome[i] = kHit; slot[i] = it->second;
            cnt_.hits++;
        }
        if (!nmiss) return;
        // the slots a miss may take, in the order of preference: free ones by number, then entries by (stamp, number)
        std::vector<uint32_t> cand;
        for (uint32_t q = 0; q < slots_.size(); q++) if (!slots_[q].used) cand.push_back(q);
        const size_t nfree = cand.size();
        if (nfree < nmiss) {
            for (uint32_t q = 0; q < slots_.size(); q++) if (slots_[q].used && slots_[q].stamp < call) cand.push_back(q);
            std::sort(cand.begin() + (long)nfree, cand.end(), [&](uint32_t a, uint32_t b) {
                return slots_[a].stamp != slots_[b].stamp ? slots_[a].stamp < slots_[b].stamp : a < b;
            });
        }
        size_t next = 0;
        for (size_t i = 0; i < n; i++) {
            if (outcome[i] != kMiss) continue;
            if (next == cand.size()) { outcome[i] = kBypass; cnt_.bypassed++; continue; }
            const uint32_t q = cand[next++];
            Slot &s = slots_[q];
            journal_.push_back(Undo{ q, s });
            if (s.used) { map_.erase(s.key); cnt_.evictions++; }
            s = Slot{ keys[i], call, true };
            map_[keys[i]] = q;
            slot[i] = q;
            cnt_.misses++;
        }
    }
    // a call that cannot use the index (its arena lives on another device): its n units are decoded and not kept; no call number
    void bypass_all(size_t n) { begin_ = cnt_; journal_.clear(); cnt_.bypassed += n; }
    // slot q's contents are no longer what the index says (a call that failed had begun to write it): whatever it holds is dropped
    void spoil(uint32_t q) { Slot &s = slots_[q]; if (s.used) map_.erase(s.key); s = Slot(); }
    void commit() { journal_.clear(); }
    void rollback() {
        for (size_t j = journal_.size(); j-- > 0;) {
            Slot &s = slots_[journal_[j].slot];
            if (s.used) map_.erase(s.key);
            s = journal_[j].was;
            if (s.used) map_[s.key] = journal_[j].slot;
        }
        journal_.clear();
        cnt_ = begin_;
    }
    // an entry this call made whose unit is bad: it was decoded and is not kept
    void release(const Key &k) {
        const auto it = map_.find(k);
        if (it == map_.end()) return;
        slots_[it->second] = Slot();
        map_.erase(it);
        cnt_.misses--; cnt_.bypassed++;
    }
    void drop_owner(uint64_t owner) {
        for (Slot &s : slots_) if (s.used && s.key.owner == owner) { map_.erase(s.key); s = Slot(); }
    }
    void clear() { for (Slot &s : slots_) s = Slot(); map_.clear(); }

private:
    struct Slot { Key key{ 0, 0 }; uint64_t stamp = 0; bool used = false; };
    struct Undo { uint32_t slot; Slot was; };
    struct Hash { size_t operator()(const Key &k) const { return (size_t)((k.owner * 0x9E3779B97F4A7C15ull) ^ (k.unit * 0xC2B2AE3D27D4EB4Full + (k.owner >> 17))); } };
    std::vector<Slot> slots_;
    std::unordered_map<Key, uint32_t, Hash> map_;
    Counters cnt_, begin_;
    std::vector<Undo> journal_;
};

uint64_t tile_cache_new_owner();                     // an owner number no other reader or store generation has (mic_tile_cache.hip)

}  // namespace micapi

// The object behind mic_hip_tile_cache_*.  mu guards everything below it; a patch call holds it from its planning to its final
// stream synchronise, so a slot is never read on one stream while another call's stream writes it.
struct mic_hip_tile_cache {
    std::mutex mu;
    int tw, th, channels, bps;
    uint64_t slot_bytes;
    micapi::SlotIndex index;
    void *arena = nullptr; int device = -1;           // one allocation of nslots * slot_bytes, made by the first call that uses the cache
    uint64_t attached = 0;                             // readers and sessions that hold this cache
    mic_hip_tile_cache(int tw_, int th_, int ch, int bps_, uint64_t sb, uint64_t nslots) : tw(tw_), th(th_), channels(ch), bps(bps_), slot_bytes(sb), index(nslots) {}
    // the arena on `dev` for a call there: MIC_OK and *usable = whether the call may use the cache (false: it lives on another
    // device); the allocation's own code when it fails.  Call with mu held and `dev` current.
    int ensure_arena(int dev, bool *usable);
    // an owner lets go: its entries are dropped (mu is taken here)
    void detach(uint64_t owner);
};
// mic_hip_session's hook (mic_session.h): detaches the session's store from its cache
void mic_tile_cache_detach(mic_hip_tile_cache *c, uint64_t owner);
